"""GPU tier (-m gpu): fftConv.groups, grouped and depthwise convolution, through the C ABI.

The tables and their bars are fftconv_group_cases.py's, shared with the CPU tier.  On the device as well: more work items than resident workgroups (the
grouped kernel's grid-stride loop over (image, kernel, tile) items), the kernel-list form of Plan.exec and its length errors, and the exec contract and
replay (test_gpu_exec_contract.py's harness) on grouped dense, grouped strided and depthwise-by-map requests."""
import numpy as np
import pytest

import fftconv_group_cases as groups
import fftconv_ols_scaffold as scaffold
import fftconv_sum_cases as sums
import test_gpu_exec_contract as contract
from test_emu_fftconv_real import _rel
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _runner(fft, dev, monkeypatch):
    run, setenv = scaffold.gpu_runner(fft, dev, monkeypatch)
    return run, setenv, lambda name: monkeypatch.delenv("MI355FFT_" + name, raising=False)


@pytest.mark.parametrize("case", groups.GROUP_CASES + groups.MAP_CASES + groups.COMPOSED_CASES, ids=repr)
def test_grouped_and_depthwise(fft, dev, oracle, monkeypatch, case):
    groups.check_case(*_runner(fft, dev, monkeypatch), oracle, case)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch, real):
    groups.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, real)


@pytest.mark.parametrize("name", ["complex_150x100_k9x5_C4_K4_G2_conv_same", "real_150x130_k9x5_depthwise3_conv_absent_partner"])
def test_the_grouped_kernel_agrees_with_the_switch_at_0(fft, dev, monkeypatch, name):
    run, setenv = scaffold.gpu_runner(fft, dev, monkeypatch)
    case = next(c for c in groups.GROUP_CASES if c.name == name)
    x, h, want = groups.data(case)
    setenv(groups.SWITCH, "64")
    one, route, launches = run(case.opts, x, want.size, h)
    setenv(groups.SWITCH, "0")
    if case.Cg == 1:
        setenv("RCONV_OLS2D" if case.real else "CONV_OLS2D", "64")
    other, route0, launches0 = run(case.opts, x, want.size, h)
    assert case.tag in route and launches == 2 and "-group[" not in route0, (route, route0)
    assert (f",G={case.G}]" in route0 and launches0 == 1 + case.K) if case.Cg == 1 else groups.composed_tag(case.real, case.K, case.C, case.G) in route0, (route0, launches0)
    rel = _rel(one, other)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= groups.PARITY_BAR


@pytest.mark.parametrize("real,shape,ks,batch,C,K,boundary,env", groups.G1_CASES, ids=lambda v: None)
def test_one_group_is_the_request_without_the_option(fft, dev, monkeypatch, real, shape, ks, batch, C, K, boundary, env):
    run, setenv = scaffold.gpu_runner(fft, dev, monkeypatch)
    for name, value in env.items():
        setenv(name, value)
    rand = sums._route(real).rand
    x, h = rand(int(np.prod(shape)) * batch * C, 0x6C11), rand(int(np.prod(ks)) * K * C, 0x6C12)
    out_floats = int(np.prod(shape)) * batch * K * (1 if real else 2)
    plain = run(groups.options(real, shape, ks, batch, C, K, None, boundary=boundary), x, out_floats, h)
    one = run(groups.options(real, shape, ks, batch, C, K, 1, boundary=boundary), x, out_floats, h)
    assert plain[1:] == one[1:], (plain[1:], one[1:])
    assert "G=" not in one[1] and "-group" not in one[1], one[1]
    assert np.array_equal(np.asarray(plain[0]).view(np.uint32), np.asarray(one[0]).view(np.uint32))


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_more_work_items_than_resident_workgroups(fft, dev, monkeypatch, real):
    """70 x 70 (*) 9 x 9, batch 80, depthwise C = K = G = 8: L = 56 x 56 on the domain 78 x 78, 2 x 2 tiles an image: 80 * 8 * 4 = 2560 work items (1280 real pairs) in
    the one launch against at most 1024 resident workgroups of the 64-point tile.  Results (b, k) = (0, 0), (40, 3) and (79, 7) against float64"""
    shape, ks, batch, C = (70, 70), (9, 9), 80, 8
    n, kn = shape[0] * shape[1], ks[0] * ks[1]
    rand = sums._route(real).rand
    x, h = rand(n * batch * C, 0x6C21), rand(kn * C, 0x6C22)
    run, setenv = scaffold.gpu_runner(fft, dev, monkeypatch)
    setenv(groups.SWITCH, "64")
    width = 1 if real else 2
    got, route, launches = run(groups.options(real, shape, ks, batch, C, C, C), x, n * batch * C * width, h)
    assert groups.group_tag(real, ks, C, C, C) in route and launches == 2, (route, launches)
    got = np.asarray(got).reshape(C, batch, n * width)                    # kernel-major
    xs, hs = x.reshape(batch, C, n * width), h.reshape(C, kn * width)
    for b, k in ((0, 0), (40, 3), (batch - 1, C - 1)):
        want = sums.reference(real, shape, ks, 1, 1, 1, "convolution", "linear-same", None, xs[b, k], hs[k]).reshape(-1)
        err = np.abs(got[k, b] - want)
        rel = _rel(got[k, b], want)
        print(f"{route.strip()} result ({b}, {k}): rel_l2={rel:.3e} max_abs={err.max():.3e}")
        assert np.all(err <= sums.ATOL + sums.RTOL * np.abs(want)) and rel <= sums.F64_BAR, (b, k, rel)


def test_kernel_arrays(fft, dev):
    """Plan.exec takes the packed array of kernelCount * C / G kernels or a list of that many; with G > 1 the length errors name the count as
    kernelCount=K x inputChannels/groups=Cg"""
    case = next(c for c in groups.COMPOSED_CASES if c.shape == (1000,) and not c.real)
    x, h, want = groups.data(case)
    kn = 2 * case.ks[0]
    plan = fft.createPlan(dev, case.opts)
    assert case.tag in plan.describe()[0]
    inp = dev.createBuffer({"size": x.nbytes})
    dev.queue.writeBuffer(inp, 0, x)
    out = dev.createBuffer({"size": 4 * want.size})
    for kernel in (h, [h[i * kn:(i + 1) * kn] for i in range(case.K * case.Cg)]):
        enc = dev.createCommandEncoder()
        plan.exec(enc, {"input": inp, "output": out, "kernel": kernel})
        dev.queue.submit([enc.finish()])
        dev.queue.onSubmittedWorkDone()
        assert _rel(fft.downloadF32(dev, out, want.size), want) <= groups.F64_BAR
    enc = dev.createCommandEncoder()
    with pytest.raises(fft.Mi355Error, match=r"kernel array length must equal fftConv.kernelCount=2 x inputChannels/groups=2; got 2"):
        plan.exec(enc, {"input": inp, "output": out, "kernel": [h[:kn], h[kn:2 * kn]]})
    with pytest.raises(fft.Mi355Error, match=r"kernel Float32Array length must be 248 for kernelCount=2 x inputChannels/groups=2; got 124"):
        plan.exec(enc, {"input": inp, "output": out, "kernel": h[:2 * kn]})
    for b in (inp, out):
        b.destroy()
    plan.destroy()


def test_planning_errors(fft, dev):
    with pytest.raises(Exception, match="fftConv.groups must be a positive integer"):
        fft.createPlan(dev, groups.options(False, (64, 48), (5, 5), 2, 4, 4, 0))
    with pytest.raises(Exception, match="fftConv.groups=3 must divide fftConv.inputChannels=4"):
        fft.createPlan(dev, groups.options(False, (64, 48), (5, 5), 2, 4, 6, 3))


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", groups.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", groups.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
