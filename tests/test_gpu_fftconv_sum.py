"""GPU tier (-m gpu): fftConv.inputChannels, the sum over input channels, through the C ABI.

The tables and their bars are fftconv_sum_cases.py's, shared with the CPU tier.  On the device as well: more work items than resident workgroups
(the tile kernel's grid-stride loop over work items with the channel loop inside), the kernel-list form of Plan.exec and its length errors, and the
exec contract and replay (test_gpu_exec_contract.py's harness) on dense, strided and composed requests."""
import numpy as np
import pytest

import fftconv_ols_scaffold as scaffold
import fftconv_sum_cases as sums
import test_gpu_exec_contract as contract
from test_emu_fftconv_real import _rel
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sums.TILE_CASES + sums.COMPOSED_CASES, ids=repr)
def test_sum_over_input_channels(fft, dev, oracle, monkeypatch, case):
    sums.check_case(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, case)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch, real):
    sums.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, real)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_the_composed_route_agrees_with_the_tile_route(fft, dev, monkeypatch, real):
    run, setenv = scaffold.gpu_runner(fft, dev, monkeypatch)
    case = next(c for c in sums.TILE_CASES if c.real == real)
    x, h, want = sums.data(case)
    setenv(sums.SWITCH, "64")
    tile, route, _ = run(case.opts, x, want.size, h)
    setenv(sums.SWITCH, "0")
    composed, route0, _ = run(case.opts, x, want.size, h)
    assert case.tag in route and sums.composed_tag(real, case.K, case.C) in route0 and "ols-sum" not in route0, (route, route0)
    rel = _rel(tile, composed)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= sums.PARITY_BAR


@pytest.mark.parametrize("real,shape,ks,batch,K,boundary,env", sums.C1_CASES, ids=lambda v: None)
def test_one_channel_is_the_request_without_the_option(fft, dev, monkeypatch, real, shape, ks, batch, K, boundary, env):
    run, setenv = scaffold.gpu_runner(fft, dev, monkeypatch)
    for name, value in env.items():
        setenv(name, value)
    rand = sums._route(real).rand
    x, h = rand(int(np.prod(shape)) * batch, 0x5C11), rand(int(np.prod(ks)) * K, 0x5C12)
    out_shape = [n + k - 1 if boundary == "linear-full" else n for n, k in zip(shape, ks)]
    out_floats = int(np.prod(out_shape)) * batch * K * (1 if real else 2)
    plain = run(sums.options(real, shape, ks, batch, None, K, boundary=boundary), x, out_floats, h)
    one = run(sums.options(real, shape, ks, batch, 1, K, boundary=boundary), x, out_floats, h)
    assert plain[1:] == one[1:], (plain[1:], one[1:])
    assert "-sum" not in one[1], one[1]
    assert np.array_equal(np.asarray(plain[0]).view(np.uint32), np.asarray(one[0]).view(np.uint32))


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_more_work_items_than_resident_workgroups(fft, dev, monkeypatch, real):
    """70 x 70 (*) 9 x 9, batch 300, C = 2: L = 56 x 56 on the domain 78 x 78, 2 x 2 tiles an image: 1200 work items (600 real pairs) a launch against at most
    1024 resident workgroups of the 64-point tile.  The first, a middle and the last item against float64"""
    shape, ks, batch, C = (70, 70), (9, 9), 300, 2
    n, kn = shape[0] * shape[1], ks[0] * ks[1]
    rand = sums._route(real).rand
    x, h = rand(n * batch * C, 0x5C21), rand(kn * C, 0x5C22)
    run, setenv = scaffold.gpu_runner(fft, dev, monkeypatch)
    setenv(sums.SWITCH, "64")
    width = 1 if real else 2
    got, route, launches = run(sums.options(real, shape, ks, batch, C), x, n * batch * width, h)
    assert sums.tile_tag(real, 64, ks, C) in route and launches == 2, (route, launches)
    got = np.asarray(got).reshape(batch, n * width)
    per = n * C * width
    for b in (0, 149, batch - 1):
        want = sums.reference(real, shape, ks, 1, C, 1, "convolution", "linear-same", None, x[b * per:(b + 1) * per], h).reshape(-1)
        err = np.abs(got[b] - want)
        rel = _rel(got[b], want)
        print(f"{route.strip()} item {b}: rel_l2={rel:.3e} max_abs={err.max():.3e}")
        assert np.all(err <= sums.ATOL + sums.RTOL * np.abs(want)) and rel <= sums.F64_BAR, (b, rel)


def test_kernel_arrays(fft, dev):
    """Plan.exec takes the packed array of kernelCount * C kernels or a list of that many; the length errors name both counts"""
    case = next(c for c in sums.COMPOSED_CASES if c.shape == (1000,) and not c.real)
    x, h, want = sums.data(case)
    kn = 2 * case.ks[0]
    plan = fft.createPlan(dev, case.opts)
    assert sums.composed_tag(False, case.K, case.C) in plan.describe()[0]
    inp = dev.createBuffer({"size": x.nbytes})
    dev.queue.writeBuffer(inp, 0, x)
    out = dev.createBuffer({"size": 4 * want.size})
    for kernel in (h, [h[i * kn:(i + 1) * kn] for i in range(case.K * case.C)]):
        enc = dev.createCommandEncoder()
        plan.exec(enc, {"input": inp, "output": out, "kernel": kernel})
        dev.queue.submit([enc.finish()])
        dev.queue.onSubmittedWorkDone()
        assert _rel(fft.downloadF32(dev, out, want.size), want) <= sums.F64_BAR
    enc = dev.createCommandEncoder()
    with pytest.raises(fft.Mi355Error, match=r"kernel array length must equal fftConv.kernelCount=2 x inputChannels=3; got 2"):
        plan.exec(enc, {"input": inp, "output": out, "kernel": [h[:kn], h[kn:2 * kn]]})
    with pytest.raises(fft.Mi355Error, match=r"kernel Float32Array length must be 372 for kernelCount=2 x inputChannels=3; got 124"):
        plan.exec(enc, {"input": inp, "output": out, "kernel": h[:2 * kn]})
    small = dev.createBuffer({"size": x.nbytes // case.C})
    with pytest.raises(fft.Mi355Error):      # the input side covers batch * C lines
        plan.exec(enc, {"input": small, "output": out, "kernel": h})
    for b in (inp, out, small):
        b.destroy()
    plan.destroy()


def test_planning_errors(fft, dev):
    with pytest.raises(Exception, match="fftConv.inputChannels must be a positive integer"):
        fft.createPlan(dev, sums.options(False, (64, 48), (5, 5), 2, 0))
    with pytest.raises(Exception) as e:
        fft.createPlan(dev, sums.options(True, (63, 48), (5, 5), 2, 2, boundary="circular"))
    assert sums.UNSUPPORTED_ODD in str(e.value), e.value


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", sums.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", sums.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
