"""GPU tier (-m gpu): the overlap-save brick route of rank-3 real fftconv (bricks-rconv-ols[N=16x16x16,L=L0xL1xL2]) through the C ABI.

The case table and its bars are fftconv_rbricks_cases.py's, shared with the CPU tier.  On the device as well: the capability the route adds
(2 real volumes of 128^3 points under a 5^3 kernel) against float64 direct sums on windows at a volume's corner, across a brick seam on each
axis (on axis 2 a window holds the seam between the two partners of a pair and the seam between two pairs), at a triple seam and at the far
corner; a plan destroyed, created again and run twice; the accuracy ladder; and the exec contract and replay (test_gpu_exec_contract.py's
harness) on a dense and a strided request."""
import numpy as np
import pytest

import fftconv_ols_scaffold as scaffold
import fftconv_rbricks_cases as rbricks
import test_gpu_accuracy as accuracy
import test_gpu_exec_contract as contract
from test_emu_fftconv_real import _opts, _rand, _rel
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)
from test_gpu_fftconv_bricks import capability_windows
from test_gpu_parity import run_plan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", rbricks.CASES, ids=repr)
def test_overlap_save_real_bricks(fft, dev, oracle, monkeypatch, case):
    rbricks.ROUTE.check_case(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch):
    def unsupported(opts):
        with pytest.raises(Exception) as e:
            fft.createPlan(dev, opts)
        assert rbricks.UNSUPPORTED in str(e.value), e.value
    rbricks.ROUTE.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, unsupported)


def test_capability_volumes_of_128_cubed_points(fft, dev, monkeypatch):
    """2 x 128^3 (*) 5^3 linear-same (16 MiB each way): windows of 24^3 outputs of the first and the last volume against float64 direct sums"""
    shape, ks, batch = (128, 128, 128), (5, 5, 5), 2
    n = int(np.prod(shape))
    x, h = _rand(n * batch, 0x4BF1), _rand(int(np.prod(ks)), 0x4BF2)
    monkeypatch.setenv("MI355FFT_" + rbricks.ROUTE.switch, "16")
    got, (route, launches) = run_plan(fft, dev, _opts(list(shape), list(ks), batch, boundary="linear-same"), x, n * batch, kernel=h)
    assert rbricks.ROUTE.tag_of(16, ks) in route and launches == 2 and not any(f in route for f in rbricks.ROUTE.forbidden), (route, launches)
    got = np.asarray(got).reshape((batch,) + shape[::-1])
    for b in (0, batch - 1):
        for lo in capability_windows(shape, ks, (12, 12, 12)):
            hi = tuple(v + 24 for v in lo)
            want = rbricks.ROUTE.direct_same_conv(x[n * b:n * (b + 1)], h, shape, ks, lo, hi)
            g = got[b, lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].astype(np.float64)
            err = np.abs(g - want)
            rel = float(np.linalg.norm(g - want) / np.linalg.norm(want))
            print(f"{route.strip()} volume {b} outputs {lo}..{hi}: rel_l2={rel:.3e} max_abs={err.max():.3e}")
            assert np.all(err <= 4e-3 + 4e-3 * np.abs(want)) and rel <= 1e-5, (b, lo, rel)


def test_plan_destroyed_and_created_again(fft, dev, monkeypatch):
    """the first case of the table: create, exec, destroy, create again, exec twice into one buffer"""
    case = rbricks.CASES[0]
    x, h, want = rbricks.ROUTE.data(case)
    monkeypatch.setenv("MI355FFT_" + rbricks.ROUTE.switch, str(case.P))
    inp = dev.createBuffer({"size": x.nbytes})
    dev.queue.writeBuffer(inp, 0, x)
    out = dev.createBuffer({"size": 4 * want.size})
    for round_, execs in enumerate((1, 2)):
        plan = fft.createPlan(dev, case.opts)
        rbricks.ROUTE.assert_route(case, *plan.describe())
        for _ in range(execs):
            enc = dev.createCommandEncoder()
            plan.exec(enc, {"input": inp, "output": out, "kernel": h})
            dev.queue.submit([enc.finish()])
            dev.queue.onSubmittedWorkDone()
            got = fft.downloadF32(dev, out, want.size)
            assert _rel(got, want.reshape(-1)) <= 1e-5, round_
        plan.destroy()
    inp.destroy()
    out.destroy()


# ---- accuracy ladder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", rbricks.ACCURACY_CASES, ids=repr)
def test_accuracy(fft, dev, oracle, monkeypatch, case):
    accuracy.test_accuracy(fft, dev, oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", rbricks.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", rbricks.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
