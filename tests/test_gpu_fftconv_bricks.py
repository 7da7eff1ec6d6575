"""GPU tier (-m gpu): the overlap-save brick route of rank-3 complex fftconv (bricks-conv-ols[N=16x16x16,L=L0xL1xL2]) through the C ABI.

The case table and its bars are fftconv_bricks_cases.py's, shared with the CPU tier.  On the device as well: the capability the route adds
(2 volumes of 128^3 points under a 5^3 kernel) against float64 direct sums on windows at a volume's corner, across a brick seam on each axis,
at a triple seam and at the far corner, a plan destroyed, created again and run twice, the accuracy ladder, and the exec contract and replay
(test_gpu_exec_contract.py's harness) on a dense and a strided request."""
import numpy as np
import pytest

import fftconv_bricks_cases as bricks
import fftconv_ols_scaffold as scaffold
import test_gpu_accuracy as accuracy
import test_gpu_exec_contract as contract
from test_emu_fftconv_real import _rel
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)
from test_gpu_parity import run_plan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", bricks.CASES, ids=repr)
def test_overlap_save_bricks(fft, dev, oracle, monkeypatch, case):
    bricks.ROUTE.check_case(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch):
    bricks.ROUTE.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle)


def capability_windows(shape, ks, L):
    """the low corners of the 24^3 windows: the origin corner, across a brick seam on each axis alone, at a triple seam, the far corner.  A seam is
    the output index of the first result of a brick: j L - (M - 1) // 2; every window is 24 = 2 L wide at L = 12 and so holds two seams an axis"""
    seam = [5 * l - (m - 1) // 2 for l, m in zip(L, ks)]
    mid = [n // 2 + 3 for n in shape]
    return ((0, 0, 0), (seam[0] - 12, mid[1], mid[2]), (mid[0], seam[1] - 12, mid[2]), (mid[0], mid[1], seam[2] - 12),
            tuple(s - 12 for s in seam), tuple(n - 24 for n in shape))


def test_capability_volumes_of_128_cubed_points(fft, dev, monkeypatch):
    """2 x 128^3 (*) 5^3 linear-same (32 MiB each way): windows of 24^3 outputs of the first and the last volume against float64 direct sums"""
    shape, ks, batch = (128, 128, 128), (5, 5, 5), 2
    n = int(np.prod(shape))
    x, h = bricks.ROUTE.rand(n * batch, 0xB3F1), bricks.ROUTE.rand(int(np.prod(ks)), 0xB3F2)
    monkeypatch.setenv("MI355FFT_" + bricks.ROUTE.switch, "16")
    got, (route, launches) = run_plan(fft, dev, scaffold.options(shape, ks, batch), x, 2 * n * batch, kernel=h)
    assert bricks.ROUTE.tag_of(16, ks) in route and launches == 2 and not any(f in route for f in bricks.ROUTE.forbidden), (route, launches)
    got = got.reshape((batch,) + shape[::-1] + (2,))
    for b in (0, batch - 1):
        for lo in capability_windows(shape, ks, (12, 12, 12)):
            hi = tuple(v + 24 for v in lo)
            want = bricks.ROUTE.direct_same_conv(x[2 * n * b:2 * n * (b + 1)], h, shape, ks, lo, hi)
            w = got[b, lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
            g = w[..., 0].astype(np.float64) + 1j * w[..., 1]
            err = np.abs(g - want)
            rel = float(np.linalg.norm(g - want) / np.linalg.norm(want))
            print(f"{route.strip()} volume {b} outputs {lo}..{hi}: rel_l2={rel:.3e} max_abs={err.max():.3e}")
            assert np.all(err <= 4e-3 + 4e-3 * np.abs(want)) and rel <= 1e-5, (b, lo, rel)


def test_plan_destroyed_and_created_again(fft, dev, monkeypatch):
    """the first case of the table: create, exec, destroy, create again, exec twice into one buffer"""
    case = bricks.CASES[0]
    x, h, want = bricks.ROUTE.data(case)
    monkeypatch.setenv("MI355FFT_" + bricks.ROUTE.switch, str(case.P))
    inp, out = fft.uploadComplex(dev, x), dev.createBuffer({"size": 4 * want.size})
    for round_, execs in enumerate((1, 2)):
        plan = fft.createPlan(dev, case.opts)
        bricks.ROUTE.assert_route(case, *plan.describe())
        for _ in range(execs):
            enc = dev.createCommandEncoder()
            plan.exec(enc, {"input": inp, "output": out, "kernel": h})
            dev.queue.submit([enc.finish()])
            dev.queue.onSubmittedWorkDone()
            got = fft.downloadComplex(dev, out, want.size // 2).reshape(-1)
            assert _rel(got, want) <= 1e-5, round_
        plan.destroy()
    inp.destroy()
    out.destroy()


# ---- accuracy ladder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", bricks.ACCURACY_CASES, ids=repr)
def test_accuracy(fft, dev, oracle, monkeypatch, case):
    accuracy.test_accuracy(fft, dev, oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", bricks.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", bricks.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
