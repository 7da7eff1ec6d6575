"""GPU tier (-m gpu): the overlap-save tile route of rank-2 complex fftconv (tiles-conv-ols[N=PxP,L=L0xL1]) through the C ABI.

The case table and its bars are fftconv_tiles_cases.py's, shared with the CPU tier.  On the device as well: the capability the route adds
(4 images of 1024 x 1024 points under a 9 x 9 kernel: 33 launches and hundreds of MiB of workspace before it) against float64 direct sums on
windows at an image corner, across a tile seam on each axis and at the far corner, a plan destroyed, created again and run twice, the
accuracy ladder, and the exec contract and replay (test_gpu_exec_contract.py's harness) on a dense and a strided request."""
import numpy as np
import pytest

import fftconv_ols_scaffold as scaffold
import fftconv_tiles_cases as tiles
import test_gpu_accuracy as accuracy
import test_gpu_exec_contract as contract
from test_emu_fftconv_real import _rel
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)
from test_gpu_parity import run_plan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", tiles.CASES, ids=repr)
def test_overlap_save_tiles(fft, dev, oracle, monkeypatch, case):
    tiles.ROUTE.check_case(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch):
    tiles.ROUTE.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle)


def test_capability_images_of_1024x1024_points(fft, dev):
    """4 x 1024 x 1024 (*) 9 x 9 linear-same (32 MiB each way): windows of 48 x 48 outputs of the first and the last image at the image's
    corner, across the first tile seam on each axis and at the far corner, against float64 direct sums"""
    shape, ks, batch = (1024, 1024), (9, 9), 4
    n = shape[0] * shape[1]
    x, h = tiles.ROUTE.rand(n * batch, 0x71F1), tiles.ROUTE.rand(ks[0] * ks[1], 0x71F2)
    got, (route, launches) = run_plan(fft, dev, scaffold.options(shape, ks, batch), x, 2 * n * batch, kernel=h)
    assert tiles.ROUTE.tag in route and launches == 2 and not any(f in route for f in tiles.ROUTE.forbidden), (route, launches)
    L0, L1 = (int(v) for v in route.split(",L=")[1].split("]")[0].split("x"))
    seam0, seam1 = L0 - (ks[0] - 1) // 2, L1 - (ks[1] - 1) // 2        # output index of the first result of the second tile on each axis
    got = got.reshape(batch, shape[1], shape[0], 2)
    for b in (0, batch - 1):
        for lo in ((0, 0), (seam0 - 24, 500), (500, seam1 - 24), (seam0 - 24, seam1 - 24), (shape[0] - 48, shape[1] - 48)):
            hi = (lo[0] + 48, lo[1] + 48)
            want = tiles.ROUTE.direct_same_conv(x[2 * n * b:2 * n * (b + 1)], h, shape, ks, lo, hi)
            g = got[b, lo[1]:hi[1], lo[0]:hi[0], 0].astype(np.float64) + 1j * got[b, lo[1]:hi[1], lo[0]:hi[0], 1]
            err = np.abs(g - want)
            rel = float(np.linalg.norm(g - want) / np.linalg.norm(want))
            print(f"{route.strip()} image {b} outputs {lo}..{hi}: rel_l2={rel:.3e} max_abs={err.max():.3e}")
            assert np.all(err <= 4e-3 + 4e-3 * np.abs(want)) and rel <= 1e-5, (b, lo, rel)


def test_plan_destroyed_and_created_again(fft, dev, monkeypatch):
    """the first case of the table: create, exec, destroy, create again, exec twice into one buffer"""
    case = tiles.CASES[0]
    x, h, want = tiles.ROUTE.data(case)
    monkeypatch.setenv("MI355FFT_" + tiles.ROUTE.switch, str(case.P))
    inp, out = fft.uploadComplex(dev, x), dev.createBuffer({"size": 4 * want.size})
    for round_, execs in enumerate((1, 2)):
        plan = fft.createPlan(dev, case.opts)
        tiles.ROUTE.assert_route(case, *plan.describe())
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

@pytest.mark.parametrize("case", tiles.ACCURACY_CASES, ids=repr)
def test_accuracy(fft, dev, oracle, monkeypatch, case):
    accuracy.test_accuracy(fft, dev, oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", tiles.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", tiles.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
