"""GPU tier (-m gpu): the headline kernel (fft_xcd_rt1k_kernel, kern_regtile.hpp) with the four-step root tables HI and LO staged in LDS
once per launch (MI355_RT1K_ROOTS_LDS).  c2c N = 2^20 on the default route, both directions, unscaled and unitary, as one transform and
as 69 over the 32 groups (ragged ends; every group re-uses its slot and reads the staged tables in every row tile of every transform);
first, last and one middle transform against the oracle at the suite's bars.  One 2^21 case on the 2048 x 1024 instance of the same
template, which has no room for the tables and keeps reading them from global memory through the same root lambda."""
import numpy as np
import pytest

import rt1k_roots_cases as cases
from test_gpu_parity import check, run_plan

pytestmark = pytest.mark.gpu

N = cases.N20


@pytest.fixture(scope="module")
def fft():
    import mi355fft
    return mi355fft


@pytest.fixture(scope="module")
def dev(fft):
    d = fft.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def lines(oracle):
    """the seeded lines, and the references of the lines that are compared, computed once and left unchanged"""
    x = oracle.random_complex_batch(N, cases.GPU_BATCH_MAX, 0x4007).reshape(-1)
    x.setflags(write=False)
    want = {}
    wanted = sorted({b for batch in cases.GPU_BATCHES for b in cases.checked_lines(batch)})
    for direction, norm in cases.DIRECTION_NORMALIZE:
        for b in wanted:
            w = oracle.c2c_ref_batch(x[2 * N * b:2 * N * (b + 1)], [N], 1, direction, norm)
            w.setflags(write=False)
            want[direction, norm, b] = w
    return x, want


@pytest.mark.parametrize("batch", cases.GPU_BATCHES)
@pytest.mark.parametrize("direction,norm", cases.DIRECTION_NORMALIZE)
def test_rt1k_roots_lds(fft, dev, oracle, lines, direction, norm, batch):
    x, want = lines
    opts = {"type": "c2c", "shape": [N], "batch": batch, "direction": direction, "normalize": norm}
    got, (route, launches) = run_plan(fft, dev, opts, x[:2 * N * batch], 2 * N * batch)
    assert route.strip() == cases.ROUTE_2P20 and launches == 2, (route, launches)
    for b in cases.checked_lines(batch):
        line = slice(2 * N * b, 2 * N * (b + 1))
        check(oracle, got[line].astype(np.float64), want[direction, norm, b].astype(np.float64), f"{route.strip()} {direction} {norm} batch={batch} line {b}", tol=cases.TOL)


def test_rt1k_2048_keeps_global_tables(fft, dev, oracle, monkeypatch):
    monkeypatch.setenv("MI355FFT_XCD_RT", "3")        # 2^21 as 2048 x 1024 on register tiles
    n, batch = cases.N21, 3
    x = oracle.random_complex_batch(n, batch, 0x4008).reshape(-1)
    for direction, norm in (("forward", "none"), ("inverse", "unitary")):
        got, (route, launches) = run_plan(fft, dev, {"type": "c2c", "shape": [n], "batch": batch, "direction": direction, "normalize": norm}, x, 2 * n * batch)
        assert route.strip() == cases.ROUTE_2P21 and launches == 2, (route, launches)
        want = oracle.c2c_ref_batch(x, [n], batch, direction, norm)
        for b in range(batch):
            line = slice(2 * n * b, 2 * n * (b + 1))
            check(oracle, got[line].astype(np.float64), want[line].astype(np.float64), f"{route.strip()} {direction} {norm} line {b}", tol=cases.TOL)
