"""GPU tier (-m gpu): the headline kernel (fft_xcd_rt1k_kernel, kern_regtile.hpp) with the modifier-form butterflies (MI355_RT1K_LEAN_BFLY) and, in a build
with MI355_RT1K_EARLY_B=1 (plan.hpp: measured, not the default), phase B's head loads between the arrive and the wait of the A | B barrier.  c2c N = 2^20 on the
default route, both directions, unscaled and unitary, as one transform and as 69 over the 32 groups (ragged ends, every group re-uses its slot); first, middle
and last transform against the oracle.  Then 69 transforms, forward and inverse, with the groups resized through MI355FFT_XCD_SPLIT to the edge of the head's
per-launch condition (16 workgroups, two rounds), far inside it (2, sixteen rounds) and outside it (32, one round: the head follows the wait), and once with
two slots per group: every one of the 69 transforms is compared there, because a head read too early or from a stale L1 line spoils single transforms, and a
wrong butterfly every one of them."""
import numpy as np
import pytest

import rt1k_early_cases as cases
from test_gpu_parity import check, run_plan

pytestmark = pytest.mark.gpu

N = cases.N20
BATCH = cases.GPU_BATCH_MAX


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
    """the seeded lines and the unscaled references of all of them, both directions, computed once and left unchanged"""
    x = oracle.random_complex_batch(N, BATCH, 0x4009).reshape(-1)
    x.setflags(write=False)
    want = {}
    for direction in ("forward", "inverse"):
        w = oracle.c2c_ref_batch(x, [N], BATCH, direction, "none")
        w.setflags(write=False)
        want[direction] = w
    return x, want


@pytest.fixture(scope="module")
def unitary(oracle, lines):
    """the unitary references of the lines the default-grouping cases compare"""
    x, _ = lines
    want = {}
    for direction in ("forward", "inverse"):
        for b in sorted({b for batch in cases.GPU_BATCHES for b in cases.checked_lines(batch)}):
            w = oracle.c2c_ref_batch(x[2 * N * b:2 * N * (b + 1)], [N], 1, direction, "unitary")
            w.setflags(write=False)
            want[direction, b] = w
    return want


@pytest.mark.parametrize("batch", cases.GPU_BATCHES)
@pytest.mark.parametrize("direction,norm", cases.DIRECTION_NORMALIZE)
def test_rt1k_early_default_grouping(fft, dev, oracle, lines, unitary, direction, norm, batch):
    x, want = lines
    opts = {"type": "c2c", "shape": [N], "batch": batch, "direction": direction, "normalize": norm}
    got, (route, launches) = run_plan(fft, dev, opts, x[:2 * N * batch], 2 * N * batch)
    assert route.strip() == cases.ROUTE_2P20 and launches == 2, (route, launches)
    for b in cases.checked_lines(batch):
        line = slice(2 * N * b, 2 * N * (b + 1))
        w = want[direction][line] if norm == "none" else unitary[direction, b]
        check(oracle, got[line].astype(np.float64), w.astype(np.float64), f"{route.strip()} {direction} {norm} batch={batch} line {b}", tol=cases.TOL)


def every_line(oracle, got, want, what):
    for b in range(BATCH):
        line = slice(2 * N * b, 2 * N * (b + 1))
        l2, mx = oracle.rel_l2(got[line], want[line]), oracle.rel_max(got[line], want[line])
        assert l2 <= cases.TOL and mx <= cases.TOL, f"{what} transform {b}: rel_l2={l2:.3e} rel_max={mx:.3e}"


@pytest.mark.parametrize("split,gsize", cases.SPLIT_GSIZE)
@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_rt1k_early_group_sizes(fft, dev, oracle, monkeypatch, lines, direction, split, gsize):
    monkeypatch.setenv("MI355FFT_XCD_SPLIT", str(split))      # groups per XCD: 32 / split workgroups in a group on a 256-CU device
    x, want = lines
    got, (route, launches) = run_plan(fft, dev, {"type": "c2c", "shape": [N], "batch": BATCH, "direction": direction, "normalize": "none"}, x, 2 * N * BATCH)
    assert route.strip() == cases.ROUTE_2P20 and launches == 2, (route, launches)
    every_line(oracle, got, want[direction], f"{route.strip()} {direction} group size {gsize}")


@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_rt1k_early_two_slots(fft, dev, oracle, monkeypatch, lines, direction):
    monkeypatch.setenv("MI355FFT_XCD_SLOTS", "2")
    x, want = lines
    got, (route, launches) = run_plan(fft, dev, {"type": "c2c", "shape": [N], "batch": BATCH, "direction": direction, "normalize": "none"}, x, 2 * N * BATCH)
    assert route.strip() == cases.ROUTE_2P20 and launches == 2, (route, launches)
    every_line(oracle, got, want[direction], f"{route.strip()} {direction} two slots")
