"""GPU tier (-m gpu): the slot hand-off of the headline kernel (fft_xcd_rt1k_kernel, kern_regtile.hpp) past a group's first transform.
c2c N = 2^20 on the default route with 2 * 32 + 5 = 69 transforms: of the 32 groups some run three transforms and the rest two, so every
group re-uses its slot (one-slot mode: early arrive in the last phase-B tile, late wait in the next first phase-A tile, kern_xcd.hpp) and the
groups end at different transforms.  Both directions, every transform against the oracle at the suite's bars; the same with two slots per
group, the form without that barrier."""
import numpy as np
import pytest

from test_gpu_parity import check, run_plan

pytestmark = pytest.mark.gpu

N, BATCH = 1 << 20, 2 * 32 + 5


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
    """the seeded lines and both references, computed once for both cases"""
    x = oracle.random_complex_batch(N, BATCH, 0x4A0FF).reshape(-1)
    x.setflags(write=False)
    want = {}
    for direction in ("forward", "inverse"):
        w = oracle.c2c_ref_batch(x, [N], BATCH, direction, "backward")
        w.setflags(write=False)
        want[direction] = w
    return x, want


@pytest.mark.parametrize("slots", [None, 2])
def test_rt1k_slot_handoff_over_three_transforms_per_group(fft, dev, oracle, monkeypatch, lines, slots):
    if slots is not None:
        monkeypatch.setenv("MI355FFT_XCD_SLOTS", str(slots))
    x, want = lines
    for direction in ("forward", "inverse"):
        got, (route, launches) = run_plan(fft, dev, {"type": "c2c", "shape": [N], "batch": BATCH, "direction": direction, "normalize": "backward"}, x, x.size)
        assert route.startswith("xcd-fused-rt32[") and launches == 2, route
        for b in range(BATCH):      # per transform: a wrong line must not hide in the norm of 69
            line = slice(2 * N * b, 2 * N * (b + 1))   # (widened once here: check's helpers each take f64)
            check(oracle, got[line].astype(np.float64), want[direction][line].astype(np.float64), f"{route.strip()} {direction} slots={slots} line {b}")
