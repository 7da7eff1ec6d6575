"""GPU tier (-m gpu): the software pipeline of the headline kernel (fft_xcd_rt1k_kernel, kern_regtile.hpp).  Part of a workgroup's next tile is
requested while the current one is in stage 1 (MI355_RT1K_PREFETCH_A / _B), and, where MI355_RT1K_PREFETCH_X is built in, in its last phase-B
tile of a transform the head of its first phase-A tile of the group's NEXT transform, a line that exists only if the group runs another one.
The shapes hold for every setting of the three: c2c N = 2^20 on the default route, every transform on its own against the oracle at the suite's bars, both directions:
  32 + 3 transforms: three of the 32 groups run two transforms, 29 run one — the request happens in some groups and must be absent in the rest;
  2 * 32 + 5 transforms with one group per XCD (32 workgroups, ONE tile each): no next tile inside a phase, only the boundary;
  5 transforms in place: the requested line is read while the same launch is still writing other lines of the buffer."""
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
    """the seeded lines and both references, computed once; a case with b transforms uses the first b"""
    x = oracle.random_complex_batch(N, BATCH, 0x91BE1).reshape(-1)
    x.setflags(write=False)
    want = {}
    for direction in ("forward", "inverse"):
        w = oracle.c2c_ref_batch(x, [N], BATCH, direction, "backward")
        w.setflags(write=False)
        want[direction] = w
    return x, want


def _each(oracle, got, want, batch, what):
    for b in range(batch):      # per transform: a line computed from another line's head must not hide in the norm of the batch
        line = slice(2 * N * b, 2 * N * (b + 1))
        check(oracle, got[line].astype(np.float64), want[line].astype(np.float64), f"{what} line {b}")


@pytest.mark.parametrize("batch,split,in_place", [(32 + 3, None, False), (2 * 32 + 5, 1, False), (5, None, True)])
def test_rt1k_pipeline(fft, dev, oracle, monkeypatch, lines, batch, split, in_place):
    if split is not None:
        monkeypatch.setenv("MI355FFT_XCD_SPLIT", str(split))
    x, want = lines
    for direction in ("forward", "inverse"):
        opts = {"type": "c2c", "shape": [N], "batch": batch, "direction": direction, "normalize": "backward"}
        if in_place:
            opts["inPlace"] = True
        got, (route, launches) = run_plan(fft, dev, opts, x[:2 * N * batch], 2 * N * batch, in_place=in_place)
        assert route.startswith("xcd-fused-rt32[") and launches == 2, route
        _each(oracle, got, want[direction], batch, f"{route.strip()} {direction} batch={batch} split={split} in_place={in_place}")
