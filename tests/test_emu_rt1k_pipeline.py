"""CPU tier: the software pipeline of fft_xcd_rt1k_kernel (kern_regtile.hpp) under host emulation.  Part of a workgroup's next tile is
requested while the current one is in stage 1 (MI355_RT1K_PREFETCH_A / _B), and in its last phase-B tile of a transform the head of its
first phase-A tile of the group's next transform (MI355_RT1K_PREFETCH_X): a line that exists only if the group runs another transform.
The cases make that condition fail at different places — per workgroup (uneven tile shares), per group (ragged batch), everywhere (one
transform per group) — and run the instances that compile the pipeline out beside them.  Every transform against the oracle.
The emulation compiles the shipped depths: phase B's next tile; phase A's pipeline and the boundary request are build macros, off.  So by
default these cases check the phase-B pipeline only, and the guard tr + groups < num_transforms is NOT tested: the ragged, one-transform-per-group
and in-place cases reach it only with a library built with -DMI355_RT1K_PREFETCH_X=32 (selected through MI355_EMU_LIB; run once that way, with
-DMI355_RT1K_PREFETCH=32 too: profiles/rt1k_pipeline_ab.log)."""
import numpy as np
import pytest

import emu_harness as emu
from mi355fft import _abi
from mi355fft.layout import resolve_plan_options

N = 1 << 20
TOL = 1e-5  # the suite's bar (test_emu_kernels.py): norm-relative, both norms
DIRECTIONS = (("forward", "none"), ("inverse", "backward"))


def check_each(oracle, got, want, batch, what):
    """every transform on its own: a line computed from another line's head must not hide in a batch-wide norm"""
    for b in range(batch):
        g, w = got[2 * N * b:2 * N * (b + 1)], want[2 * N * b:2 * N * (b + 1)]
        l2, mx = oracle.rel_l2(g, w), oracle.rel_max(g, w)
        assert l2 <= TOL and mx <= TOL, f"{what} transform {b}: rel_l2={l2:.3e} rel_max={mx:.3e}"


def _env(monkeypatch, cus, xcds, split, slots, hx=2):
    monkeypatch.setenv("MI355_EMU_XCD_FUSED", "1")
    monkeypatch.setenv("MI355_EMU_XCD_HX", str(hx))
    monkeypatch.setenv("MI355_EMU_CUS", str(cus))
    monkeypatch.setenv("MI355_EMU_XCDS", str(xcds))
    monkeypatch.setenv("MI355_EMU_XCD_SPLIT", str(split))
    monkeypatch.setenv("MI355_EMU_XCD_SLOTS", str(slots))


@pytest.fixture(scope="module")
def lines(oracle):
    """5 seeded lines and their forward / backward-normalised inverse transforms, computed once; a case with b transforms uses the first b"""
    x = oracle.random_complex_batch(N, 5, 0x91BE1).reshape(-1)
    x.setflags(write=False)
    want = {}
    for direction, norm in DIRECTIONS:
        w = oracle.c2c_ref_batch(x, [N], 5, direction, norm)
        w.setflags(write=False)
        want[direction] = w
    return x, want


# (cus, split, slots, hx, batch, label)
CASES = [
    (3, 1, 1, 2, 4, "rt32"),      # one group, tile shares 11 / 11 / 10: the last phase-B tile is a different round per workgroup; 3 boundaries, none after the 4th transform
    (4, 2, 1, 2, 5, "rt32"),      # ragged: one group runs 3 transforms, the other 2: tr + groups < num_transforms fails at a different k per group
    (4, 2, 1, 2, 2, "rt32"),      # one transform per group: no boundary at all
    (2, 1, 1, 3, 3, "rt16x2"),    # 16-line tiles: the pipeline is compiled out of this instance
    (4, 2, 2, 2, 5, "rt32"),      # two slots: no slot-reuse barrier between a boundary request and the loads it serves
]


@pytest.mark.parametrize("cus,split,slots,hx,batch,label", CASES)
def test_rt1k_pipeline(oracle, monkeypatch, lines, cus, split, slots, hx, batch, label):
    _env(monkeypatch, cus, 1, split, slots, hx)
    x, want = lines
    for direction, norm in DIRECTIONS:
        desc = _abi.make_desc("c2c", [N], batch, direction, norm)
        got, route, launches = emu.run_plan(desc, x[:2 * N * batch], 2 * N * batch)
        assert route.startswith(f"xcd-fused-{label}[N=1024x1024]") and launches == 2, route
        check_each(oracle, got, want[direction], batch, f"{route.strip()} {direction} cus={cus} split={split} slots={slots}")


def test_rt1k_pipeline_in_place(oracle, monkeypatch, lines):
    """in place: the boundary request reads line tr + groups while phase B of transform tr is still storing line tr — and nobody else writes
    line tr + groups before this group's own phase B of it"""
    _env(monkeypatch, 3, 1, 1, 1)
    x, want = lines
    batch = 3
    for direction, norm in DIRECTIONS:
        desc = _abi.make_desc("c2c", [N], batch, direction, norm, in_place=True)
        got, route, launches = emu.run_plan(desc, x[:2 * N * batch], 2 * N * batch)
        assert route.startswith("xcd-fused-rt32[N=1024x1024]") and launches == 2, route
        check_each(oracle, got, want[direction], batch, f"{route.strip()} in place {direction}")


def test_rt1k_pipeline_view_instance(oracle, monkeypatch):
    """fft_xcd_rt1k_kernel<.., VIEW> compiles the pipeline out (its loads are predicated): a shifted, shorter input view and a cropped output
    window, one group of 3 running both lines"""
    _env(monkeypatch, 3, 1, 1, 1)
    batch = 2
    vin = {"shape": [N - 3000], "offset": [1000]}            # logical i <- view element i - 1000
    vout = {"shape": [N // 2 + 77], "offset": [-50]}         # view element j <- logical j - 50
    rng = np.random.default_rng(0x91BE)
    x = rng.standard_normal(2 * vin["shape"][0] * batch).astype(np.float32)
    out_init = rng.standard_normal(2 * vout["shape"][0] * batch).astype(np.float32)
    logical = np.zeros((batch, N, 2), np.float32)
    logical[:, 1000:N - 2000] = x.reshape(batch, -1, 2)
    for direction, norm in DIRECTIONS:
        r = resolve_plan_options({"type": "c2c", "shape": [N], "batch": batch, "direction": direction, "normalize": norm,
                                  "ioView": {"input": vin, "output": vout}})
        desc = _abi.make_desc(r["type"], r["shape"], r["batch"], r["direction"], r["normalize"], r["inPlace"], r["input_layout"], r["output_layout"],
                              r["conv"], r["io_view"], r["zero_pad"])
        got, route, launches = emu.run_plan(desc, x, out_init.size, out_init=out_init)
        assert "xcd-fused-view[N=1024x1024]" in route and launches == 2, (route, launches)
        y = oracle.c2c_ref_batch(logical.reshape(-1), [N], batch, direction, norm).reshape(batch, N, 2)
        want = out_init.reshape(batch, -1, 2).copy()
        want[:, 50:] = y[:, :vout["shape"][0] - 50]
        n = vout["shape"][0]
        for b in range(batch):
            g, w = got.reshape(batch, -1)[b], want.reshape(batch, -1)[b]
            l2, mx = oracle.rel_l2(g, w), oracle.rel_max(g, w)
            assert l2 <= TOL and mx <= TOL, f"{route.strip()} {direction} line {b} ({n} elements): rel_l2={l2:.3e} rel_max={mx:.3e}"
