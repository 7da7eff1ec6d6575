"""CPU tier: the slot hand-off of fft_xcd_rt1k_kernel (kern_regtile.hpp) under host emulation.  In one-slot mode a workgroup signals its
last read of the group's slot inside its last phase-B tile and waits for its peers inside the first phase-A tile of the next transform
(kern_xcd.hpp); these cases make groups run more than one transform each, with ragged ends, uneven tile shares, in place, on 16-line
tiles and on the view instance, and keep the two-slot form (no such barrier) beside them.  Every transform against the oracle."""
import numpy as np
import pytest

import emu_harness as emu
from mi355fft import _abi
from mi355fft.layout import resolve_plan_options

N = 1 << 20
TOL = 1e-5  # the suite's bar (test_emu_kernels.py): norm-relative, both norms


def check(got, want, what):
    from oracle import oracle as orc
    l2, mx = orc.rel_l2(got, want), orc.rel_max(got, want)
    assert l2 <= TOL and mx <= TOL, f"{what}: rel_l2={l2:.3e} rel_max={mx:.3e}"


def _env(monkeypatch, cus, xcds, split, slots, hx=2):
    monkeypatch.setenv("MI355_EMU_XCD_FUSED", "1")
    monkeypatch.setenv("MI355_EMU_XCD_HX", str(hx))
    monkeypatch.setenv("MI355_EMU_CUS", str(cus))
    monkeypatch.setenv("MI355_EMU_XCDS", str(xcds))
    monkeypatch.setenv("MI355_EMU_XCD_SPLIT", str(split))
    monkeypatch.setenv("MI355_EMU_XCD_SLOTS", str(slots))


@pytest.fixture(scope="module")
def lines(oracle):
    """7 seeded lines and their forward / backward-normalised inverse transforms, computed once; a case with b transforms uses the first b"""
    x = oracle.random_complex_batch(N, 7, 0x4A0FF).reshape(-1)
    x.setflags(write=False)
    want = {}
    for direction, norm in (("forward", "none"), ("inverse", "backward")):
        w = oracle.c2c_ref_batch(x, [N], 7, direction, norm)
        w.setflags(write=False)
        want[direction] = w
    return x, want


# (cus, xcds, split, slots, hx, batch, label)
CASES = [
    (4, 1, 2, 1, 2, 5, "rt32"),      # two groups of 2 run 3 and 2 transforms: ragged end, no wait after a group's last transform
    (3, 1, 1, 1, 2, 7, "rt32"),      # one group of 3, tile shares 11 / 11 / 10: the last tile is a different round for the third workgroup
    (4, 1, 2, 2, 2, 5, "rt32"),      # two slots: no slot-reuse barrier at all (unchanged path)
    (2, 1, 1, 1, 3, 3, "rt16x2"),    # the same code on 16-line tiles (64 tiles over 2 workgroups)
]


@pytest.mark.parametrize("cus,xcds,split,slots,hx,batch,label", CASES)
def test_rt1k_slot_handoff(oracle, monkeypatch, lines, cus, xcds, split, slots, hx, batch, label):
    _env(monkeypatch, cus, xcds, split, slots, hx)
    x, want = lines
    for direction, norm in (("forward", "none"), ("inverse", "backward")):
        desc = _abi.make_desc("c2c", [N], batch, direction, norm)
        got, route, launches = emu.run_plan(desc, x[:2 * N * batch], 2 * N * batch)
        assert route.startswith(f"xcd-fused-{label}[N=1024x1024]") and launches == 2, route
        check(got, want[direction][:2 * N * batch], f"{route.strip()} {direction} cus={cus} split={split} slots={slots}")


def test_rt1k_slot_handoff_in_place(oracle, monkeypatch, lines):
    """in place: phase B of transform k overwrites x of transform k only; the group's next transform reads its own line"""
    _env(monkeypatch, 3, 1, 1, 1)
    x, want = lines
    batch = 3
    for direction, norm in (("forward", "none"), ("inverse", "backward")):
        desc = _abi.make_desc("c2c", [N], batch, direction, norm, in_place=True)
        got, route, launches = emu.run_plan(desc, x[:2 * N * batch], 2 * N * batch)
        assert route.startswith("xcd-fused-rt32[N=1024x1024]") and launches == 2, route
        check(got, want[direction][:2 * N * batch], f"{route.strip()} in place {direction}")


def test_rt1k_slot_handoff_view_instance(oracle, monkeypatch):
    """fft_xcd_rt1k_kernel<.., VIEW>: a shifted, shorter input view and a cropped output window as predicates of the first loads and the last
    stores; one group of 3 runs both lines, so the second one passes the late wait"""
    _env(monkeypatch, 3, 1, 1, 1)
    batch = 2
    vin = {"shape": [N - 3000], "offset": [1000]}            # logical i <- view element i - 1000
    vout = {"shape": [N // 2 + 77], "offset": [-50]}         # view element j <- logical j - 50
    rng = np.random.default_rng(0x4A0F)
    x = rng.standard_normal(2 * vin["shape"][0] * batch).astype(np.float32)
    out_init = rng.standard_normal(2 * vout["shape"][0] * batch).astype(np.float32)
    logical = np.zeros((batch, N, 2), np.float32)
    logical[:, 1000:N - 2000] = x.reshape(batch, -1, 2)
    for direction, norm in (("forward", "none"), ("inverse", "backward")):
        r = resolve_plan_options({"type": "c2c", "shape": [N], "batch": batch, "direction": direction, "normalize": norm,
                                  "ioView": {"input": vin, "output": vout}})
        desc = _abi.make_desc(r["type"], r["shape"], r["batch"], r["direction"], r["normalize"], r["inPlace"], r["input_layout"], r["output_layout"],
                              r["conv"], r["io_view"], r["zero_pad"])
        got, route, launches = emu.run_plan(desc, x, out_init.size, out_init=out_init)
        assert "xcd-fused-view[N=1024x1024]" in route and launches == 2, (route, launches)
        y = oracle.c2c_ref_batch(logical.reshape(-1), [N], batch, direction, norm).reshape(batch, N, 2)
        want = out_init.reshape(batch, -1, 2).copy()
        want[:, 50:] = y[:, :vout["shape"][0] - 50]
        check(got, want.reshape(-1), f"{route.strip()} {direction}")
