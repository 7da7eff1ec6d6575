"""CPU tier: fft_xcd_rt1k_kernel (kern_regtile.hpp) with the four-step root tables HI and LO staged in LDS once per launch
(MI355_RT1K_ROOTS_LDS, the emulation compiles the shipped setting of the macro and runs the same code path).  c2c N = 2^20 through the
32-line register-tile route, both directions, unscaled and unitary; three emulated workgroups in one group run three transforms, so
every workgroup takes several row tiles per phase B (each one reads its six roots from the staged tables) and re-uses the group's slot.
Every transform against the oracle."""
import pytest

import emu_harness as emu
import rt1k_roots_cases as cases
from mi355fft import _abi

N = cases.N20


@pytest.fixture(scope="module")
def lines(oracle):
    """the seeded lines and the four references, computed once and left unchanged"""
    x = oracle.random_complex_batch(N, cases.EMU_BATCH, 0x4007).reshape(-1)
    x.setflags(write=False)
    want = {}
    for direction, norm in cases.DIRECTION_NORMALIZE:
        w = oracle.c2c_ref_batch(x, [N], cases.EMU_BATCH, direction, norm)
        w.setflags(write=False)
        want[direction, norm] = w
    return x, want


@pytest.mark.parametrize("direction,norm", cases.DIRECTION_NORMALIZE)
def test_rt1k_roots_lds(oracle, monkeypatch, lines, direction, norm):
    monkeypatch.setenv("MI355_EMU_XCD_FUSED", "1")
    monkeypatch.setenv("MI355_EMU_XCD_HX", "2")
    monkeypatch.setenv("MI355_EMU_CUS", str(cases.EMU_CUS))
    monkeypatch.setenv("MI355_EMU_XCDS", "1")
    monkeypatch.setenv("MI355_EMU_XCD_SPLIT", str(cases.EMU_SPLIT))
    monkeypatch.setenv("MI355_EMU_XCD_SLOTS", str(cases.EMU_SLOTS))
    x, want = lines
    batch = cases.EMU_BATCH
    desc = _abi.make_desc("c2c", [N], batch, direction, norm)
    got, route, launches = emu.run_plan(desc, x, 2 * N * batch)
    assert route.strip() == cases.ROUTE_2P20 and launches == 2, (route, launches)
    for b in range(batch):
        g, w = got[2 * N * b:2 * N * (b + 1)], want[direction, norm][2 * N * b:2 * N * (b + 1)]
        l2, mx = oracle.rel_l2(g, w), oracle.rel_max(g, w)
        print(f"{route.strip()} {direction} {norm} transform {b}: rel_l2={l2:.3e} rel_max={mx:.3e}")
        assert l2 <= cases.TOL and mx <= cases.TOL, f"{direction} {norm} transform {b}: rel_l2={l2:.3e} rel_max={mx:.3e}"
