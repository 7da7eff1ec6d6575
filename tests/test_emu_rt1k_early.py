"""CPU tier: fft_xcd_rt1k_kernel (kern_regtile.hpp) with phase B's head loads between the arrive and the wait of the A | B barrier
(MI355_RT1K_EARLY_B, plan.hpp: measured and not the default, so this module builds the emulation a second time with the macro at 1, tests/emu/
rt1k_early.mk -> libmi355emu_early.so from emu_rt1k_early.cpp, and runs the hand-off protocol of kern_xcd.hpp from that build; the modifier-form
butterflies of MI355_RT1K_LEAN_BFLY are inline assembly and are plain bfly32 in any emulation).  c2c N = 2^20 through the 32-line register-tile
route, both directions, unscaled and unitary, three transforms in one group whose only slot is re-used twice:
  4 workgroups  8 tiles each, the per-launch condition holds: every workgroup signals the head's counter in its last phase-A tile
  3 workgroups  32 % 3 != 0: the path is off, nobody touches the counter
Every transform against the oracle, and the counter word bar[gslot][2] of the emulated control block at the end of the launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rt1k_early_cases as cases
from mi355fft import _abi

N = cases.N20
BATCH = max(b for _, _, b in cases.EMU_CONFIGS)
EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


@pytest.fixture(scope="module")
def early_lib():
    """the emulation with MI355_RT1K_EARLY_B=1 and its entry point emu_rt1k_early_run"""
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "-f", "rt1k_early.mk"])
    L = ctypes.CDLL(os.path.join(EMU_DIR, "libmi355emu_early.so"))
    L.emu_rt1k_early_run.restype = ctypes.c_int
    L.emu_rt1k_early_run.argtypes = [ctypes.POINTER(_abi.PlanDesc), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint,
                                     ctypes.POINTER(ctypes.c_uint), ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_int)]
    return L


@pytest.fixture(scope="module")
def lines(oracle):
    """the seeded lines and the four references, computed once and left unchanged"""
    x = oracle.random_complex_batch(N, BATCH, 0x4009).reshape(-1)
    x.setflags(write=False)
    want = {}
    for direction, norm in cases.DIRECTION_NORMALIZE:
        w = oracle.c2c_ref_batch(x, [N], BATCH, direction, norm)
        w.setflags(write=False)
        want[direction, norm] = w
    return x, want


def run(L, desc, x, out_floats, gslot):
    """(out, route, launches, the 16 words of group line gslot)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(out_floats, dtype=np.float32)
    bar = (ctypes.c_uint * 16)()
    err, route, launches = ctypes.create_string_buffer(1024), ctypes.create_string_buffer(1024), ctypes.c_int(0)
    rc = L.emu_rt1k_early_run(ctypes.byref(desc), x.ctypes.data, x.nbytes, out.ctypes.data, out.nbytes, gslot, bar, err, 1024, route, 1024,
                              ctypes.byref(launches))
    assert rc == 0, (rc, err.value.decode())
    return out, route.value.decode(), launches.value, list(bar)


@pytest.mark.parametrize("cus,slots,batch", cases.EMU_CONFIGS)
@pytest.mark.parametrize("direction,norm", cases.DIRECTION_NORMALIZE)
def test_rt1k_early_head(oracle, monkeypatch, early_lib, lines, direction, norm, cus, slots, batch):
    monkeypatch.setenv("MI355_EMU_XCD_FUSED", "1")
    monkeypatch.setenv("MI355_EMU_XCD_HX", "2")
    monkeypatch.setenv("MI355_EMU_CUS", str(cus))
    monkeypatch.setenv("MI355_EMU_XCDS", "1")
    monkeypatch.setenv("MI355_EMU_XCD_SPLIT", "1")
    monkeypatch.setenv("MI355_EMU_XCD_SLOTS", str(slots))
    x, want = lines
    desc = _abi.make_desc("c2c", [N], batch, direction, norm)
    # one XCD, one group: group line 0
    got, route, launches, bar = run(early_lib, desc, x[:2 * N * batch], 2 * N * batch, 0)
    assert route.strip() == cases.ROUTE_2P20 and launches == 2, (route, launches)
    for b in range(batch):
        g, w = got[2 * N * b:2 * N * (b + 1)], want[direction, norm][2 * N * b:2 * N * (b + 1)]
        l2, mx = oracle.rel_l2(g, w), oracle.rel_max(g, w)
        print(f"{route.strip()} {cus} workgroups {direction} {norm} transform {b}: rel_l2={l2:.3e} rel_max={mx:.3e}")
        assert l2 <= cases.TOL and mx <= cases.TOL, f"{cus} workgroups {direction} {norm} transform {b}: rel_l2={l2:.3e} rel_max={mx:.3e}"
    # [0] is the A | B barrier (one arrival per workgroup and transform), [2] the head's counter
    assert bar[0] == batch * cus
    assert bar[2] == (batch * cus if cases.early_enabled(cus) else 0)
