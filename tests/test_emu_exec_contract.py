"""CPU tier: the exec contract of exec_contract_cases.py under emulation.

Every case the emulator plans on the route the table names (others skip by route; the 2^20 .. 2^22 cases are left to the GPU tier: Case.emu)
runs twice more than the plain way: each side at a byte offset of 8 (mod 16) (f16: 4) inside an array with 1 MiB of poison before and after
it, and with the input aligned and the output not; both on a workspace whose every byte, the 256 spare ones included, is 0xFF.  The result
is the plain run's bit for bit and within the route's oracle bar; nothing around the output, nothing of the input or the kernel, and nothing
behind the workspace changes.  An out-of-place c2c plan run with its output on its input either does the same or is refused."""
import numpy as np
import pytest

import emu_harness as emu
import exec_contract_cases as t

EMU_CASES = [c for c in t.CASES if c.emu]


def _words(raw):
    return np.asarray(raw).view(np.uint32)


def _assert_guards(buf, off, nbytes, what):
    """every word of `buf` outside [off, off + nbytes) still holds the poison pattern"""
    end = off + (nbytes + 3) // 4 * 4
    for name, part in (("before", buf[:off]), ("after", buf[end:])):
        bad = np.flatnonzero(_words(part) != t.POISON)
        assert bad.size == 0, f"{what}: {bad.size} guard words {name} the range were written, the first at word {int(bad[0])}"


def _out_bytes(case, want):
    return (want.size * (2 if case.f16 else 4) + 3) // 4 * 4


def _region(run, nbytes, aliased=False):
    buf = run.in_after if (aliased or run.out_after is None) else run.out_after
    return buf[run.out_off:run.out_off + nbytes]


def _check_sides(case, run, x, nbytes, what):
    assert not run.tail_modified, f"{what}: bytes behind the workspace were written"
    if run.out_after is not None:
        _assert_guards(run.out_after, run.out_off, nbytes, f"{what}: output")
        assert np.array_equal(run.in_after, run.in_before), f"{what}: the input buffer was written"
    else:
        _assert_guards(run.in_after, run.in_off, max(nbytes, x.nbytes), f"{what}: input")
    if run.kernel_after is not None:
        assert np.array_equal(run.kernel_after, run.kernel_before), f"{what}: the kernel buffer was written"


@pytest.mark.parametrize("case", EMU_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    for k, v in case.emu_env.items():
        monkeypatch.setenv("MI355_EMU_" + k, v)
    desc, _ = t.desc_of(case.opts)
    route, _ = emu.route_of(desc)
    if not case.route_ok(route):
        pytest.skip(f"the emulator plans this request as {route.strip()}")
    x, kern, want, keep = t.data(oracle, case)
    nbytes = _out_bytes(case, want)
    pad = 4 if case.f16 else 8
    plain = emu.run_plan_guarded(desc, x, nbytes, kern, in_pad=0, out_pad=0, kernel_pad=0, work_fill=0)
    assert plain.route == route
    base = _region(plain, nbytes).copy()
    got = base.view(t.out_dtype(case))[:want.size]
    t.compare(oracle, case, got, want, keep, f"{case.name} ({route.strip()})")
    t.assert_untouched(base, keep, case, case.name)
    _check_sides(case, plain, x, nbytes, f"{case.name} plain")
    for in_pad, out_pad in ((pad, pad), (0, pad)):
        if case.in_place and in_pad != out_pad:
            continue
        what = f"{case.name} input +{in_pad} output +{out_pad} ({route.strip()})"
        run = emu.run_plan_guarded(desc, x, nbytes, kern, in_pad=in_pad, out_pad=out_pad, kernel_pad=8, work_fill=0xFF)
        assert run.route == route
        _check_sides(case, run, x, nbytes, what)
        differ = np.flatnonzero(_region(run, nbytes) != base)
        assert differ.size == 0, f"{what}: {differ.size} bytes differ from the plain run, the first at byte {int(differ[0])}"


@pytest.mark.parametrize("case", [c for c in EMU_CASES if c.type == "c2c" and not c.in_place], ids=repr)
def test_out_of_place_c2c_on_one_buffer(oracle, monkeypatch, case):
    """output = the input buffer at the same offset: the oracle's result with the guards intact.  No case of the table is refused."""
    for k, v in case.emu_env.items():
        monkeypatch.setenv("MI355_EMU_" + k, v)
    desc, _ = t.desc_of(case.opts)
    route, _ = emu.route_of(desc)
    if not case.route_ok(route):
        pytest.skip(f"the emulator plans this request as {route.strip()}")
    x, kern, want, keep = t.data(oracle, case)
    nbytes = _out_bytes(case, want)
    run = emu.run_plan_guarded(desc, x, nbytes, kern, in_pad=4 if case.f16 else 8, work_fill=0xFF, alias=True)
    what = f"{case.name} on one buffer ({run.route.strip()})"
    assert not run.tail_modified, f"{what}: bytes behind the workspace were written"
    _assert_guards(run.in_after, run.in_off, max(nbytes, x.nbytes), what)
    raw = _region(run, nbytes, aliased=True)
    t.compare(oracle, case, raw.view(t.out_dtype(case))[:want.size], want, keep, what)
    if keep.any():      # elements the plan leaves alone hold what the input had there
        bits = np.uint16 if case.f16 else np.uint32
        was = run.in_before[run.out_off:run.out_off + nbytes].view(bits)[:want.size]
        assert np.array_equal(raw.view(bits)[:want.size][keep], was[keep]), f"{what}: elements outside the plan's stores were written"


def test_dense_ranges_that_overlap_at_different_offsets_are_refused():
    """the rule exec applies (plan.hpp alias_variant), through the emulator's entry point: one range and disjoint ranges run"""
    import ctypes
    desc, _ = t.desc_of(t.BY_NAME["lines64"].opts)
    nbytes = 64 * 37 * 8
    buf = np.zeros(3 * nbytes, np.uint8)

    def run(out_off):
        err, route, launches = ctypes.create_string_buffer(1024), ctypes.create_string_buffer(1024), ctypes.c_int(0)
        rc = emu.lib().emu_run_plan_ex(ctypes.byref(desc), buf.ctypes.data, nbytes, buf.ctypes.data + out_off, nbytes, None, 0, 0, 0, 0, None,
                                       err, 1024, route, 1024, ctypes.byref(launches))
        return rc, err.value.decode()

    rc, msg = run(64)
    assert rc != 0 and "output range overlaps the input range at another offset" in msg, (rc, msg)
    assert run(0)[0] == 0 and run(nbytes)[0] == 0
