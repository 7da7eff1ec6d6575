"""Python side of the host-emulation harness (tests/emu/emu.cpp): test infrastructure only."""
import ctypes
import os
import subprocess

import numpy as np

from mi355fft import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.environ.get("MI355_EMU_LIB")
        if not path:
            subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "emu"), "libmi355emu.so"])
            path = os.path.join(_HERE, "emu", "libmi355emu.so")
        L = ctypes.CDLL(path)
        L.emu_run_plan.restype = ctypes.c_int
        L.emu_run_plan.argtypes = [ctypes.POINTER(_abi.PlanDesc), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                   ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        L.emu_run_plan_ex.restype = ctypes.c_int
        L.emu_run_plan_ex.argtypes = [ctypes.POINTER(_abi.PlanDesc), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                      ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)]
        L.emu_check_registry.restype = ctypes.c_int
        L.emu_check_registry.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        L.emu_check_xcd_registry.restype = ctypes.c_int
        L.emu_check_xcd_registry.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        L.emu_fill_random.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
        L.emu_diff_sumsq.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_uint64, ctypes.POINTER(ctypes.c_double)]
        L.emu_plan_only.restype = ctypes.c_int
        L.emu_plan_only.argtypes = [ctypes.POINTER(_abi.PlanDesc), ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint64)]
        L.emu_plan_dump.restype = ctypes.c_int
        L.emu_plan_dump.argtypes = [ctypes.POINTER(_abi.PlanDesc), ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
        _LIB = L
    return _LIB


class EmuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def plan_only(desc, compute_units=256):
    """The product planner (MI355FFT_* environment as the library reads it) without running anything: (route, launches, workspace bytes)."""
    err = ctypes.create_string_buffer(1024)
    route = ctypes.create_string_buffer(2048)
    launches = ctypes.c_int(0)
    work = ctypes.c_uint64(0)
    rc = lib().emu_plan_only(ctypes.byref(desc), compute_units, err, 1024, route, 2048, ctypes.byref(launches), ctypes.byref(work))
    if rc != 0:
        raise EmuError(rc, err.value.decode())
    return route.value.decode(), launches.value, work.value


def plan_dump(desc, compute_units=256):
    """The product planner's whole PlanIR as text (emu_plan_dump): (status, dump), or (status, error text) when planning fails."""
    size = 1 << 16
    while True:
        buf = ctypes.create_string_buffer(size)
        needed = ctypes.c_size_t(0)
        rc = lib().emu_plan_dump(ctypes.byref(desc), compute_units, buf, size, ctypes.byref(needed))
        if needed.value <= size:
            return rc, buf.value.decode()
        size = needed.value


def run_plan(desc, x, out_floats, kernel=None, force_generic=False, chunk_bytes=0, out_init=None):
    """Runs the planned transform on host arrays; returns (out, route, launches)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if desc.in_place:
        buf = x.copy()
        out = buf
        outp, outb = None, 0
    else:
        buf = x
        out = np.zeros(out_floats, dtype=np.float32) if out_init is None else np.array(out_init, dtype=np.float32, copy=True)
        outp, outb = out.ctypes.data, out.nbytes
    kp, kb = (None, 0)
    if kernel is not None:
        kernel = np.ascontiguousarray(kernel, dtype=np.float32)
        kp, kb = kernel.ctypes.data, kernel.nbytes
    err = ctypes.create_string_buffer(1024)
    route = ctypes.create_string_buffer(1024)
    launches = ctypes.c_int(0)
    rc = lib().emu_run_plan(ctypes.byref(desc), buf.ctypes.data, buf.nbytes, outp, outb, kp, kb, 1 if force_generic else 0, chunk_bytes,
                            err, 1024, route, 1024, ctypes.byref(launches))
    if rc != 0:
        raise EmuError(rc, err.value.decode())
    return out, route.value.decode(), launches.value


def banded(payload, guard, pad, room, word=0x7FC17FC1):
    """a uint8 array: `guard` bytes, `pad` more, `room` bytes (rounded up to 16) that start with `payload`, `guard` bytes again; `word`
    (a quiet NaN as f32 and as two binary16 values) everywhere but in the payload"""
    total = guard + pad + ((room + 15) // 16) * 16 + guard
    buf = np.full(total // 4, word, np.uint32).view(np.uint8)
    raw = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    buf[guard + pad:guard + pad + raw.size] = raw
    return buf


def route_of(desc):
    """(route, launches) as run_plan would plan `desc` (the MI355_EMU_* switches and the emulator's defaults), nothing run"""
    err = ctypes.create_string_buffer(1024)
    route = ctypes.create_string_buffer(2048)
    launches = ctypes.c_int(0)
    rc = lib().emu_run_plan_ex(ctypes.byref(desc), None, 0, None, 0, None, 0, 0, 0, 0, None, err, 1024, route, 2048, ctypes.byref(launches))
    if rc != 0:
        raise EmuError(rc, err.value.decode())
    return route.value.decode(), launches.value


class GuardedRun:
    """What run_plan_guarded leaves behind: every buffer whole, before and after, as bytes"""


def run_plan_guarded(desc, x, out_bytes, kernel=None, in_pad=8, out_pad=8, kernel_pad=8, guard=1 << 20, word=0x7FC17FC1, work_fill=0xFF, alias=False):
    """Runs the plan with each side at byte offset guard + pad of a larger array filled with `word`, the workspace (and its spare tail)
    filled with `work_fill`.  alias: the output is the input region itself (in-place plans, and out-of-place c2c run on one buffer).
    Returns a GuardedRun: in_before / in_after, out_after (None when aliased), kernel_before / kernel_after, the offsets, tail_modified,
    route, launches."""
    r = GuardedRun()
    alias = alias or bool(desc.in_place)
    x = np.ascontiguousarray(x)
    ibuf = banded(x, guard, in_pad, max(x.nbytes, out_bytes) if alias else x.nbytes, word)
    r.in_before, r.in_off = ibuf.copy(), guard + in_pad
    obuf = None
    if not alias:
        obuf = banded(np.empty(0, np.uint8), guard, out_pad, out_bytes, word)
    r.out_off = r.in_off if alias else guard + out_pad
    kbuf, kp, kb = None, None, 0
    if kernel is not None:
        kernel = np.ascontiguousarray(kernel, dtype=np.float32)
        kbuf = banded(kernel, guard, kernel_pad, kernel.nbytes, word)
        r.kernel_before = kbuf.copy()
        kp, kb = kbuf.ctypes.data + guard + kernel_pad, kernel.nbytes
    err = ctypes.create_string_buffer(1024)
    route = ctypes.create_string_buffer(2048)
    launches, tail = ctypes.c_int(0), ctypes.c_int(0)
    ip = ibuf.ctypes.data + r.in_off
    if desc.in_place:
        op, ob = None, 0
    else:
        op, ob = (ip if alias else obuf.ctypes.data + r.out_off), out_bytes
    rc = lib().emu_run_plan_ex(ctypes.byref(desc), ip, ibuf.size - r.in_off - guard, op, ob, kp, kb, 0, 0, work_fill, ctypes.byref(tail),
                               err, 1024, route, 2048, ctypes.byref(launches))
    if rc != 0:
        raise EmuError(rc, err.value.decode())
    r.in_after, r.out_after, r.kernel_after = ibuf, obuf, kbuf
    r.tail_modified, r.route, r.launches = bool(tail.value), route.value.decode(), launches.value
    return r
