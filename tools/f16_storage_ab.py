#!/usr/bin/env python3
"""precision "f16-storage" against f32, same workload, same process: for each case the f32 and the f16 plan are built, warmed,
and timed alternately with hipEvents on the library's stream (K back-to-back submits of one recorded exec per sample, the median
of R samples).  One JSON line per case: routes, launches, ms per step, GPoints/s (complex points for c2c, real points for r2c /
c2r) and the f16/f32 ratio.  Inputs come from the device PRNG (mi355fft_fill_random); on the binary16 side its f32 bit patterns
are read as binary16 pairs — arbitrary values, which the arithmetic does not care about.

  python tools/f16_storage_ab.py [--steps K] [--reps R] [--gib G] [--only c2c|r2c|c2r|conv] [--lg 10 12 ...]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-fft_amd", "python")]
try:
    import torch  # noqa: F401,E402  (load torch's HIP runtime first, as the tests do)
except Exception:
    pass
import mi355fft  # noqa: E402


class Events:
    def __init__(self):
        self.hip = None
        for name in ("libamdhip64.so.7", "libamdhip64.so"):
            try:
                self.hip = ctypes.CDLL(name)
                break
            except OSError:
                continue
        self.hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]

    def create(self):
        e = ctypes.c_void_p()
        assert self.hip.hipEventCreate(ctypes.byref(e)) == 0
        return e

    def time(self, dev, fn):
        a, b = self.create(), self.create()
        assert self.hip.hipEventRecord(a, dev.stream) == 0
        fn()
        assert self.hip.hipEventRecord(b, dev.stream) == 0
        self.hip.hipEventSynchronize(b)
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), a, b) == 0
        return float(ms.value)


class Side:
    """one plan with its buffers and one recorded exec"""

    def __init__(self, dev, opts, in_bytes, out_bytes):
        self.plan = mi355fft.createPlan(dev, opts)
        self.inp = dev.createBuffer({"size": in_bytes})
        self.out = dev.createBuffer({"size": out_bytes})
        mi355fft._chk(mi355fft.lib().mi355fft_fill_random(dev._h, self.inp._h, 0, in_bytes // 4, 1, 0x5EED0F16, 0))
        enc = dev.createCommandEncoder()
        self.plan.exec(enc, {"input": self.inp, "output": self.out})
        self.cmds = enc.finish(use_graph=False)
        self.route, self.launches = self.plan.describe()

    def run(self, dev, k):
        for _ in range(k):
            dev.queue.submit([self.cmds])

    def destroy(self):
        self.plan.destroy()
        self.inp.destroy()
        self.out.destroy()


def case(dev, ev, name, opts, points, in32, out32, in16, out16, steps, reps):
    a = Side(dev, opts, in32, out32)
    b = Side(dev, dict(opts, precision="f16-storage"), in16, out16)
    for s in (a, b):
        s.run(dev, 3)
    dev.queue.onSubmittedWorkDone()
    t32, t16 = [], []
    for _ in range(reps):
        t32.append(ev.time(dev, lambda: a.run(dev, steps)) / steps)
        t16.append(ev.time(dev, lambda: b.run(dev, steps)) / steps)
    m32, m16 = statistics.median(t32), statistics.median(t16)
    row = {"case": name, "route_f32": a.route.strip(), "route_f16": b.route.strip(), "launches_f32": a.launches, "launches_f16": b.launches,
           "ms_f32": round(m32, 4), "ms_f16": round(m16, 4), "gpoints_f32": round(points / m32 / 1e6, 1), "gpoints_f16": round(points / m16 / 1e6, 1),
           "ratio": round(m32 / m16, 3), "bytes_f16": in16 + out16}
    print(json.dumps(row), flush=True)
    a.destroy()
    b.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gib", type=float, default=1.0, help="binary16 input bytes per case (GiB)")
    ap.add_argument("--only", default="")
    ap.add_argument("--lg", type=int, nargs="*", default=None, help="log2 of the c2c line lengths / r2c, c2r half lengths (default: all)")
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    total = int(args.gib * (1 << 30))
    if args.only in ("", "c2c"):
        for lg in args.lg or range(8, 15):
            n = 1 << lg
            batch = total // (4 * n)
            pts = n * batch
            case(dev, ev, f"c2c lines[{n}] x {batch}", {"type": "c2c", "shape": [n], "batch": batch, "direction": "forward"}, pts,
                 8 * pts, 8 * pts, 4 * pts, 4 * pts, args.steps, args.reps)
    for kind in ("r2c", "c2r"):
        if args.only not in ("", kind):
            continue
        for lg in args.lg or range(10, 15):
            h = 1 << lg
            n = 2 * h
            batch = total // (2 * n)
            real, packed = n * batch, (h + 1) * batch
            opts = {"type": kind, "shape": [n], "batch": batch, "direction": "forward" if kind == "r2c" else "inverse"}
            if kind == "r2c":
                case(dev, ev, f"r2c half {h} x {batch}", opts, real, 4 * real, 8 * packed, 2 * real, 4 * packed, args.steps, args.reps)
            else:
                case(dev, ev, f"c2r half {h} x {batch}", opts, real, 8 * packed, 4 * real, 4 * packed, 2 * real, args.steps, args.reps)
    if args.only in ("", "conv"):
        n = 1 << 20
        batch = max(1, total // (4 * n))
        pts = n * batch
        case(dev, ev, f"c2c 2^20 x {batch} (conversion route)", {"type": "c2c", "shape": [n], "batch": batch, "direction": "forward"}, pts,
             8 * pts, 8 * pts, 4 * pts, 4 * pts, args.steps, args.reps)
    dev.close()


if __name__ == "__main__":
    main()
