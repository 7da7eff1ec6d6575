#!/usr/bin/env python3
"""Rank-3 fftconv of volumes with small kernels, complex data or (--real) real data: the overlap-save brick route against the plan the planner gave
before it, plans of one request in one process, timed alternately with hipEvents on the library's stream (K back-to-back submits of one recorded
exec per sample, the median of R samples).  The method of tools/fftconv_tiles_ab.py:

  16    MI355FFT_CONV_OLS3D=16 (--real: MI355FFT_RCONV_OLS3D=16): bricks-spectrum for the kernels, then bricks-conv-ols, one launch per kernel over
        batch * nb0 * nb1 * nb2 bricks (--real: bricks-rspectrum, bricks-rconv-ols over batch * nb0 * nb1 * ceil(nb2 / 2) brick pairs)
  old   the switch at 0: the composed route on the exact-length domain (Bluestein / mixed-radix / power-of-two lines per axis, fftconv[K] or
        rconv[K]).  Before it is timed, its route, launches and workspace are asserted to be the parent commit's for the same request (PARENT
        below: the parent's planner, read with emu.plan_only; the route as the first 12 hex digits of its SHA-1), so that the baseline is the
        parent's code and not the code under test

Both forms are sampled twice per round (16, old, 16 again, old again): the distance between a form's two medians is the run-to-run spread the
comparison has to be read against.  One JSON line per request: routes, launches, workspace, device ms per exec, G points of `shape` per second and kernel
(batch * shape * kernelCount / time), the old / brick time ratio (the FASTER of the old plan's two medians over the SLOWER of the brick's), the bytes the route moves per
point and kernel by construction (E 4096 / (L0 L1 L2) read for the brick + E written, E = 8 or 4 bytes an element) and the bandwidth that comes
to.  Inputs and kernels come from the device PRNG.

  python tools/fftconv_bricks_ab.py [--real] [--steps K] [--reps R] [--cases 0 1 ...]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-fft_amd", "python"), os.path.join(ROOT, "tools")]
from f16_storage_ab import Events  # noqa: E402  (also loads torch's HIP runtime first, as the tests do)
from fftconv_real_ab import fill  # noqa: E402
import mi355fft  # noqa: E402

P = 16
# (batch, shape, kernelShape, boundary): 256^3 under the four kernel-edge classes, batches of smaller volumes, a volume that is no multiple of anything,
# and the nearest competitor: linear-full requests whose domain is 256^3, so that their old plan is the power-of-two lines and columns
REQUESTS = [(1, (256, 256, 256), (3, 3, 3), "linear-same"), (1, (256, 256, 256), (5, 5, 5), "linear-same"), (1, (256, 256, 256), (7, 7, 7), "linear-same"),
            (1, (256, 256, 256), (9, 9, 9), "linear-same"), (8, (128, 128, 128), (5, 5, 5), "linear-same"), (64, (64, 64, 64), (3, 3, 3), "linear-same"),
            (1, (500, 300, 200), (5, 5, 3), "linear-same"), (1, (252, 252, 252), (5, 5, 5), "linear-full"),
            # the same competitor for the two larger kernel-edge classes: the domain 256^3 again
            (1, (250, 250, 250), (7, 7, 7), "linear-full"), (1, (248, 248, 248), (9, 9, 9), "linear-full")]
# the parent commit's plan per (real, request, kernelCount): route SHA-1[:12], launches, workspace bytes (the same for both modes)
PARENT = {
    (False, 0, 1): ("e299b1c50109", 54, 1094845440),   # bluestein-lines[N=258,M=1024] ... fftconv[K=1]
    (False, 0, 4): ("3317118345a2", 108, 3280273920),   # bluestein-lines[N=258,M=1024] ... fftconv[K=4]
    (False, 1, 1): ("824f9d3b3260", 15, 421824000),   # mixed-lines[N=260,S=1,T=15,n=3] ... fftconv[K=1]
    (False, 1, 4): ("8805214464de", 30, 843648000),   # mixed-lines[N=260,S=1,T=15,n=3] ... fftconv[K=4]
    (False, 2, 1): ("39662b806132", 54, 1137843200),   # bluestein-lines[N=262,M=1024] ... fftconv[K=1]
    (False, 2, 4): ("20c539584bf7", 108, 3400349184),   # bluestein-lines[N=262,M=1024] ... fftconv[K=4]
    (False, 3, 1): ("dd5260a10a44", 15, 441593856),   # mixed-lines[N=264,S=1,T=15,n=3] ... fftconv[K=1]
    (False, 3, 4): ("27696e4309f1", 30, 883187712),   # mixed-lines[N=264,S=1,T=15,n=3] ... fftconv[K=4]
    (False, 4, 1): ("81acc3f8df86", 15, 312795648),   # mixed-lines[N=132,S=1,T=31,n=3] ... fftconv[K=1]
    (False, 4, 4): ("6f663fbf6259", 30, 367994880),   # mixed-lines[N=132,S=1,T=31,n=3] ... fftconv[K=4]
    (False, 5, 1): ("63577d0bf5a6", 15, 296696064),   # mixed-lines[N=66,S=1,T=62,n=3] ... fftconv[K=1]
    (False, 5, 4): ("0679f6617174", 30, 303595776),   # mixed-lines[N=66,S=1,T=62,n=3] ... fftconv[K=4]
    (False, 6, 1): ("08319d8ac4db", 51, 1824399360),   # mixed-lines[N=504,S=1,T=8,n=4] ... fftconv[K=1]
    (False, 6, 4): ("5875a6f0ee68", 102, 5316820992),   # mixed-lines[N=504,S=1,T=8,n=4] ... fftconv[K=4]
    (False, 7, 1): ("5e524f0496f2", 10, 402653184),   # lines-mapped[N=256] ... fftconv[K=1]
    (False, 7, 4): ("6f9e9f12c6cc", 22, 805306368),   # lines-mapped[N=256] ... fftconv[K=4]
    (False, 8, 1): ("5e524f0496f2", 10, 402653184),   # lines-mapped[N=256] ... fftconv[K=1]
    (False, 8, 4): ("6f9e9f12c6cc", 22, 805306368),   # lines-mapped[N=256] ... fftconv[K=4]
    (False, 9, 1): ("5e524f0496f2", 10, 402653184),   # lines-mapped[N=256] ... fftconv[K=1]
    (False, 9, 4): ("6f9e9f12c6cc", 22, 805306368),   # lines-mapped[N=256] ... fftconv[K=4]
    (True, 0, 1): ("0a1d85063c6e", 57, 895138048),   # bluestein-lines[N=129,M=512] ... rconv[K=1]
    (True, 0, 4): ("626c9bfa443b", 114, 2202403840),   # bluestein-lines[N=129,M=512] ... rconv[K=4]
    (True, 1, 1): ("c04881fc654f", 18, 634358784),   # mixed-lines[N=130,S=1,T=31,n=3] ... rconv[K=1]
    (True, 1, 4): ("2e0affb3304c", 36, 1479629056),   # mixed-lines[N=130,S=1,T=31,n=3] ... rconv[K=4]
    (True, 2, 1): ("09debe1818b9", 57, 932960256),   # bluestein-lines[N=131,M=512] ... rconv[K=1]
    (True, 2, 4): ("25894fc43aee", 114, 2288664576),   # bluestein-lines[N=131,M=512] ... rconv[K=4]
    (True, 3, 1): ("bc29d9f3bb9f", 18, 664063488),   # mixed-lines[N=132,S=1,T=31,n=3] ... rconv[K=1]
    (True, 3, 4): ("6a5c6a71cc92", 36, 1548923904),   # mixed-lines[N=132,S=1,T=31,n=3] ... rconv[K=4]
    (True, 4, 1): ("de09b115c126", 18, 471563264),   # mixed-lines[N=66,S=1,T=62,n=3] ... rconv[K=1]
    (True, 4, 4): ("01b87f5f3c38", 36, 775577088),   # mixed-lines[N=66,S=1,T=62,n=3] ... rconv[K=4]
    (True, 5, 1): ("6776955266a4", 18, 449539840),   # mixed-lines[N=33,S=1,T=64,n=2] ... rconv[K=1]
    (True, 5, 4): ("d8349b49cb3d", 36, 680790784),   # mixed-lines[N=33,S=1,T=64,n=2] ... rconv[K=4]
    (True, 6, 1): ("7def74d2fa91", 54, 1534812160),   # mixed-lines[N=252,S=1,T=16,n=4] ... rconv[K=1]
    (True, 6, 4): ("ad9da1c6887b", 108, 3659347968),   # mixed-lines[N=252,S=1,T=16,n=4] ... rconv[K=4]
    (True, 7, 1): ("9c2505e2fd71", 15, 404226048),   # lines-r2c[N=256] ... rconv[K=1]
    (True, 7, 4): ("2d7c28ef1d1b", 30, 808452096),   # lines-r2c[N=256] ... rconv[K=4]
    (True, 8, 1): ("9c2505e2fd71", 15, 404226048),   # lines-r2c[N=256] ... rconv[K=1]
    (True, 8, 4): ("2d7c28ef1d1b", 30, 808452096),   # lines-r2c[N=256] ... rconv[K=4]
    (True, 9, 1): ("9c2505e2fd71", 15, 404226048),   # lines-r2c[N=256] ... rconv[K=1]
    (True, 9, 4): ("2d7c28ef1d1b", 30, 808452096),   # lines-r2c[N=256] ... rconv[K=4]
}
# (request, kernelCount, mode): K = 1 and 4 of every request, both modes on the first
CASES = [(r, K, "convolution") for r in range(len(REQUESTS)) for K in (1, 4)] + [(0, 1, "correlation")]


class Side:
    """one plan of the request (built with `switch` at `value`) and one recorded exec into the shared output buffer"""

    def __init__(self, dev, opts, switch, value, inp, kern, out):
        saved = os.environ.get(switch)
        os.environ[switch] = value
        try:
            self.plan = mi355fft.createPlan(dev, opts)
        finally:
            os.environ.pop(switch, None)
            if saved is not None:
                os.environ[switch] = saved
        enc = dev.createCommandEncoder()
        self.plan.exec(enc, {"input": inp, "output": out, "kernel": kern})
        self.cmds = enc.finish(use_graph=False)
        self.route, self.launches = self.plan.describe()
        self.work = self.plan.getWorkspaceSizeBytes()

    def run(self, dev, k):
        for _ in range(k):
            dev.queue.submit([self.cmds])


def prod(v):
    n = 1
    for s in v:
        n *= s
    return n


def options(real, batch, shape, ks, boundary, K, mode):
    opts = {"type": "fftconv", "shape": list(shape), "batch": batch, "fftConv": {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": list(ks)}}
    if real:
        opts["layout"] = {"interleavedComplex": False}
    return opts


def case(dev, ev, real, req, K, mode, steps, reps):
    batch, shape, ks, boundary = REQUESTS[req]
    E = 4 if real else 8
    switch = "MI355FFT_RCONV_OLS3D" if real else "MI355FFT_CONV_OLS3D"
    n, kn = prod(shape), prod(ks)
    opts = options(real, batch, shape, ks, boundary, K, mode)
    opoints = prod({"linear-full": s + k - 1, "linear-same": s, "linear-valid": s - k + 1}[boundary] for s, k in zip(shape, ks)) * batch * K
    x, h, out = dev.createBuffer({"size": E * n * batch}), dev.createBuffer({"size": E * kn * K}), dev.createBuffer({"size": E * opoints})
    fill(dev, x, E * n * batch, 0x5EED0B31)
    fill(dev, h, E * kn * K, 0x5EED0B32)
    old = Side(dev, opts, switch, "0", x, h, out)
    got = (hashlib.sha1(old.route.strip().encode()).hexdigest()[:12], old.launches, old.work)
    assert got == PARENT[(real, req, K)], f"the baseline is not the parent commit's plan: {got} != {PARENT[(real, req, K)]} ({old.route.strip()})"
    new = Side(dev, opts, switch, str(P), x, h, out)
    L = [P - k + 1 for k in ks]
    tag = f"bricks-{'r' if real else ''}conv-ols[N=16x16x16,L={L[0]}x{L[1]}x{L[2]}]"
    assert tag in new.route and new.launches == 1 + K and new.work < 1 << 20, (new.route, new.launches, new.work)
    sides = {"16": new, "old": old}
    for s in sides.values():
        s.run(dev, 2)
    dev.queue.onSubmittedWorkDone()
    order = ["16", "old", "16'", "old'"]
    t = {k: [] for k in order}
    for _ in range(reps):
        for key in order:
            s = sides[key.rstrip("'")]
            t[key].append(ev.time(dev, lambda: s.run(dev, steps)) / steps)
    med = {k: statistics.median(v) for k, v in t.items()}
    pts = n * batch * K
    slow, fast = max(med["16"], med["16'"]), min(med["16"], med["16'"])
    oslow, ofast = max(med["old"], med["old'"]), min(med["old"], med["old'"])
    bpp = E * P ** 3 / prod(L) + E
    words = old.route.strip().split(" ")
    row = {"case": f"{'real ' if real else ''}{batch} x {'x'.join(map(str, shape))} (*) {'x'.join(map(str, ks))} {boundary} {mode} K={K}",
           "input_mib": round(E * n * batch / (1 << 20), 1),
           "route_old": words[0] + " ... " + words[-1], "launches_old": old.launches, "work_mib_old": round(old.work / (1 << 20), 1),
           "ms_old": [round(med["old"], 4), round(med["old'"], 4)], "spread_pct_old": round(100 * (oslow - ofast) / ofast, 1),
           "gpoints_per_s_old": round(pts / ofast / 1e6, 1),
           "L": "x".join(map(str, L)), "returned": round(prod(L) / P ** 3, 3), "launches": new.launches, "work_kib": round(new.work / 1024, 1),
           "ms": [round(med["16"], 4), round(med["16'"], 4)], "spread_pct": round(100 * (slow - fast) / fast, 1),
           "gpoints_per_s": [round(pts / med["16"] / 1e6, 1), round(pts / med["16'"] / 1e6, 1)],
           "old_over_bricks": round(ofast / slow, 2), "bytes_per_point": round(bpp, 2), "tb_per_s": round(bpp * pts / slow / 1e9, 2)}
    print(json.dumps(row), flush=True)
    for s in sides.values():
        s.plan.destroy()
    for b in (x, h, out):
        b.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", action="store_true", help="real data: bricks-rconv-ols against rconv[K]")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the case list (default: all)")
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    for i, (req, K, mode) in enumerate(CASES):
        if args.cases is None or i in args.cases:
            case(dev, ev, args.real, req, K, mode, args.steps, args.reps)
    dev.close()


if __name__ == "__main__":
    main()
