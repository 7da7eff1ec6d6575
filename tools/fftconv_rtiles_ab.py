#!/usr/bin/env python3
"""Rank-2 REAL fftconv of images with small kernels: the overlap-save tile route on real tile pairs against (a) the plan the planner gave before
it and (b) the complex tile route on the same data widened with zero imaginary parts, plans of one request in one process, timed alternately
with hipEvents on the library's stream (K back-to-back submits of one recorded exec per sample, the median of R samples).  The method of
tools/fftconv_tiles_ab.py:

  P     MI355FFT_RCONV_OLS2D=P, P in {64, 128} where a tile gives L_a >= 2 results on both axes: tiles-rspectrum for the kernels, then
        tiles-rconv-ols, one launch per kernel over batch * nb0 * ceil(nb1 / 2) tile pairs
  cP    the complex request (interleaved data, zero imaginary parts; MI355FFT_CONV_OLS2D=P): tiles-spectrum, tiles-conv-ols over batch * nb0 * nb1
        tiles — what a user could do before the route.  Only the route is timed: widening the data and narrowing the result are extra
  old   MI355FFT_RCONV_OLS2D=0: rconv[K] on the exact-length domain (r2c on axis 0, Bluestein / mixed-radix columns, a pointwise pass, the inverse
        and a staged crop per kernel).  Before it is timed, its route, launches and workspace are asserted to be the parent commit's for the same
        request (PARENT below: the parent's planner, read with emu.plan_only; the route as the first 12 hex digits of its SHA-1), so that the
        baseline is the parent's code and not the code under test

Every P and cP is sampled twice per round (P..., cP..., old, P... again, cP... again): the distance between its two medians is the run-to-run
spread the comparison has to be read against.  One JSON line per request: routes, launches, workspace, device ms per exec, G real points of
`shape` per second and kernel (batch * shape * kernelCount / time; for cP the same count of complex points), old / P and cP / P time ratios,
nb1 and the share of a launch's arithmetic an absent partner costs (odd nb1: 1 / (nb1 + 1)), the bytes the route moves per real point and
kernel by construction (4 P^2 / (L0 L1) read for the tile + 4 written) and the bandwidth that comes to.  Real inputs and kernels come from the
device PRNG; the complex side's are those values with zero imaginary parts.

  python tools/fftconv_rtiles_ab.py [--steps K] [--reps R] [--cases 0 1 ...] [--tiles 64 128]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-fft_amd", "python"), os.path.join(ROOT, "tools")]
from f16_storage_ab import Events  # noqa: E402  (also loads torch's HIP runtime first, as the tests do)
from fftconv_real_ab import fill  # noqa: E402
import mi355fft  # noqa: E402

SWITCH, COMPLEX_SWITCH = "MI355FFT_RCONV_OLS2D", "MI355FFT_CONV_OLS2D"
# (batch, shape, kernelShape, boundary): the six requests of the complex route's table as real data (nb1 is odd at the rule's tile in every one
# of them), then the first one with axis 1 grown to a whole number of pairs (nb1 = 20 at P = 64 where 1024 gives 19): the odd-nb1 loss
REQUESTS = [(8, (1024, 1024), (9, 9), "linear-same"), (4, (512, 512), (5, 5), "linear-same"), (3, (1920, 1080), (17, 17), "linear-same"),
            (1, (4096, 4096), (33, 33), "linear-valid"), (16, (256, 256), (3, 3), "linear-same"), (8, (1016, 1016), (9, 9), "linear-full"),
            (8, (1024, 1112), (9, 9), "linear-same")]
# the parent commit's plan per (request, kernelCount): route SHA-1[:12], launches, workspace bytes
PARENT = {
    (0, 1): ("1801aeeefe42", 36, 352999936), (0, 4): ("4784958358f0", 72, 493607680),      # bluestein-lines[N=516,M=2048] ... rconv[K]
    (1, 1): ("57e13892e592", 36, 45784064), (1, 4): ("55594184f2d1", 72, 68161536),        # bluestein-lines[N=258,M=1024] ... rconv[K]
    (2, 1): ("336c941c5f72", 33, 273580544), (2, 4): ("cfe4b15f48c9", 66, 426380288),      # mixed-lines[N=968,S=1,T=1,n=3] ... rconv[K]
    (3, 1): ("03fac1b2884c", 36, 884249600), (3, 4): ("259df3cf6209", 72, 2173503488),     # bluestein-lines[N=2064,M=8192] ... rconv[K]
    (4, 1): ("6f1724ab5a9f", 36, 43500544), (4, 4): ("b74a4aeb0854", 72, 58683136),        # bluestein-lines[N=129,M=512] ... rconv[K]
    (5, 1): ("b3e3fd9903c0", 12, 142745600), (5, 4): ("46f503c81a58", 24, 167936000),      # lines-r2c[N=1024] ... rconv[K]
    (6, 1): None,                                                                          # (not a request of the table: no baseline is timed)
}
# (request, kernelCount, mode): K = 1 and 4 of every request, both modes on the first
CASES = [(r, K, "convolution") for r in range(6) for K in (1, 4)] + [(0, 1, "correlation"), (6, 1, "convolution")]


class Side:
    """one plan of the request (built with `switch` at `value`) and one recorded exec into its output buffer"""

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


def out_points(shape, ks, boundary):
    n = 1
    for s, k in zip(shape, ks):
        n *= {"linear-full": s + k - 1, "linear-same": s, "linear-valid": s - k + 1}[boundary]
    return n


def widen(dev, src, floats):
    """a complex buffer holding the `floats` real values of `src` with zero imaginary parts"""
    z = np.zeros(2 * floats, np.float32)
    z[0::2] = mi355fft.downloadF32(dev, src, floats)
    dst = dev.createBuffer({"size": 8 * floats})
    dev.queue.writeBuffer(dst, 0, z)
    return dst


def case(dev, ev, req, K, mode, tile_edges, steps, reps):
    batch, shape, ks, boundary = REQUESTS[req]
    n, kn = shape[0] * shape[1], ks[0] * ks[1]
    conv = {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": list(ks)}
    real = {"type": "fftconv", "shape": list(shape), "batch": batch, "layout": {"interleavedComplex": False}, "fftConv": conv}
    cplx = {"type": "fftconv", "shape": list(shape), "batch": batch, "fftConv": conv}
    opoints = out_points(shape, ks, boundary) * batch * K
    x, h, out = dev.createBuffer({"size": 4 * n * batch}), dev.createBuffer({"size": 4 * kn * K}), dev.createBuffer({"size": 4 * opoints})
    fill(dev, x, 4 * n * batch, 0x5EED0F31)
    fill(dev, h, 4 * kn * K, 0x5EED0F32)
    xc, hc, outc = widen(dev, x, n * batch), widen(dev, h, kn * K), dev.createBuffer({"size": 8 * opoints})
    sides = {}
    old = None
    if PARENT[(req, K)] is not None:
        old = sides["old"] = Side(dev, real, SWITCH, "0", x, h, out)
        got = (hashlib.sha1(old.route.strip().encode()).hexdigest()[:12], old.launches, old.work)
        assert got == PARENT[(req, K)], f"the baseline is not the parent commit's plan: {got} != {PARENT[(req, K)]} ({old.route.strip()})"
    ps = [str(P) for P in tile_edges if P - ks[0] + 1 >= 2 and P - ks[1] + 1 >= 2]
    cs = ["c" + p for p in ps]
    for p in ps:
        sides[p] = Side(dev, real, SWITCH, p, x, h, out)
        sides["c" + p] = Side(dev, cplx, COMPLEX_SWITCH, p, xc, hc, outc)
    for s in sides.values():
        s.run(dev, 2)
    dev.queue.onSubmittedWorkDone()
    order = ps + cs + (["old"] if old else []) + [p + "'" for p in ps + cs]
    t = {k: [] for k in order}
    for _ in range(reps):
        for key in order:
            s = sides[key.rstrip("'")]
            t[key].append(ev.time(dev, lambda: s.run(dev, steps)) / steps)
    med = {k: statistics.median(v) for k, v in t.items()}
    pts = n * batch * K
    row = {"case": f"{batch} x {shape[0]}x{shape[1]} (*) {ks[0]}x{ks[1]} {boundary} {mode} K={K}", "input_mib": round(4 * n * batch / (1 << 20), 1)}
    if old:
        row.update({"route_old": old.route.strip().split(" ")[0] + " ... " + old.route.strip().split(" ")[-1], "launches_old": old.launches,
                    "work_mib_old": round(old.work / (1 << 20), 1), "ms_old": round(med["old"], 4), "greal_per_s_old": round(pts / med["old"] / 1e6, 1)})
    for p in ps:
        P = int(p)
        L0, L1 = P - ks[0] + 1, P - ks[1] + 1
        nb1 = -(-(shape[1] + ks[1] - 1) // L1)
        assert f"tiles-rconv-ols[N={P}x{P},L={L0}x{L1}]" in sides[p].route and sides[p].launches == 1 + K, sides[p].route
        assert f"tiles-conv-ols[N={P}x{P},L={L0}x{L1}]" in sides["c" + p].route and sides["c" + p].launches == 1 + K, sides["c" + p].route
        slow, fast = max(med[p], med[p + "'"]), min(med[p], med[p + "'"])
        cslow, cfast = max(med["c" + p], med["c" + p + "'"]), min(med["c" + p], med["c" + p + "'"])
        bpp = 4 * P * P / (L0 * L1) + 4
        row[f"P{p}"] = {"L": f"{L0}x{L1}", "nb1": nb1, "absent_partner_pct": round(100 / (nb1 + 1), 1) if nb1 & 1 else 0.0,
                        "launches": sides[p].launches, "work_kib": round(sides[p].work / 1024, 1),
                        "ms": [round(med[p], 4), round(med[p + "'"], 4)], "spread_pct": round(100 * (slow - fast) / fast, 1),
                        "greal_per_s": [round(pts / med[p] / 1e6, 1), round(pts / med[p + "'"] / 1e6, 1)],
                        "ms_complex": [round(med["c" + p], 4), round(med["c" + p + "'"], 4)], "spread_pct_complex": round(100 * (cslow - cfast) / cfast, 1),
                        "gcplx_per_s_complex": round(pts / cslow / 1e6, 1), "complex_over_real": round(cfast / slow, 2),
                        "bytes_per_point": round(bpp, 2), "tb_per_s": round(bpp * pts / slow / 1e9, 2)}
        if old:
            row[f"P{p}"]["old_over_tiles"] = round(med["old"] / slow, 2)
    print(json.dumps(row), flush=True)
    for s in sides.values():
        s.plan.destroy()
    for b in (x, h, out, xc, hc, outc):
        b.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the case list (default: all)")
    ap.add_argument("--tiles", type=int, nargs="*", default=[64, 128])
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    for i, (req, K, mode) in enumerate(CASES):
        if args.cases is None or i in args.cases:
            case(dev, ev, req, K, mode, args.tiles, args.steps, args.reps)
    dev.close()


if __name__ == "__main__":
    main()
