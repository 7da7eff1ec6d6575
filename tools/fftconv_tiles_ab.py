#!/usr/bin/env python3
"""Rank-2 complex fftconv of images with small kernels: the overlap-save tile route against the plan the planner gave before it, plans of one
request in one process, timed alternately with hipEvents on the library's stream (K back-to-back submits of one recorded exec per sample, the
median of R samples).  The method of tools/fftconv_cols_ab.py:

  P     MI355FFT_CONV_OLS2D=P, P in {64, 128} where a tile gives L_a >= 2 results on both axes: tiles-spectrum for the kernels, then
        tiles-conv-ols, one launch per kernel over batch * nb0 * nb1 tiles
  old   MI355FFT_CONV_OLS2D=0: the composed route on the exact-length domain (Bluestein / mixed-radix lines per axis, fftconv[K]).  Before it is
        timed, its route, launches and workspace are asserted to be the parent commit's for the same request (PARENT below: the parent's planner,
        read with emu.plan_only; the route as the first 12 hex digits of its SHA-1), so that the baseline is the parent's code and not the code under test

Every P is sampled twice per round (P..., old, P... again): the distance between its two medians is the run-to-run spread the comparison
has to be read against.  One JSON line per request: routes, launches, workspace, device ms per exec, G complex points of `shape` per second
and kernel (batch * shape * kernelCount / time), old / P time ratios, the bytes the route moves per point and kernel by construction
(8 P^2 / (L0 L1) read for the tile + 8 written) and the bandwidth that comes to.  Inputs and kernels come from the device PRNG.

  python tools/fftconv_tiles_ab.py [--steps K] [--reps R] [--cases 0 1 ...] [--tiles 64 128]"""
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

SWITCH = "MI355FFT_CONV_OLS2D"
# (batch, shape, kernelShape, boundary): the six requests of the route's issue, then two for the rule's boundary
REQUESTS = [(8, (1024, 1024), (9, 9), "linear-same"), (4, (512, 512), (5, 5), "linear-same"), (3, (1920, 1080), (17, 17), "linear-same"),
            (1, (4096, 4096), (33, 33), "linear-valid"), (16, (256, 256), (3, 3), "linear-same"), (8, (1016, 1016), (9, 9), "linear-full"),
            # between the kernels of 17 and of 33 points: where the 128-point tile overtakes the 64-point one
            (3, (1920, 1080), (21, 21), "linear-same"), (3, (1920, 1080), (25, 25), "linear-same")]
# the parent commit's plan per (request, kernelCount): route SHA-1[:12], launches, workspace bytes (the same for both modes)
PARENT = {
    (0, 1): ("8df2e3ced590", 33, 483537408), (0, 4): ("2d5cb578f16d", 66, 509097984),
    (1, 1): ("180faef13b4f", 33, 61507328), (1, 2): ("0de76fd1444a", 44, 63637248), (1, 4): ("d4373d67c2e1", 66, 67897344),
    (2, 1): ("a213a459adb2", 30, 360065024), (2, 4): ("a3c8070bddb0", 60, 410989568),
    (3, 1): ("50b9e8677e21", 33, 1086357504), (3, 4): ("73f7e9b65459", 66, 3254845440),
    (4, 1): ("c285322eacc4", 33, 59909888), (4, 4): ("c1f6028c856a", 66, 61507328),
    (5, 1): ("873b8aa89c95", 7, 142606336), (5, 4): ("f7e5a89fa0f6", 16, 167772160),
    (6, 1): ("8ff97c3c54b7", 24, 227638784), (7, 1): ("06291ce9e345", 30, 362797056),
}
# (request, kernelCount, mode): K = 1 and 4 of every request, both modes on the first
CASES = [(r, K, "convolution") for r in range(6) for K in (1, 4)] + [(0, 1, "correlation"), (1, 2, "convolution"), (6, 1, "convolution"), (7, 1, "convolution")]


class Side:
    """one plan of the request (built with the switch at `value`) and one recorded exec into the shared output buffer"""

    def __init__(self, dev, opts, value, inp, kern, out):
        saved = os.environ.get(SWITCH)
        os.environ[SWITCH] = value
        try:
            self.plan = mi355fft.createPlan(dev, opts)
        finally:
            os.environ.pop(SWITCH, None)
            if saved is not None:
                os.environ[SWITCH] = saved
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


def case(dev, ev, req, K, mode, tile_edges, steps, reps):
    batch, shape, ks, boundary = REQUESTS[req]
    n, kn = shape[0] * shape[1], ks[0] * ks[1]
    opts = {"type": "fftconv", "shape": list(shape), "batch": batch,
            "fftConv": {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": list(ks)}}
    obytes = 8 * out_points(shape, ks, boundary) * batch * K
    x, h, out = dev.createBuffer({"size": 8 * n * batch}), dev.createBuffer({"size": 8 * kn * K}), dev.createBuffer({"size": obytes})
    fill(dev, x, 8 * n * batch, 0x5EED0F21)
    fill(dev, h, 8 * kn * K, 0x5EED0F22)
    sides = {"old": Side(dev, opts, "0", x, h, out)}
    old = sides["old"]
    got = (hashlib.sha1(old.route.strip().encode()).hexdigest()[:12], old.launches, old.work)
    assert got == PARENT[(req, K)], f"the baseline is not the parent commit's plan: {got} != {PARENT[(req, K)]} ({old.route.strip()})"
    for P in tile_edges:
        if P - ks[0] + 1 >= 2 and P - ks[1] + 1 >= 2:
            sides[str(P)] = Side(dev, opts, str(P), x, h, out)
    for s in sides.values():
        s.run(dev, 2)
    dev.queue.onSubmittedWorkDone()
    ps = [k for k in sides if k != "old"]
    order = ps + ["old"] + [p + "'" for p in ps]
    t = {k: [] for k in order}
    for _ in range(reps):
        for key in order:
            s = sides[key.rstrip("'")]
            t[key].append(ev.time(dev, lambda: s.run(dev, steps)) / steps)
    med = {k: statistics.median(v) for k, v in t.items()}
    pts = n * batch * K
    row = {"case": f"{batch} x {shape[0]}x{shape[1]} (*) {ks[0]}x{ks[1]} {boundary} {mode} K={K}", "input_mib": round(8 * n * batch / (1 << 20), 1),
           "route_old": old.route.strip().split(" ")[0] + " ... " + old.route.strip().split(" ")[-1], "launches_old": old.launches,
           "work_mib_old": round(old.work / (1 << 20), 1), "ms_old": round(med["old"], 4), "gcplx_per_s_old": round(pts / med["old"] / 1e6, 1)}
    for p in ps:
        P = int(p)
        L0, L1 = P - ks[0] + 1, P - ks[1] + 1
        assert f"tiles-conv-ols[N={P}x{P},L={L0}x{L1}]" in sides[p].route and sides[p].launches == 1 + K, sides[p].route
        slow, fast = max(med[p], med[p + "'"]), min(med[p], med[p + "'"])
        bpp = 8 * P * P / (L0 * L1) + 8
        row[f"P{p}"] = {"L": f"{L0}x{L1}", "launches": sides[p].launches, "work_kib": round(sides[p].work / 1024, 1),
                        "ms": [round(med[p], 4), round(med[p + "'"], 4)], "spread_pct": round(100 * (slow - fast) / fast, 1),
                        "gcplx_per_s": [round(pts / med[p] / 1e6, 1), round(pts / med[p + "'"] / 1e6, 1)],
                        "old_over_tiles": round(med["old"] / slow, 2), "bytes_per_point": round(bpp, 2), "tb_per_s": round(bpp * pts / slow / 1e9, 2)}
    print(json.dumps(row), flush=True)
    for s in sides.values():
        s.plan.destroy()
    for b in (x, h, out):
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
