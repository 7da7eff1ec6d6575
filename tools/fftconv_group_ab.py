#!/usr/bin/env python3
"""fftConv.groups (y[b][k] = sum_{c < Cg} x[b][g Cg + c] (*) h[k][c], g = k // Kg) on rank-2 images with small kernels, complex and real data: the grouped
tile kernel (every output kernel in one launch) against the switch at 0 and against what a caller could do before the option, plans of one request in
one process, timed alternately with hipEvents on the library's stream (S back-to-back submits of one recorded command list per sample, the median of R
samples).  The method of tools/fftconv_sum_ab.py:

  a  MI355FFT_GROUP_OLS2D=64: tiles-(r)spectrum tiles-(r)conv-ols-group[N=64x64,..,C=c,G=g,K=k], 2 launches
  b  MI355FFT_GROUP_OLS2D=0: depthwise requests (Cg = 1) on the single-channel tile route through the per-kernel load map, 1 + K launches; Cg > 1 on the
     composed route fftconv-sum[K,C,G] / rconv-sum[K,C,G]
  c  what a caller could do before: the plan with inputChannels = Cg and kernelCount = Kg (the planner's own rule) executed G times back to back, exec g at
     the offsets of a buffer already sliced per group ([G][batch][Cg][shape] data, [G][Kg][Cg] kernels with each group's block padded to a multiple of 8 bytes, [G][Kg][batch] results).  The slicing, which such a
     caller has to do on top, is not counted: c flatters the parent

The three forms are sampled twice per round (a, b, c, a', b', c'): the distance between a form's two medians is the run-to-run spread the comparison has
to be read against.  One JSON line per request: routes, launches, device ms per exec, b / a (the FASTER of b's two medians over the SLOWER of a's) and
c / a (the same); then one verdict line per class (depthwise / grouped sum, complex / real): the class enters the planner's rule only if a is ahead of both
b and c on every request of it by more than the spread.  Inputs and kernels come from the device PRNG.

  python tools/fftconv_group_ab.py [--reps R] [--cases 0 1 ...] [--only complex|real]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-fft_amd", "python"), os.path.join(ROOT, "tools")]
from f16_storage_ab import Events  # noqa: E402  (also loads torch's HIP runtime first, as the tests do)
from fftconv_real_ab import fill  # noqa: E402
import mi355fft  # noqa: E402

SWITCH = "MI355FFT_GROUP_OLS2D"
# (batch, shape, kernelShape, C, K, G), linear-same
REQUESTS = [
    (8, (256, 256), (3, 3), 64, 64, 64),
    (8, (256, 256), (5, 5), 64, 64, 64),
    (4, (512, 512), (9, 9), 32, 32, 32),
    (8, (256, 256), (3, 3), 64, 64, 4),
    (8, (256, 256), (3, 3), 16, 32, 16),
    (3, (1920, 1080), (17, 17), 3, 3, 3),
]


def prod(v):
    n = 1
    for s in v:
        n *= s
    return n


def options(real, batch, shape, ks, C, K, G=None):
    fc = {"mode": "convolution", "boundary": "linear-same", "kernelCount": K, "kernelShape": list(ks)}
    if C > 1:
        fc["inputChannels"] = C
    if G:
        fc["groups"] = G
    return {"type": "fftconv", "shape": list(shape), "batch": batch, "fftConv": fc, "layout": {"interleavedComplex": not real}}


class Side:
    """one plan (built with the switch at `value`) and one recorded command list: `execs` execs of it, exec g at the offsets offs(g)"""

    def __init__(self, dev, opts, value, inp, kern, out, execs=1, offs=lambda g: (0, 0, 0)):
        saved = os.environ.get(SWITCH)
        if value is not None:
            os.environ[SWITCH] = value
        try:
            self.plan = mi355fft.createPlan(dev, opts)
        finally:
            os.environ.pop(SWITCH, None)
            if saved is not None:
                os.environ[SWITCH] = saved
        enc = dev.createCommandEncoder()
        for g in range(execs):
            io, ko, oo = offs(g)
            self.plan.exec(enc, {"input": inp, "output": out, "kernel": kern, "inputOffsetBytes": io, "kernelOffsetBytes": ko, "outputOffsetBytes": oo})
        self.cmds = enc.finish(use_graph=False)
        self.route, self.launches = self.plan.describe()
        self.launches *= execs
        self.work = self.plan.getWorkspaceSizeBytes()

    def run(self, dev, k):
        for _ in range(k):
            dev.queue.submit([self.cmds])


def case(dev, ev, real, req, reps):
    batch, shape, ks, C, K, G = REQUESTS[req]
    Cg, Kg = C // G, K // G
    E = 4 if real else 8
    n, kn = prod(shape), prod(ks)
    kblock = (E * kn * Kg * Cg + 7) // 8 * 8                 # form c: each group's kernels in a block padded to a multiple of 8 bytes (exec offsets are multiples of 8),
    kbytes = max(E * kn * K * Cg, G * kblock)                # so every exec reads whole, aligned kernels; forms a and b read the packed K Cg kernels at the front
    x, h, out = dev.createBuffer({"size": E * n * batch * C}), dev.createBuffer({"size": kbytes}), dev.createBuffer({"size": E * n * batch * K})
    fill(dev, x, E * n * batch * C, 0x5EED6C00)
    fill(dev, h, kbytes // 4 * 4, 0x5EED6C01)
    grouped = options(real, batch, shape, ks, C, K, G)
    per_group = options(real, batch, shape, ks, Cg, Kg)
    sides = {"a": Side(dev, grouped, "64", x, h, out), "b": Side(dev, grouped, "0", x, h, out),
             "c": Side(dev, per_group, None, x, h, out, G, lambda g: (E * n * batch * Cg * g, kblock * g, E * n * batch * Kg * g))}
    r = "r" if real else ""
    assert f"tiles-{r}conv-ols-group[N=64x64" in sides["a"].route and sides["a"].launches == 2, sides["a"].route
    assert "-group[" not in sides["b"].route and sides["b"].launches > 2, sides["b"].route      # (a long composed route is cut short by describe(): its last tag may be missing)
    steps = {}
    for k, s in sides.items():
        s.run(dev, 1)
        dev.queue.onSubmittedWorkDone()
        once = ev.time(dev, lambda: s.run(dev, 1))
        steps[k] = max(1, min(5, int(40.0 / max(once, 1e-3))))      # about 40 ms a sample, at most five submits
    order = list(sides) + [k + "'" for k in sides]
    t = {k: [] for k in order}
    for _ in range(reps):
        for key in order:
            k = key.rstrip("'")
            t[key].append(ev.time(dev, lambda: sides[k].run(dev, steps[k])) / steps[k])
    med = {k: statistics.median(v) for k, v in t.items()}

    def both(k):
        return min(med[k], med[k + "'"]), max(med[k], med[k + "'"])
    (af, as_), (bf, bs), (cf, cs) = both("a"), both("b"), both("c")
    spread = max((as_ - af) / af, (bs - bf) / bf, (cs - cf) / cf)
    row = {"case": f"{'real ' if real else ''}{batch} x {'x'.join(map(str, shape))} (*) {'x'.join(map(str, ks))} linear-same C={C} K={K} G={G}",
           "class": ("depthwise" if Cg == 1 else "sum") + (" real" if real else " complex"),
           "route_a": sides["a"].route.strip().split(" ")[-1], "launches_a": sides["a"].launches, "work_kib_a": round(sides["a"].work / 1024, 1),
           "ms_a": [round(af, 4), round(as_, 4)], "spread_pct_a": round(100 * (as_ - af) / af, 1),
           "route_b": sides["b"].route.strip().split(" ")[-1], "launches_b": sides["b"].launches,
           "ms_b": [round(bf, 4), round(bs, 4)], "spread_pct_b": round(100 * (bs - bf) / bf, 1), "b_over_a": round(bf / as_, 2),
           "route_c": f"{G} x " + sides["c"].route.strip().split(" ")[-1], "launches_c": sides["c"].launches,
           "ms_c": [round(cf, 4), round(cs, 4)], "spread_pct_c": round(100 * (cs - cf) / cf, 1), "c_over_a": round(cf / as_, 2),
           "a_ahead_of_both": bool(bf / as_ > 1 + spread and cf / as_ > 1 + spread)}
    print(json.dumps(row), flush=True)
    for s in sides.values():
        s.plan.destroy()
    for b in (x, h, out):
        b.destroy()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the request list (default: all)")
    ap.add_argument("--only", choices=["complex", "real"], default=None)
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    rows = []
    for real in (False, True):
        if args.only and (args.only == "real") != real:
            continue
        for req in range(len(REQUESTS)):
            if args.cases is None or req in args.cases:
                try:
                    rows.append(case(dev, ev, real, req, args.reps))
                except mi355fft.Mi355Error as e:        # (a request the device cannot hold: reported, the sweep goes on)
                    print(json.dumps({"case": f"request {req} real={real}", "error": str(e)}), flush=True)
    for cls in sorted({r["class"] for r in rows}):
        mine = [r for r in rows if r["class"] == cls]
        print(json.dumps({"class": cls, "requests": len(mine), "enters_the_rule": all(r["a_ahead_of_both"] for r in mine),
                          "b_over_a": [r["b_over_a"] for r in mine], "c_over_a": [r["c_over_a"] for r in mine]}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
