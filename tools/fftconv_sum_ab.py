#!/usr/bin/env python3
"""fftConv.inputChannels (y[b][k] = sum_c x[b][c] (*) h[k][c]) on rank-2 images with small kernels, complex data or (--real) real data: the sum form
of the overlap-save tile kernel against the composed sum route and against what the library could do before the option, plans of one request in one
process, timed alternately with hipEvents on the library's stream (S back-to-back submits of one recorded exec per sample, the median of R samples).
The method of tools/fftconv_circular_ab.py:

  a  MI355FFT_SUM_OLS2D=64: tiles-(r)spectrum tiles-(r)conv-ols-sum[N=64x64,..,C=c], 1 + K launches
  b  MI355FFT_SUM_OLS2D=0: the composed route fftconv-sum[K,C] / rconv-sum[K,C] (forward transforms of the batch * C lines on the exact domain, one
     multiply-accumulate pass and one inverse per output kernel)
  c  the single-channel tile plan of the same images (batch lines, K kernels, the planner's own rule) executed C times back to back, exec c reading
     channel c's lines (input batch stride C * prod(shape), input offset c * prod(shape)) and K of the kernels, every exec writing the same output:
     the C plans a caller had to run before, WITHOUT the sum of their C K batch partial results, which is extra work on top (so c flatters the parent)

The three forms are sampled twice per round (a, b, c, a', b', c'): the distance between a form's two medians is the run-to-run spread the comparison
has to be read against.  One JSON line per request: routes, launches, workspace, device ms per exec, G input points (batch * C * shape * K) per
second, b / a (the FASTER of b's two medians over the SLOWER of a's) and c / a (the same).  Inputs and kernels come from the device PRNG.  One
process per sweep:

  python tools/fftconv_sum_ab.py [--real] [--reps R] [--cases 0 1 ...] [--channels 3 16 64] [--kernels 1 4]"""
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

SWITCH = "MI355FFT_SUM_OLS2D"
# (batch, shape, kernelShape): the requests of tools/fftconv_tiles_ab.py whose kernels the 64-point tile takes
REQUESTS = [(8, (1024, 1024), (9, 9)), (4, (512, 512), (5, 5)), (3, (1920, 1080), (17, 17))]


def prod(v):
    n = 1
    for s in v:
        n *= s
    return n


def options(real, batch, shape, ks, K, C=None, layout=None):
    opts = {"type": "fftconv", "shape": list(shape), "batch": batch,
            "fftConv": {"mode": "convolution", "boundary": "linear-same", "kernelCount": K, "kernelShape": list(ks)},
            "layout": dict({"interleavedComplex": not real}, **(layout or {}))}
    if C:
        opts["fftConv"]["inputChannels"] = C
    return opts


class Side:
    """one plan (built with the switch at `value`) and one recorded command list: `execs` execs of it, exec c at the offsets offs(c)"""

    def __init__(self, dev, opts, value, inp, kern, out, execs=1, offs=lambda c: (0, 0)):
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
        for c in range(execs):
            io, ko = offs(c)
            self.plan.exec(enc, {"input": inp, "output": out, "kernel": kern, "inputOffsetBytes": io, "kernelOffsetBytes": ko})
        self.cmds = enc.finish(use_graph=False)
        self.route, self.launches = self.plan.describe()
        self.launches *= execs
        self.work = self.plan.getWorkspaceSizeBytes()

    def run(self, dev, k):
        for _ in range(k):
            dev.queue.submit([self.cmds])


def case(dev, ev, real, req, C, K, reps):
    batch, shape, ks = REQUESTS[req]
    E = 4 if real else 8
    n, kn = prod(shape), prod(ks)
    x, h, out = dev.createBuffer({"size": E * n * batch * C}), dev.createBuffer({"size": E * kn * K * C + 8}), dev.createBuffer({"size": E * n * batch * K})
    fill(dev, x, E * n * batch * C, 0x5EED5C00)
    fill(dev, h, E * kn * K * C, 0x5EED5C01)
    summed = options(real, batch, shape, ks, K, C)
    strides, st = [], 1
    for s in shape:
        strides.append(st)
        st *= s
    single = options(real, batch, shape, ks, K, None, {"inputStrides": strides, "inputBatchStrideElements": C * n})
    sides = {"a": Side(dev, summed, "64", x, h, out), "b": Side(dev, summed, "0", x, h, out),
             "c": Side(dev, single, None, x, h, out, C, lambda c: (E * n * c, E * kn * K * c // 8 * 8))}      # (exec offsets are multiples of 8 bytes)
    r = "r" if real else ""
    assert f"tiles-{r}conv-ols-sum[N=64x64" in sides["a"].route and sides["a"].launches == 1 + K, sides["a"].route
    assert (r or "fft") + "conv-sum[K=" in sides["b"].route and "ols" not in sides["b"].route, sides["b"].route
    assert f"tiles-{r}conv-ols[N=64x64" in sides["c"].route and sides["c"].launches == C * (1 + K), sides["c"].route
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
    pts = n * batch * C * K
    words = sides["b"].route.strip().split(" ")
    row = {"case": f"{'real ' if real else ''}{batch} x {'x'.join(map(str, shape))} (*) {'x'.join(map(str, ks))} linear-same C={C} K={K}",
           "input_mib": round(E * n * batch * C / (1 << 20), 1),
           "route_a": sides["a"].route.strip().split(" ")[-1], "launches_a": sides["a"].launches, "work_kib_a": round(sides["a"].work / 1024, 1),
           "ms_a": [round(af, 4), round(as_, 4)], "spread_pct_a": round(100 * (as_ - af) / af, 1), "gpoints_per_s_a": round(pts / as_ / 1e6, 1),
           "route_b": words[0] + " ... " + words[-1], "launches_b": sides["b"].launches, "work_mib_b": round(sides["b"].work / (1 << 20), 1),
           "ms_b": [round(bf, 4), round(bs, 4)], "spread_pct_b": round(100 * (bs - bf) / bf, 1), "b_over_a": round(bf / as_, 2),
           "route_c": f"{C} x " + sides["c"].route.strip().split(" ")[-1], "launches_c": sides["c"].launches,
           "ms_c": [round(cf, 4), round(cs, 4)], "spread_pct_c": round(100 * (cs - cf) / cf, 1), "c_over_a": round(cf / as_, 2)}
    print(json.dumps(row), flush=True)
    for s in sides.values():
        s.plan.destroy()
    for b in (x, h, out):
        b.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--real", action="store_true", help="real data")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--channels", type=int, nargs="*", default=[3, 16, 64])
    ap.add_argument("--kernels", type=int, nargs="*", default=[1, 4], help="kernelCount values")
    ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the request list (default: all)")
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    for C in args.channels:
        for req in range(len(REQUESTS)):
            if args.cases is None or req in args.cases:
                for K in args.kernels:
                    try:
                        case(dev, ev, args.real, req, C, K, args.reps)
                    except mi355fft.Mi355Error as e:        # (a request the device cannot hold: reported, the sweep goes on)
                        print(json.dumps({"case": f"request {req} C={C} K={K}", "error": str(e)}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
