#!/usr/bin/env python3
"""Circular fftconv with short kernels, complex data or (--real) real data: the wrapping form of the overlap-save routes against the plan of
MI355FFT_OLS_CIRCULAR=0 (what the planner gave before), and against the LINEAR request of the same shape on the same route, plans of one request in
one process, timed alternately with hipEvents on the library's stream (K back-to-back submits of one recorded exec per sample, the median of R
samples).  The method of tools/fftconv_tiles_ab.py:

  wrap  MI355FFT_OLS_CIRCULAR=2 (every request inside the bounds, power-of-two domains included): ...-ols[..,wrap], 1 + K launches
  old   MI355FFT_OLS_CIRCULAR=0: Bluestein / mixed-radix / per-radix stages / power-of-two lines per axis, fftconv[K], rconv[K], fftconv-pipeline;
        "none" where the request has no plan at all
  lin   the same shape, kernels and data with boundary "linear-same" under the default switches: the same kernel's linear instance on (nearly) the
        same number of blocks.  wrap / lin is the cost of the wrap

The three forms are sampled twice per round (wrap, old, lin, wrap', old', lin'): the distance between a form's two medians is the run-to-run spread
the comparison has to be read against.  One JSON line per request: routes, launches, workspace, device ms per exec, G points of `shape` per second
and kernel (batch * shape * kernelCount / time), old / wrap (the FASTER of the old plan's two medians over the SLOWER of the route's) and wrap / lin
(the slower of wrap over the faster of lin).  Inputs and kernels come from the device PRNG.  One process per sweep:

  python tools/fftconv_circular_ab.py --rank {1,2,3} [--real] [--steps K] [--reps R] [--cases 0 1 ...]"""
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

SWITCH = "MI355FFT_OLS_CIRCULAR"
# (batch, shape, kernelShape) per rank: two domains that are no power of two, then the power-of-two domain the default rule leaves alone
REQUESTS = {
    1: [(256, (1000000,), (255,)), (16, (5000000,), (255,)), (512, (1 << 20,), (255,))],
    2: [(8, (1000, 1000), (9, 9)), (3, (1920, 1080), (17, 17)), (8, (1024, 1024), (9, 9))],
    3: [(1, (250, 250, 250), (5, 5, 5)), (1, (500, 300, 200), (5, 5, 3)), (1, (256, 256, 256), (3, 3, 3))],
}
TAGS = {(1, False): "lines-conv-ols[", (1, True): "lines-rconv-ols[", (2, False): "tiles-conv-ols[", (2, True): "tiles-rconv-ols[",
        (3, False): "bricks-conv-ols[", (3, True): "bricks-rconv-ols["}


class Side:
    """one plan of the request (built with the switch at `value`) and one recorded exec into the shared output buffer; plan = None: no plan"""

    def __init__(self, dev, opts, value, inp, kern, out):
        saved = os.environ.get(SWITCH)
        if value is not None:
            os.environ[SWITCH] = value
        try:
            self.plan = mi355fft.createPlan(dev, opts)
        except Exception as e:
            if "Unsupported" not in str(e):
                raise
            self.plan, self.route, self.launches, self.work = None, "none (" + str(e).strip() + ")", 0, 0
            return
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


def prod(v):
    n = 1
    for s in v:
        n *= s
    return n


def options(real, batch, shape, ks, boundary, K):
    opts = {"type": "fftconv", "shape": list(shape), "batch": batch, "fftConv": {"mode": "convolution", "boundary": boundary, "kernelCount": K, "kernelShape": list(ks)}}
    if real:
        opts["layout"] = {"interleavedComplex": False}
    return opts


def case(dev, ev, rank, real, req, K, steps, reps):
    batch, shape, ks = REQUESTS[rank][req]
    E = 4 if real else 8
    n, kn = prod(shape), prod(ks)
    x, h, out = dev.createBuffer({"size": E * n * batch}), dev.createBuffer({"size": E * kn * K}), dev.createBuffer({"size": E * n * batch * K})
    fill(dev, x, E * n * batch, 0x5EEDC1C0)
    fill(dev, h, E * kn * K, 0x5EEDC1C1)
    circular, linear = options(real, batch, shape, ks, "circular", K), options(real, batch, shape, ks, "linear-same", K)
    sides = {"wrap": Side(dev, circular, "2", x, h, out), "old": Side(dev, circular, "0", x, h, out), "lin": Side(dev, linear, None, x, h, out)}
    tag = TAGS[(rank, real)]
    assert tag in sides["wrap"].route and ",wrap]" in sides["wrap"].route and sides["wrap"].launches == 1 + K, sides["wrap"].route
    assert tag in sides["lin"].route and "wrap" not in sides["lin"].route and sides["lin"].launches == 1 + K, sides["lin"].route
    assert tag not in sides["old"].route, sides["old"].route
    timed = [k for k, s in sides.items() if s.plan is not None]
    for k in timed:
        sides[k].run(dev, 2)
    dev.queue.onSubmittedWorkDone()
    order = timed + [k + "'" for k in timed]
    t = {k: [] for k in order}
    for _ in range(reps):
        for key in order:
            s = sides[key.rstrip("'")]
            t[key].append(ev.time(dev, lambda: s.run(dev, steps)) / steps)
    med = {k: statistics.median(v) for k, v in t.items()}
    pts = n * batch * K

    def both(k):
        return (min(med[k], med[k + "'"]), max(med[k], med[k + "'"])) if k in timed else (None, None)
    (wf, ws), (of, os_), (lf, ls) = both("wrap"), both("old"), both("lin")
    words = sides["old"].route.strip().split(" ")
    row = {"case": f"{'real ' if real else ''}{batch} x {'x'.join(map(str, shape))} (*) {'x'.join(map(str, ks))} circular K={K}",
           "input_mib": round(E * n * batch / (1 << 20), 1),
           "route_old": (words[0] + " ... " + words[-1]) if sides["old"].plan is not None else sides["old"].route, "launches_old": sides["old"].launches,
           "work_mib_old": round(sides["old"].work / (1 << 20), 1),
           "ms_old": [round(of, 4), round(os_, 4)] if of else None, "spread_pct_old": round(100 * (os_ - of) / of, 1) if of else None,
           "gpoints_per_s_old": round(pts / of / 1e6, 1) if of else None,
           "route": sides["wrap"].route.strip().split(" ")[-1], "launches": sides["wrap"].launches, "work_kib": round(sides["wrap"].work / 1024, 1),
           "ms": [round(wf, 4), round(ws, 4)], "spread_pct": round(100 * (ws - wf) / wf, 1), "gpoints_per_s": round(pts / ws / 1e6, 1),
           "old_over_wrap": round(of / ws, 2) if of else None,
           "route_linear": sides["lin"].route.strip().split(" ")[-1], "ms_linear": [round(lf, 4), round(ls, 4)], "spread_pct_linear": round(100 * (ls - lf) / lf, 1),
           "wrap_over_linear": round(ws / lf, 3)}
    print(json.dumps(row), flush=True)
    for s in sides.values():
        if s.plan is not None:
            s.plan.destroy()
    for b in (x, h, out):
        b.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rank", type=int, choices=(1, 2, 3), required=True)
    ap.add_argument("--real", action="store_true", help="real data")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the case list (default: all): request r with K = 1 is 2 r, with K = 4 is 2 r + 1")
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    for i, (req, K) in enumerate((r, K) for r in range(len(REQUESTS[args.rank])) for K in (1, 4)):
        if args.cases is None or i in args.cases:
            case(dev, ev, args.rank, args.real, req, K, args.steps, args.reps)
    dev.close()


if __name__ == "__main__":
    main()
