#!/usr/bin/env python3
"""Real fftconv of long lines with short kernels: the overlap-save route against the plan the planner gave before it, plans of one request
in one process, timed alternately with hipEvents on the library's stream (K back-to-back submits of one recorded exec per sample, the
median of R samples):

  P     MI355FFT_RCONV_OLS=P, P in {1024, 2048, 4096, 8192} where a block gives L >= 2 results: lines-r2c-mapped for the kernels, then
        lines-rconv-ols, one launch per kernel over batch * ceil(fN / L) block-lines
  old   MI355FFT_RCONV_OLS=0: pad[..] + the composed real route rconv[K], or Bluestein above 2^22

Every P is sampled twice per round (P..., old, P... again): the distance between its two medians is the run-to-run spread the comparison
has to be read against.  One JSON line per request: routes, launches, workspace, device ms per exec, G real points of `shape` per second
and kernel (batch * shape * kernelCount / time), old / P time ratios, and the bytes the route moves per point and kernel by construction
(8 P / L: 4 B read and 4 B written per block position).  Inputs and kernels come from the device PRNG.

  python tools/fftconv_ols_ab.py [--steps K] [--reps R] [--cases 0 1 ...] [--blocks 1024 2048 4096 8192] [--request BATCH SHAPE KERNEL MODE K]"""
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

# (batch, shape, kernelShape, mode, kernelCount): linear-same, about 1 GiB of real input where the earlier plan's workspace allows it
CASES = [(256, 1 << 20, kn, "convolution", K) for kn in (31, 255, 1024, 4096) for K in (1, 4)] + [
    (64, 1 << 22, 255, "convolution", 1),
    (16, 5000000, 255, "convolution", 1),
    (2048, 100000, 129, "correlation", 1),
]
SWITCH = "MI355FFT_RCONV_OLS"


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


def case(dev, ev, batch, n, kn, mode, K, blocks, steps, reps):
    opts = {"type": "fftconv", "shape": [n], "batch": batch, "layout": {"interleavedComplex": False},
            "fftConv": {"mode": mode, "boundary": "linear-same", "kernelCount": K, "kernelShape": [kn]}}
    x, h, out = dev.createBuffer({"size": 4 * n * batch}), dev.createBuffer({"size": 4 * kn * K}), dev.createBuffer({"size": 4 * n * batch * K})
    fill(dev, x, 4 * n * batch, 0x5EED0E11)
    fill(dev, h, 4 * kn * K, 0x5EED0E12)
    pre = (kn - 1) + ((kn - 1) & 1)
    sides = {str(P): Side(dev, opts, str(P), x, h, out) for P in blocks if ((P - pre) & ~1) >= 2}
    sides["old"] = Side(dev, opts, "0", x, h, out)
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
    row = {"case": f"{batch} x {n} (*) {kn} {mode} K={K}", "input_gib": round(4 * n * batch / (1 << 30), 3),
           "route_old": sides["old"].route.strip(), "launches_old": sides["old"].launches, "work_mib_old": round(sides["old"].work / (1 << 20), 1),
           "ms_old": round(med["old"], 4), "greal_per_s_old": round(pts / med["old"] / 1e6, 1)}
    for p in ps:
        assert "lines-rconv-ols[N=" + p in sides[p].route, sides[p].route
        L = (int(p) - pre) & ~1
        row[f"P{p}"] = {"L": L, "launches": sides[p].launches, "work_kib": round(sides[p].work / 1024, 1),
                        "ms": [round(med[p], 4), round(med[p + "'"], 4)],
                        "greal_per_s": [round(pts / med[p] / 1e6, 1), round(pts / med[p + "'"] / 1e6, 1)],
                        "old_over_ols": round(med["old"] / max(med[p], med[p + "'"]), 3),
                        "bytes_per_point": round(8 * int(p) / L, 2)}
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
    ap.add_argument("--blocks", type=int, nargs="*", default=[1024, 2048, 4096, 8192])
    ap.add_argument("--request", nargs=5, metavar=("BATCH", "SHAPE", "KERNEL", "MODE", "K"), help="one request instead of the case list (profiler runs)")
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    if args.request:
        batch, n, kn, mode, K = args.request
        case(dev, ev, int(batch), int(n), int(kn), mode, int(K), args.blocks, args.steps, args.reps)
    for i, (batch, n, kn, mode, K) in enumerate([] if args.request else CASES):
        if args.cases is None or i in args.cases:
            case(dev, ev, batch, n, kn, mode, K, args.blocks, args.steps, args.reps)
    dev.close()


if __name__ == "__main__":
    main()
