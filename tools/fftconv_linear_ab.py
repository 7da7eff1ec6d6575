#!/usr/bin/env python3
"""Long rank-1 linear fftconv requests, three plans of the same request in one process, timed alternately with hipEvents on the
library's stream (K back-to-back submits of one recorded exec per sample, the median of R samples):

  a  the default plan: padded power-of-two domain, one-launch pipeline in its VIEW form where the domain is 2^20 points
  b  MI355FFT_CONV_PIPELINE=0: the composed route (zero + embed, forward, products, inverse, crop) on the same padded domain
  c  MI355FFT_CONV_PAD=0: the exact-length domain shape + kernelShape - 1 (Bluestein / mixed-radix transforms)

`a` is sampled twice per round (a, b, c, a): the distance between its two medians and the min..max of its samples are the
run-to-run spread the comparison has to be read against.  One JSON line per case: routes, launches, device ms per exec and
G points of `shape` per second (batch * shape / time).  Inputs and kernels come from the device PRNG.

  python tools/fftconv_linear_ab.py [--steps K] [--reps R] [--gib G] [--kernels 1 4]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-fft_amd", "python"), os.path.join(ROOT, "tools")]
from f16_storage_ab import Events  # noqa: E402  (also loads torch's HIP runtime first, as the tests do)
import mi355fft  # noqa: E402

CASES = [("same conv 524288 (*) 524288", 524288, 524288, "linear-same", "convolution"),
         ("full corr 524288 (*) 300000", 524288, 300000, "linear-full", "correlation"),
         ("same conv 524288 (*) 1024", 524288, 1024, "linear-same", "convolution")]
ENVS = {"a": {}, "b": {"MI355FFT_CONV_PIPELINE": "0"}, "c": {"MI355FFT_CONV_PAD": "0"}}


class Side:
    """one plan of the request (built under `env`) with its output buffer and one recorded exec"""

    def __init__(self, dev, opts, env, inp, kern, out_bytes):
        saved = {k: os.environ.get(k) for k in ("MI355FFT_CONV_PIPELINE", "MI355FFT_CONV_PAD")}
        for k in saved:
            os.environ.pop(k, None)
        os.environ.update(env)
        try:
            self.plan = mi355fft.createPlan(dev, opts)
        finally:
            for k, v in saved.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        self.out = dev.createBuffer({"size": out_bytes})
        enc = dev.createCommandEncoder()
        self.plan.exec(enc, {"input": inp, "output": self.out, "kernel": kern})
        self.cmds = enc.finish(use_graph=False)
        self.route, self.launches = self.plan.describe()

    def run(self, dev, k):
        for _ in range(k):
            dev.queue.submit([self.cmds])

    def destroy(self):
        self.plan.destroy()
        self.out.destroy()


def fill(dev, buf, nbytes, seed):
    mi355fft._chk(mi355fft.lib().mi355fft_fill_random(dev._h, buf._h, 0, nbytes // 4, 1, seed, 0))


def case(dev, ev, name, n, kn, boundary, mode, K, total, steps, reps):
    batch = max(1, total // (8 * n))
    on = {"linear-full": n + kn - 1, "linear-same": n, "linear-valid": n - kn + 1}[boundary]
    opts = {"type": "fftconv", "shape": [n], "batch": batch, "fftConv": {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": [kn]}}
    inp = dev.createBuffer({"size": 8 * n * batch})
    kern = dev.createBuffer({"size": 8 * kn * K})
    fill(dev, inp, 8 * n * batch, 0x5EED0C11)
    fill(dev, kern, 8 * kn * K, 0x5EED0C12)
    sides = {k: Side(dev, opts, env, inp, kern, 8 * on * batch * K) for k, env in ENVS.items()}
    for s in sides.values():
        s.run(dev, 2)
    dev.queue.onSubmittedWorkDone()
    t = {"a": [], "b": [], "c": [], "a2": []}
    for _ in range(reps):
        for key in ("a", "b", "c", "a2"):
            s = sides[key[0]]
            t[key].append(ev.time(dev, lambda: s.run(dev, steps)) / steps)
    med = {k: statistics.median(v) for k, v in t.items()}
    pts = n * batch
    row = {"case": f"{name} x {batch}, K={K}", "fft_domain": n + kn - 1}
    for k in ("a", "b", "c"):
        row[f"route_{k}"] = sides[k].route.strip()
        row[f"launches_{k}"] = sides[k].launches
    for k in ("a", "a2", "b", "c"):
        row[f"ms_{k}"] = round(med[k], 4)
        row[f"gpoints_{k}"] = round(pts / med[k] / 1e6, 1)
    both = t["a"] + t["a2"]
    row["a_samples_min_max_ms"] = [round(min(both), 4), round(max(both), 4)]
    row["a_over_b"] = round(med["b"] / med["a"], 3)
    row["b_over_c"] = round(med["c"] / med["b"], 3)
    print(json.dumps(row), flush=True)
    for s in sides.values():
        s.destroy()
    inp.destroy()
    kern.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gib", type=float, default=1.0, help="input bytes per case (GiB)")
    ap.add_argument("--kernels", type=int, nargs="*", default=[1, 4])
    ap.add_argument("--cases", type=int, nargs="*", default=None, help="indices into the case list (default: all)")
    args = ap.parse_args()
    dev = mi355fft.Device(0)
    ev = Events()
    for i, (name, n, kn, boundary, mode) in enumerate(CASES):
        if args.cases is not None and i not in args.cases:
            continue
        for K in args.kernels:
            case(dev, ev, name, n, kn, boundary, mode, K, int(args.gib * (1 << 30)), args.steps, args.reps)
    dev.close()


if __name__ == "__main__":
    main()
