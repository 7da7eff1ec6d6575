#!/usr/bin/env python3
"""fftconv over real data, three plans of the same request in one process, timed alternately with hipEvents on the library's stream
(K back-to-back submits of one recorded exec per sample, the median of R samples):

  a  the real plan on the one-launch line route (MI355FFT_RCONV_FUSED=2: every length up to 32768): lines-r2c-mapped for the kernels, then
     lines-rconv, one launch per kernel
  b  MI355FFT_RCONV_FUSED=0: the composed real route rconv[K] (r2c, pointwise pass over the packed bins, c2r)
  c  the complex plan on the same lines widened to complex — what a caller of the complex-only library runs; its own widen and
     narrow passes are not charged

`a` is sampled twice per round (a, b, c, a): the distance between its two medians and the min..max of its samples are the
run-to-run spread the comparison has to be read against.  One JSON line per case: routes, launches, device ms per exec and
G real points of `shape` per second and kernel (batch * shape * kernelCount / time).  Inputs and kernels come from the device PRNG.

  python tools/fftconv_real_ab.py [--steps K] [--reps R] [--gib G] [--kernels 1 4] [--cases 0 1 ...]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-fft_amd", "python"), os.path.join(ROOT, "tools")]
from f16_storage_ab import Events  # noqa: E402  (also loads torch's HIP runtime first, as the tests do)
import mi355fft  # noqa: E402

# (name, shape, kernelShape, boundary, mode)
CASES = [("circular 1024", 1024, 1024, "circular", "convolution"),
         ("circular 4096", 4096, 4096, "circular", "convolution"),
         ("circular 8192", 8192, 8192, "circular", "convolution"),
         ("circular 16384", 16384, 16384, "circular", "convolution"),
         ("circular 32768", 32768, 32768, "circular", "convolution"),
         ("same corr 4000 (*) 97 -> 4096", 4000, 97, "linear-same", "correlation"),
         ("circular 256", 256, 256, "circular", "convolution"),
         ("circular 2048", 2048, 2048, "circular", "convolution")]
SWITCH = "MI355FFT_RCONV_FUSED"


class Side:
    """one plan of the request (built with the switch at `fused`) with its output buffer and one recorded exec"""

    def __init__(self, dev, opts, fused, inp, kern, out_bytes):
        saved = os.environ.get(SWITCH)
        os.environ.pop(SWITCH, None)
        if fused is not None:
            os.environ[SWITCH] = fused
        try:
            self.plan = mi355fft.createPlan(dev, opts)
        finally:
            os.environ.pop(SWITCH, None)
            if saved is not None:
                os.environ[SWITCH] = saved
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
    batch = max(1, total // (4 * n))
    on = {"circular": n, "linear-full": n + kn - 1, "linear-same": n, "linear-valid": n - kn + 1}[boundary]
    conv = {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": [kn]}
    real = {"type": "fftconv", "shape": [n], "batch": batch, "layout": {"interleavedComplex": False}, "fftConv": conv}
    cplx = {"type": "fftconv", "shape": [n], "batch": batch, "fftConv": conv}
    xr, hr = dev.createBuffer({"size": 4 * n * batch}), dev.createBuffer({"size": 4 * kn * K})
    xc, hc = dev.createBuffer({"size": 8 * n * batch}), dev.createBuffer({"size": 8 * kn * K})
    for i, (b, nb) in enumerate(((xr, 4 * n * batch), (hr, 4 * kn * K), (xc, 8 * n * batch), (hc, 8 * kn * K))):
        fill(dev, b, nb, 0x5EED0D11 + i)
    sides = {"a": Side(dev, real, "2", xr, hr, 4 * on * batch * K), "b": Side(dev, real, "0", xr, hr, 4 * on * batch * K),
             "c": Side(dev, cplx, None, xc, hc, 8 * on * batch * K)}
    for s in sides.values():
        s.run(dev, 2)
    dev.queue.onSubmittedWorkDone()
    t = {"a": [], "b": [], "c": [], "a2": []}
    for _ in range(reps):
        for key in ("a", "b", "c", "a2"):
            s = sides[key[0]]
            t[key].append(ev.time(dev, lambda: s.run(dev, steps)) / steps)
    med = {k: statistics.median(v) for k, v in t.items()}
    pts = n * batch * K
    row = {"case": f"{name} x {batch}, K={K}", "input_gib": round(4 * n * batch / (1 << 30), 3)}
    for k in ("a", "b", "c"):
        row[f"route_{k}"] = sides[k].route.strip()
        row[f"launches_{k}"] = sides[k].launches
    for k in ("a", "a2", "b", "c"):
        row[f"ms_{k}"] = round(med[k], 4)
        row[f"greal_per_s_{k}"] = round(pts / med[k] / 1e6, 1)
    both = t["a"] + t["a2"]
    row["a_samples_min_max_ms"] = [round(min(both), 4), round(max(both), 4)]
    row["b_over_a"] = round(med["b"] / med["a"], 3)
    row["c_over_a"] = round(med["c"] / med["a"], 3)
    print(json.dumps(row), flush=True)
    for s in sides.values():
        s.destroy()
    for b in (xr, hr, xc, hc):
        b.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gib", type=float, default=1.0, help="real input bytes per case (GiB)")
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
