#!/usr/bin/env python3
"""Complex fftconv of long lines with short kernels: the overlap-save route against the plan the planner gave before it, plans of one request
in one process, timed alternately with hipEvents on the library's stream (K back-to-back submits of one recorded exec per sample, the
median of R samples).  The method of tools/fftconv_ols_ab.py:

  P     MI355FFT_CONV_OLS=P, P in {512, 1024, 2048, 4096} where a block gives L >= 2 results: lines-mapped for the kernels, then
        lines-conv-ols, one launch per kernel over batch * ceil(fN / L) block-lines
  old   MI355FFT_CONV_OLS=0: pad[..] + the composed route fftconv[K], or fftconv-pipeline-view on a 2^20-point domain; above 2^22 the
        planner had no plan (an exact-length Bluestein axis): "old" is null and the row reports absolute throughput alone

Every P is sampled twice per round (P..., old, P... again): the distance between its two medians is the run-to-run spread the comparison
has to be read against.  One JSON line per request: routes, launches, workspace, device ms per exec, G complex points of `shape` per second
and kernel (batch * shape * kernelCount / time), old / P time ratios, the bytes the route moves per point and kernel by construction
(16 P / L: 8 B read and 8 B written per block position) and the bandwidth that comes to.  Inputs and kernels come from the device PRNG.

  python tools/fftconv_cols_ab.py [--steps K] [--reps R] [--cases 0 1 ...] [--blocks 512 1024 2048 4096] [--request BATCH SHAPE KERNEL MODE K]"""
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

# (batch, shape, kernelShape, mode, kernelCount): linear-same, about 1 GiB of complex input where the earlier plan's workspace allows it
CASES = [(128, 1 << 20, kn, "convolution", K) for kn in (31, 255, 513) for K in (1, 4)] + [
    (1024, 100000, 129, "correlation", 1),
    (128, 700000, 255, "convolution", 1),       # padded domain 2^20: the earlier plan is fftconv-pipeline-view
    (16, 5000000, 255, "convolution", 1),       # no earlier plan
    (32, 1 << 22, 255, "convolution", 1),       # no earlier plan
]
SWITCH = "MI355FFT_CONV_OLS"


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
    opts = {"type": "fftconv", "shape": [n], "batch": batch,
            "fftConv": {"mode": mode, "boundary": "linear-same", "kernelCount": K, "kernelShape": [kn]}}
    x, h, out = dev.createBuffer({"size": 8 * n * batch}), dev.createBuffer({"size": 8 * kn * K}), dev.createBuffer({"size": 8 * n * batch * K})
    fill(dev, x, 8 * n * batch, 0x5EED0F11)
    fill(dev, h, 8 * kn * K, 0x5EED0F12)
    pre = kn - 1
    sides = {str(P): Side(dev, opts, str(P), x, h, out) for P in blocks if P - pre >= 2}
    old_error = None
    try:
        sides["old"] = Side(dev, opts, "0", x, h, out)
    except mi355fft.Mi355Error as e:
        old_error = str(e)
    for s in sides.values():
        s.run(dev, 2)
    dev.queue.onSubmittedWorkDone()
    ps = [k for k in sides if k != "old"]
    order = ps + (["old"] if "old" in sides else []) + [p + "'" for p in ps]
    t = {k: [] for k in order}
    for _ in range(reps):
        for key in order:
            s = sides[key.rstrip("'")]
            t[key].append(ev.time(dev, lambda: s.run(dev, steps)) / steps)
    med = {k: statistics.median(v) for k, v in t.items()}
    pts = n * batch * K
    row = {"case": f"{batch} x {n} (*) {kn} {mode} K={K}", "input_gib": round(8 * n * batch / (1 << 30), 3)}
    if "old" in sides:
        row.update({"route_old": sides["old"].route.strip(), "launches_old": sides["old"].launches, "work_mib_old": round(sides["old"].work / (1 << 20), 1),
                    "ms_old": round(med["old"], 4), "gcplx_per_s_old": round(pts / med["old"] / 1e6, 1)})
    else:
        row.update({"route_old": None, "error_old": old_error})
    for p in ps:
        assert "lines-conv-ols[N=" + p in sides[p].route, sides[p].route
        L = int(p) - pre
        slow = max(med[p], med[p + "'"])
        row[f"P{p}"] = {"L": L, "launches": sides[p].launches, "work_kib": round(sides[p].work / 1024, 1),
                        "ms": [round(med[p], 4), round(med[p + "'"], 4)],
                        "gcplx_per_s": [round(pts / med[p] / 1e6, 1), round(pts / med[p + "'"] / 1e6, 1)],
                        "old_over_ols": round(med["old"] / slow, 3) if "old" in sides else None,
                        "bytes_per_point": round(16 * int(p) / L, 2),
                        "tb_per_s": round(16 * int(p) / L * pts / slow / 1e9, 2)}
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
    ap.add_argument("--blocks", type=int, nargs="*", default=[512, 1024, 2048, 4096])
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
