#!/usr/bin/env python3
"""Snapshot of the planner's output over a fixed descriptor corpus (host only, nothing is executed).

One line per case and environment: case name, environment, status, and the SHA-1 of the plan's IR dump (tests/emu emu_plan_dump: every
step with all its scalars and both side maps, workspace and extent bytes, route, table hash) — or the error text when planning fails.
Two builds of the planner plan alike when their snapshots are equal:

    MI355_EMU_LIB=<parent build>/libmi355emu.so python tools/plan_snapshot.py -o parent.txt
    MI355_EMU_LIB=<this build>/libmi355emu.so   python tools/plan_snapshot.py -o branch.txt
    python tools/plan_snapshot.py --compare parent.txt branch.txt

Without MI355_EMU_LIB the library is built from this tree (tests/emu/Makefile).  --full writes the dumps themselves.  --env NAME=VALUE
adds a planner switch to every environment (a build that does not know the switch plans as ever): MI355FFT_RCONV_OLS=0 or MI355FFT_CONV_OLS=0
on both sides compares a planner with that overlap-save route switched off against one without it.  The fftconv corpora are also planned
with each overlap-save switch forcing a block (CONV_ENVS); the other corpora never read those switches.
"""
import argparse
import hashlib
import itertools
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "webgpu-fft_amd", "python"), os.path.join(ROOT, "tests")]

from mi355fft import _abi  # noqa: E402

ENVS = [{}, {"MI355FFT_CONV_PAD": "0"}, {"MI355FFT_CONV_PIPELINE": "0"}, {"MI355FFT_CONV_LINES": "0"}, {"MI355FFT_RCONV_FUSED": "0"},
        {"MI355FFT_RCONV_FUSED": "2"}, {"MI355FFT_FORCE_GENERIC": "1"}, {"MI355FFT_FUSE_VIEWS": "0"}]
# fftconv only: a forced block on each overlap-save route, and a value that is no legal tile (the switch decoder's reject path)
CONV_ENVS = [{"MI355FFT_CONV_OLS": "256"}, {"MI355FFT_RCONV_OLS": "256"}, {"MI355FFT_CONV_OLS2D": "64"}, {"MI355FFT_RCONV_OLS2D": "128"},
             {"MI355FFT_CONV_OLS2D": "100"}]
BOUNDARIES = ["circular", "linear-full", "linear-same", "linear-valid"]
MODES = ["convolution", "correlation"]
LAYOUTS = ["kernel-major", "batch-major"]
EXTRA_ENV = {}      # --env: set in every environment (inherited by the worker processes)


def strided(shape, mult=2, offset=3, pad=5, batch_stride=True):
    """A lane layout over `shape`: element stride `mult`, an offset, batches `pad` elements apart beyond the dense extent."""
    strides, s = [], mult
    for n in shape:
        strides.append(s)
        s *= n
    spec = {"strides": strides, "offset": offset}
    if batch_stride:
        spec["batch_stride"] = s + pad
    return spec


def zrange(shape, lo_frac=8, hi_frac=4):
    return {"start": [n // lo_frac for n in shape], "end": [max(n // lo_frac, n - n // hi_frac) for n in shape]}


def conv_domain(shape, ks, boundary):
    k = ks or shape
    return list(shape) if boundary == "circular" else [n + m - 1 for n, m in zip(shape, k)]


def conv_out_shape(shape, ks, boundary):
    k = ks or shape
    if boundary in ("circular", "linear-same"):
        return list(shape)
    if boundary == "linear-full":
        return [n + m - 1 for n, m in zip(shape, k)]
    return [max(1, n - m + 1) for n, m in zip(shape, k)]


def conv_case(real, shape, ks=None, boundary="circular", mode="convolution", K=1, layout="kernel-major", batch=4, sin=False, sout=False,
              kstride=True, zr=False, zw=False, **extra):
    conv = {"mode": mode, "boundary": boundary, "kernelCount": K, "outputLayout": layout}
    if ks:
        conv["kernelShape"] = ks
    kw = {}
    os_ = conv_out_shape(shape, ks, boundary)
    if sin:
        kw["input_layout"] = strided(shape)
    if sout:
        kw["output_layout"] = strided(os_)
        if kstride:
            n = 1
            for v in os_:
                n *= v
            conv["outputKernelStrideElements"] = (2 * n + 5) * batch + 7
    dom = conv_domain(shape, ks, boundary)
    if zr or zw:
        kw["zero_pad"] = {"read": zrange(dom) if zr else None, "write": zrange(dom, 16, 8) if zw else None}
    kw.update(extra)
    name = "%s %s ks=%s %s/%s K=%d %s B=%d%s%s%s%s%s" % (
        "rconv" if real else "conv", "x".join(map(str, shape)), "x".join(map(str, ks)) if ks else "-", boundary, mode[:4], K, layout[:1], batch,
        " sin" if sin else "", (" sout" if kstride else " sout-nok") if sout else "", " zr" if zr else "", " zw" if zw else "",
        (" " + ",".join(sorted(extra))) if extra else "")
    return name, _abi.make_desc("fftconv-real" if real else "fftconv", shape, batch=batch, conv=conv, **kw)


def side_variants():
    """K, output layout, lanes and zeroPad, one factor at a time (and the lane / zeroPad combinations)."""
    out = [dict(K=K, layout=lay) for K in (1, 3, 16) for lay in LAYOUTS]
    out += [dict(K=3, sin=True), dict(K=3, sout=True), dict(K=1, sout=True, kstride=False), dict(K=3, sin=True, sout=True),
            dict(K=3, sin=True, sout=True, layout="batch-major")]
    out += [dict(K=3, zr=True), dict(K=3, zw=True), dict(K=3, zr=True, zw=True), dict(K=3, zr=True, zw=True, layout="batch-major"),
            dict(K=1, zr=True, zw=True, sin=True, sout=True), dict(K=3, zr=True, sin=True), dict(K=3, zw=True, sout=True)]
    return out


def conv_corpus(real):
    cases = []
    add = lambda *a, **k: cases.append(conv_case(real, *a, **k))  # noqa: E731
    # domains x boundaries x modes, kernelShape given and omitted
    for n in (64, 96, 105, 128, 256, 1000, 1024, 4096, 8192, 16384, 32768):
        for ks, bd, md in itertools.product((None, [7]), BOUNDARIES, MODES):
            add([n], ks, bd, md, K=3)
    # the padded domains: 20000 + 5000 (complex: -> 32768; real: -> 32768 on the line route or the composed one), a real line padded
    # 128 -> 256 and one below 128, a linear-same correlation that straddles the split
    for shape, ks in (([20000], [5000]), ([100], [50]), ([40], [9]), ([12000], [4001])):
        for bd, md, K, lay in itertools.product(BOUNDARIES, MODES, (1, 3), LAYOUTS):
            add(shape, ks, bd, md, K=K, layout=lay)
    bases = [([256], None, "circular", "convolution"), ([256], [9], "linear-same", "correlation"), ([1000], [17], "linear-full", "convolution"),
             ([105], None, "circular", "correlation"), ([96], [5], "circular", "convolution"), ([4096], None, "circular", "convolution"),
             ([16384], [33], "linear-full", "correlation"), ([16384], None, "circular", "convolution"), ([32768], [9], "circular", "correlation"),
             ([20000], [5000], "linear-same", "correlation"), ([20000], [5000], "linear-valid", "convolution"),
             ([20000], [5000], "linear-full", "correlation"), ([100], [50], "linear-same", "correlation"),
             ([32, 16], [5, 3], "linear-same", "correlation"), ([32, 16], [4, 3], "linear-full", "convolution"), ([32, 16], None, "circular", "convolution"),
             ([15, 8], [3, 3], "circular", "correlation"), ([16, 8, 4], [3, 3, 2], "linear-valid", "convolution"), ([64, 32], [64, 32], "circular", "convolution")]
    for (shape, ks, bd, md), v in itertools.product(bases, side_variants()):
        add(shape, ks, bd, md, **v)
    # ranks 2 and 3: pow2, mixed and odd axes; an axis-0 linear length that is odd (the real route rounds it up to even) and one that is even
    for shape, ks in (([32, 16], [5, 3]), ([32, 16], [4, 3]), ([30, 12], [4, 5]), ([16, 8, 4], [3, 3, 2]), ([15, 8, 4], [2, 3, 2]), ([128, 64], [9, 9])):
        for k, bd, md in itertools.product((None, ks), BOUNDARIES, MODES):
            add(shape, k, bd, md, K=3)
            add(shape, k, bd, md, K=1, layout="batch-major", batch=1)
    # the 2^20-point domain: circular dense (pipeline), with zeroPad (its VIEW form), linear with an exact and a padded 2^20 domain, lanes (composed)
    M = 1 << 20
    for K, lay in itertools.product((1, 3), LAYOUTS):
        add([M], [4096], "circular", "convolution", K=K, layout=lay, batch=2)
    add([M], None, "circular", "correlation", K=3, batch=2)
    for v in (dict(zr=True), dict(zw=True), dict(zr=True, zw=True), dict(sin=True), dict(sout=True), dict(sin=True, sout=True, zr=True)):
        add([M], [4096], "circular", "correlation", K=3, batch=2, **v)
    for (shape, ks), bd, md in itertools.product((([M - 4095], [4096]), ([900000], [5000])), BOUNDARIES[1:], MODES):
        add(shape, ks, bd, md, K=3, batch=2)
        add(shape, ks, bd, md, K=1, batch=2, layout="batch-major", zr=True, zw=True)
    add([900000], [5000], "linear-same", "correlation", K=3, batch=2, sin=True, sout=True)
    # the one-launch latency route on both sides of conv_fused_max_points, its K <= 15 bound and its lanes
    for n, K, B in ((1024, 3, 341), (1024, 3, 342), (1024, 15, 8), (1024, 16, 8), (64, 1, 16384), (64, 1, 16385), (64, 4, 100), (512, 3, 7)):
        for md in MODES:
            add([n], [5], "circular", md, K=K, batch=B)
    for v in (dict(sin=True), dict(sout=True), dict(sin=True, sout=True), dict(layout="batch-major"), dict(K=1, sout=True, kstride=False)):
        add([256], [9], "circular", "convolution", **{"K": 3, "batch": 16, **v})
    # circular with odd shape[0] (real: the widened complex plan), even mixed-radix beside it
    for shape, v in itertools.product(([105], [1001], [15, 8], [9, 5, 4], [96], [1000], [30, 12]),
                                      (dict(K=1), dict(K=3), dict(K=3, layout="batch-major"), dict(K=3, zr=True, zw=True), dict(K=16, mode="correlation"))):
        add(shape, [3] * len(shape), "circular", **v)
    # invalid descriptors: every fftconv message
    view = {"input": {"shape": [64], "offset": [0]}}
    cases.append(("%s invalid ioView" % ("rconv" if real else "conv"), _abi.make_desc("fftconv-real" if real else "fftconv", [64], conv={}, io_view=view)))
    add([64], in_place=True)
    for field, val in (("conv_mode", 5), ("conv_boundary", 7), ("conv_boundary", -1), ("conv_kernel_count", 0), ("conv_kernel_count", -2)):
        name, d = conv_case(real, [64])
        setattr(d, field, val)
        cases.append((name + " %s=%d" % (field, val), d))
    name, d = conv_case(real, [64, 32], [5, 3])
    d.conv_kernel_shape[1] = 0
    cases.append((name + " ks[1]=0", d))
    name, d = conv_case(real, [64, 32], [5, 3])
    d.conv_kernel_shape[0] = -4
    cases.append((name + " ks[0]=-4", d))
    add([64], [65], "circular")
    add([64, 32], [5, 33], "circular")
    add([64], [65], "linear-valid")
    add([64, 32], [5, 33], "linear-valid", "correlation")
    add([256], [9], "linear-full", K=3, sout=True, kstride=False)
    add([64, 32], [5, 3], "linear-same", K=3, sout=True, kstride=False)
    for key in ("read", "write"):
        name, d = conv_case(real, [256], [9], "linear-full", zr=True, zw=True)
        getattr(d, "zero_" + key).end[0] = 265
        cases.append((name + " zero_%s.end=265" % key, d))
    add([64, 32], [5, 3], "linear-same", K=1, sin=True)          # real: lanes outside the line route
    add([1000], None, "circular", K=1, sout=True)
    add([256], precision="f16-storage")
    # long lines with short kernels (overlap-save by default: MI355FFT_RCONV_OLS for real data, MI355FFT_CONV_OLS for complex; their 0 restores pad[..]
    # rconv[K] / fftconv[K] or the pipeline and, above 2^22, Bluestein or its refusal)
    add([1 << 20], [1024], "linear-same", K=1, batch=8)
    add([100000], [129], "linear-same", K=2, batch=4)
    add([9000], [33], "linear-same", K=1, batch=4)
    add([5000000], [255], "linear-same", K=1, batch=2)
    add([100000], [129], "linear-full", "correlation", K=2, batch=4, sin=True, sout=True, zr=True, zw=True)
    if not real:
        add([1 << 20], [255], "linear-same", K=4, batch=8)
        add([700000], [255], "linear-valid", "correlation", K=1, batch=4)
        add([20000], [513], "linear-same", K=1, batch=4, layout="batch-major")
    # rank-2 images with small kernels (overlap-save tiles by default: MI355FFT_CONV_OLS2D for complex data, MI355FFT_RCONV_OLS2D for real; P = 64, P = 128,
    # and an even kernel with an odd number of tiles on axis 1)
    tile_requests = (([300, 200], [9, 9]), ([300, 200], [31, 17]), ([150, 130], [8, 5]))
    for (shape, ks), bd, md, K, lay in itertools.product(tile_requests, BOUNDARIES[1:], MODES, (1, 3), LAYOUTS):
        add(shape, ks, bd, md, K=K, layout=lay)
    for (shape, ks), (bd, md), v in itertools.product(tile_requests, (("linear-full", "convolution"), ("linear-same", "correlation"), ("linear-valid", "correlation")),
                                                     side_variants()):
        add(shape, ks, bd, md, **v)
    # their neighbours, which stay off the tiles: a domain of 16384 points, a kernel beyond 33 points on an axis, a circular request
    for bd, md, K in itertools.product(BOUNDARIES[1:], MODES, (1, 3)):
        add([120, 120], [9, 9], bd, md, K=K)
        add([300, 200], [34, 3], bd, md, K=K)
    for md, K in itertools.product(MODES, (1, 3)):
        add([256, 256], [9, 9], "circular", md, K=K)
    return cases


def c2c_corpus():
    cases = []
    shapes = [([256], [None]), ([64, 32], [None, [0], [1]]), ([16, 8, 4], [None, [0, 2], [1], [2]]), ([1009], [None]), ([1009, 8], [None, [0]]),
              ([1000, 6], [None, [1]]), ([65536], [None]), ([1 << 20], [None]), ([32768], [None]), ([1 << 17], [None])]
    for shape, axes_list in shapes:
        inside = {"shape": [max(1, n - 4) for n in shape], "offset": [2 if n > 4 else 0 for n in shape]}
        partly = {"shape": list(shape), "offset": [-3] * len(shape)}
        covers = {"shape": [n + 4 for n in shape], "offset": [-2] * len(shape)}
        outside = {"shape": [4] * len(shape), "offset": [n + 1 for n in shape]}
        sides = [("plain", {}), ("sin", dict(input_layout=strided(shape))), ("sout", dict(output_layout=strided(shape))),
                 ("sin+sout", dict(input_layout=strided(shape), output_layout=strided(shape, 3, 1, 9))),
                 ("lanes", dict(input_layout=strided(shape, 1, 2, 6), output_layout=strided(shape, 1, 0, 4))),
                 ("sin-nobs", dict(input_layout=strided(shape, batch_stride=False))),
                 ("zr", dict(zero_pad={"read": zrange(shape)})), ("zw", dict(zero_pad={"write": zrange(shape)})),
                 ("zr+zw", dict(zero_pad={"read": zrange(shape), "write": zrange(shape, 16, 8)})),
                 ("inplace", dict(in_place=True)), ("inplace zr", dict(in_place=True, zero_pad={"read": zrange(shape)})),
                 ("inplace zw", dict(in_place=True, zero_pad={"write": zrange(shape)})),
                 ("inplace zr+zw", dict(in_place=True, zero_pad={"read": zrange(shape), "write": zrange(shape, 16, 8)})),
                 ("zr sin", dict(zero_pad={"read": zrange(shape)}, input_layout=strided(shape))),
                 ("zw sout", dict(zero_pad={"write": zrange(shape)}, output_layout=strided(shape)))]
        for vn, v in (("inside", inside), ("partly", partly), ("covers", covers), ("outside", outside)):
            sides.append(("vin-" + vn, dict(io_view={"input": v})))
            sides.append(("vout-" + vn, dict(io_view={"output": v})))
            sides.append(("vout-clear-" + vn, dict(io_view={"output": dict(v, clearOutside=True)})))
        sides += [("vin+vout", dict(io_view={"input": partly, "output": dict(inside, clearOutside=True)})),
                  ("vin sin", dict(io_view={"input": partly}, input_layout=strided(partly["shape"]))),
                  ("vin sin-nobs", dict(io_view={"input": partly}, input_layout=strided(partly["shape"], batch_stride=False))),
                  ("vout sout", dict(io_view={"output": inside}, output_layout=strided(inside["shape"]))),
                  ("vout sout-nobs", dict(io_view={"output": inside}, output_layout=strided(inside["shape"], batch_stride=False))),
                  ("vin zr zw vout", dict(io_view={"input": inside, "output": partly}, zero_pad={"read": zrange(shape), "write": zrange(shape, 16, 8)})),
                  ("vout-clear sout", dict(io_view={"output": dict(inside, clearOutside=True)}, output_layout=strided(inside["shape"]))),   # invalid
                  ("inplace vin", dict(in_place=True, io_view={"input": inside})), ("inplace vout", dict(in_place=True, io_view={"output": inside})),
                  ("inplace sin", dict(in_place=True, input_layout=strided(shape)))]
        for axes, (sn, kw), direction in itertools.product(axes_list, sides, ("forward", "inverse")):
            if direction == "inverse" and sn not in ("plain", "sin+sout", "vin+vout", "zr+zw", "inplace zr"):
                continue
            name = "c2c %s axes=%s %s %s" % ("x".join(map(str, shape)), "-" if axes is None else "".join(map(str, axes)), sn, direction[:3])
            cases.append((name, _abi.make_desc("c2c", shape, batch=3, direction=direction, normalize="backward", axes=axes, **kw)))
    return cases


def real_sides_corpus():
    """r2c, c2r and a DCT through the shared side staging, f32 and f16-storage, fused single-launch and staged routes."""
    cases = []
    for typ, shape in itertools.product(("c2c", "r2c", "c2r", "dct2", "dst3"), ([1024], [8192], [1000], [100], [64, 32], [1 << 17], [30, 7])):
        direction = "inverse" if typ == "c2r" else "forward"
        pk = list(shape)
        if typ in ("r2c", "c2r"):
            pk[0] = shape[0] // 2 + 1
        ishape, oshape = (pk if typ == "c2r" else shape), (pk if typ == "r2c" else shape)
        vin = {"shape": list(ishape), "offset": [-1] * len(shape)}
        vout = {"shape": [max(1, n - 2) for n in oshape], "offset": [1 if n > 2 else 0 for n in oshape]}
        sides = [("plain", {}), ("vin", dict(io_view={"input": vin})), ("vout", dict(io_view={"output": vout})),
                 ("vout-clear", dict(io_view={"output": dict(vout, clearOutside=True)})), ("vin+vout", dict(io_view={"input": vin, "output": vout})),
                 ("zr", dict(zero_pad={"read": zrange(ishape)})), ("zw", dict(zero_pad={"write": zrange(oshape)})),
                 ("zr+zw vout", dict(zero_pad={"read": zrange(ishape), "write": zrange(oshape)}, io_view={"output": vout})),
                 ("inplace", dict(in_place=True)), ("inplace zr", dict(in_place=True, zero_pad={"read": zrange(ishape)})),
                 ("sin", dict(input_layout=strided(ishape))), ("sout", dict(output_layout=strided(oshape))),
                 ("vout-clear sout", dict(io_view={"output": dict(vout, clearOutside=True)}, output_layout=strided(vout["shape"]))),
                 ("vin sin", dict(io_view={"input": vin}, input_layout=strided(vin["shape"], batch_stride=False)))]
        for (sn, kw), prec in itertools.product(sides, ("f32", "f16-storage")):
            if prec == "f32" and typ == "c2c":
                continue   # c2c_corpus
            name = "%s %s %s %s" % (typ, "x".join(map(str, shape)), sn, prec)
            cases.append((name, _abi.make_desc(typ, shape, batch=3, direction=direction, normalize="backward", precision=prec, **kw)))
    return cases


def corpus():
    """(name, descriptor, environments) of every case."""
    seen, cases = set(), []
    for envs, group in ((ENVS + CONV_ENVS, conv_corpus(False) + conv_corpus(True)), (ENVS, c2c_corpus() + real_sides_corpus())):
        for name, desc in group:
            if name not in seen:      # the name spells out every parameter: a repeated name is a repeated case
                seen.add(name)
                cases.append((name, desc, envs))
    return cases


def plan_case(job):
    import emu_harness
    name, desc, envs, full = job
    lines = []
    for env in envs:
        for k in [k for k in os.environ if k.startswith("MI355FFT_") or k.startswith("MI355_EMU_") and k != "MI355_EMU_LIB"]:
            del os.environ[k]
        os.environ.update(EXTRA_ENV)
        os.environ.update(env)
        rc, text = emu_harness.plan_dump(desc)
        envs = ",".join("%s=%s" % (k[len("MI355FFT_"):], v) for k, v in env.items()) or "default"
        if rc:
            lines.append("%s | %s | %d | %s" % (name, envs, rc, text))
        elif full:
            lines.append("%s | %s | %d\n%s" % (name, envs, rc, text))
        else:
            lines.append("%s | %s | %d | %s" % (name, envs, rc, hashlib.sha1(text.encode()).hexdigest()))
    return lines


def snapshot(full, jobs):
    import emu_harness
    emu_harness.lib()      # built (if need be) once, before the workers start
    cases = corpus()
    with multiprocessing.Pool(jobs) as pool:
        chunks = pool.map(plan_case, [(n, d, e, full) for n, d, e in cases], chunksize=16)
    return len(cases), [line for chunk in chunks for line in chunk]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", "--output", help="file to write (default: standard output)")
    ap.add_argument("--full", action="store_true", help="write the IR dumps themselves instead of their hashes")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1), help="worker processes")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two snapshots; exit status 1 when they differ")
    ap.add_argument("--env", action="append", default=[], metavar="NAME=VALUE", help="a planner switch set in every environment")
    a = ap.parse_args()
    EXTRA_ENV.update(e.split("=", 1) for e in a.env)
    if a.compare:
        la, lb = (open(p).read().splitlines() for p in a.compare)
        diff = [(x, y) for x, y in itertools.zip_longest(la, lb) if x != y]
        plans = [x for x in la if " | " in x]      # (a --full snapshot carries the dumps between them)
        print("planner IR: %d cases, %d plans compared" % (len({x.split(" | ")[0] for x in plans}), len(plans)))
        print("identical" if not diff else "DIFFERENT: %d lines" % len(diff))
        for x, y in diff[:40]:
            print("-", x)
            print("+", y)
        return 1 if diff else 0
    n, lines = snapshot(a.full, a.jobs)
    out = open(a.output, "w") if a.output else sys.stdout
    out.write("\n".join(lines) + "\n")
    print("%d cases, %d plans (%d environments, %d more for fftconv)" % (n, len(lines), len(ENVS), len(CONV_ENVS)), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
