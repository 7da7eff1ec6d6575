"""The tables of test_emu_fftconv_sum.py and test_gpu_fftconv_sum.py: fftConv.inputChannels = C, the sum over input channels
    y[b][k] = sum_c x[b][c] (*) h[k][c]
on its two kinds of route: the sum form of the rank-2 overlap-save tile kernel (tiles-spectrum[N=PxP] tiles-conv-ols-sum[N=PxP,L=L0xL1,C=c] and
its real twin: plan.cpp emit_tiles_ols, kern_tiles.hpp fft_tiles_conv_ols_sum_kernel; switch SUM_OLS2D) and the composed routes
fftconv-sum[K=k,C=c] / rconv-sum[K=k,C=c] (the reduction in the pointwise pass: kern_generic.hpp pointwise_sum_kernel).

Layout of a request: the input holds batch * C lines, line b * C + c being channel c of item b (dense [batch][C][shape]); the kernel buffer holds
kernelCount * C kernels, kernel (k, c) at k * C + c; the output side is that of C = 1.

References are numpy float64 on the exact domain, summed over c: per channel the scaffold's Route.reference (real data of any rank, complex images:
reference2d) or, for complex lines and volumes, the same statement with np.fft.fftn; zeroPad.read applies to every channel and zeroPad.write to the sum (a mask,
so applying it per channel before adding is the same thing).

Bars (the project's own for fftconv): elementwise 4e-3 / 4e-3, rel_l2 <= 1e-5 against float64, and rel_l2 <= 1e-5 against what a caller could do
before the option existed: the C single-channel plans' outputs on the same data (each channel its own request on the default routes), added in
float32 on the host in channel order.  Random data is uniform on [-1, 1]; error and signal both grow like sqrt(C), so the relative bars do not move
with C.

Every case asserts its route tag and that the route names no single-channel product (`fftconv[`, `rconv[`); a tile-route case also asserts 1 + K
launches and that the route names no Bluestein, mixed-radix or column launch.  A composed case on a domain that is no power of two is made of exactly
those launches (they are its transforms), so that part of the list cannot apply to it."""
import numpy as np

import exec_contract_cases as t
import fftconv_linear_cases as lin
import fftconv_ols_scaffold as s
import fftconv_rtiles_cases as rtiles
import fftconv_tiles_cases as tiles
from fftconv_ols_scaffold import BOUNDARIES, MODES
from test_emu_fftconv_real import _opts as real_opts, _rel

SWITCH = "SUM_OLS2D"
FORBIDDEN_TILES = ("bluestein", "mixed", "columns", "fftconv[", "rconv[")
FORBIDDEN_COMPOSED = ("fftconv[", "rconv[")
F64_BAR = PARITY_BAR = 1e-5
ATOL = RTOL = 4e-3
SEED = 0x5C00
UNSUPPORTED_ODD = "Unsupported: fftConv.inputChannels > 1 on real circular fftconv with odd shape[0]"


def tile_tag(real, P, ks, C):
    r = "r" if real else ""
    return f"tiles-{r}spectrum[N={P}x{P}] tiles-{r}conv-ols-sum[N={P}x{P},L={P - ks[0] + 1}x{P - ks[1] + 1},C={C}]"


def composed_tag(real, K, C):
    return f"{'rconv' if real else 'fftconv'}-sum[K={K},C={C}]"


class Case:
    """P: the tile the switch forces ("0": the composed route), None: the planner's own rule; tile: the tile the route tag must name (None: composed)"""
    def __init__(self, name, real, shape, ks, batch, C, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None, P=None, tile=None,
                 kernel_list=False, before=True):
        self.name, self.real, self.shape, self.ks, self.batch, self.C, self.K = name, real, tuple(shape), tuple(ks), batch, C, K
        self.mode, self.boundary, self.out_layout, self.zero_pad, self.P, self.tile = mode, boundary, out_layout, zero_pad, P, tile
        self.kernel_list, self.before = kernel_list, before

    @property
    def tag(self):
        return tile_tag(self.real, self.tile, self.ks, self.C) if self.tile else composed_tag(self.real, self.K, self.C)

    @property
    def opts(self):
        return options(self.real, self.shape, self.ks, self.batch, self.C, self.K, self.mode, self.boundary, self.out_layout, self.zero_pad)

    def __repr__(self):
        return self.name


def options(real, shape, ks, batch, C, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None):
    if real:
        o = real_opts(list(shape), list(ks), batch, K=K, mode=mode, boundary=boundary, out_layout=out_layout, zero_pad=zero_pad)
    else:
        o = s.options(shape, ks, batch, K, mode, boundary, out_layout, zero_pad)
    if C is not None:
        o["fftConv"]["inputChannels"] = C
    return o


def _route(real):
    return rtiles.ROUTE if real else tiles.ROUTE


def _complex_nd(shape, ks, batch, K, mode, boundary, x, h):
    """Route.reference for complex data of any rank (no zeroPad): [K][batch][out...][2], numpy order"""
    geo = [lin.geometry((n, kn, boundary)) for n, kn in zip(shape, ks)]
    fs = tuple(g[0] for g in geo)[::-1]
    crop = tuple(slice(g[2], g[2] + g[1]) for g in geo)[::-1]
    axes = tuple(range(1, len(shape) + 1))
    xc = np.asarray(x, np.float64).reshape((batch,) + tuple(shape)[::-1] + (2,))
    hc = np.asarray(h, np.float64).reshape((K,) + tuple(ks)[::-1] + (2,))
    X = np.fft.fftn(xc[..., 0] + 1j * xc[..., 1], s=fs, axes=axes)
    H = np.fft.fftn(hc[..., 0] + 1j * hc[..., 1], s=fs, axes=axes)
    want = []
    for k in range(K):
        y = np.fft.ifftn(X * (np.conj(H[k]) if mode == "correlation" else H[k]), axes=axes)[(slice(None),) + crop]
        want.append(np.stack([y.real, y.imag], -1))
    return np.stack(want)


def channel(a, outer, C, c):
    """channel c of the flat float array a = [outer][C][per]: [outer][per], contiguous"""
    return np.ascontiguousarray(np.asarray(a).reshape(outer, C, -1)[:, c]).reshape(-1)


def reference(real, shape, ks, batch, C, K, mode, boundary, zero_pad, x, h):
    """float64, kernel-major [K][batch][out] flat per result (complex data interleaved): the per-channel references, added"""
    total = None
    for c in range(C):
        xc, hc = channel(x, batch, C, c), channel(h, K, C, c)
        if not real and len(shape) != 2:
            w = _complex_nd(shape, ks, batch, K, mode, boundary, xc, hc)
        else:
            w = _route(real).reference(shape, ks, batch, K, mode, boundary, zero_pad, xc, hc)
        w = np.asarray(w, np.float64).reshape(K, batch, -1)
        total = w if total is None else total + w
    return total


def in_layout(want, out_layout):
    return np.ascontiguousarray(want if out_layout == "kernel-major" else want.transpose(1, 0, 2)).reshape(-1)


_DATA = {}


def data(case):
    """(x, h, float64 reference flat in the plan's output layout) of a case, computed once per process and read-only"""
    if case.name not in _DATA:
        rand = _route(case.real).rand
        n, kn = int(np.prod(case.shape)), int(np.prod(case.ks))
        x, h = rand(n * case.batch * case.C, SEED + n + kn), rand(kn * case.K * case.C, SEED + 1 + kn)
        want = in_layout(reference(case.real, case.shape, case.ks, case.batch, case.C, case.K, case.mode, case.boundary, case.zero_pad, x, h), case.out_layout)
        for a in (x, h, want):
            a.setflags(write=False)
        _DATA[case.name] = (x, h, want)
    return _DATA[case.name]


def single_channel_sum(run, case, x, h, out_floats):
    """what a caller could do before the option: C single-channel plans on the default routes, their float32 outputs added on the host in channel order"""
    o1 = options(case.real, case.shape, case.ks, case.batch, None, case.K, case.mode, case.boundary, case.out_layout, case.zero_pad)
    acc = None
    for c in range(case.C):
        got = np.asarray(run(o1, channel(x, case.batch, case.C, c), out_floats, channel(h, case.K, case.C, c))[0], np.float32)
        acc = got.copy() if acc is None else acc + got
    return acc


def assert_route(case, route, launches):
    assert case.tag in route, (route, case.tag)
    forbidden = FORBIDDEN_TILES if case.tile else FORBIDDEN_COMPOSED
    assert not any(f in route for f in forbidden), route
    if case.tile:
        assert launches == 1 + case.K, (route, launches)


def check_case(run, setenv, oracle, case):
    """run(opts, x, out_floats, kernel, out_init=None) -> (got, route, launches) and setenv(name, value): fftconv_ols_scaffold's two runners"""
    x, h, want = data(case)
    kn = int(np.prod(case.ks)) * (1 if case.real else 2)
    kernel = [h[i * kn:(i + 1) * kn] for i in range(case.K * case.C)] if case.kernel_list else h
    if case.P is not None:
        setenv(SWITCH, str(case.P))
    got, route, launches = run(case.opts, x, want.size, kernel)
    assert_route(case, route, launches)
    got = np.asarray(got).reshape(-1)
    rel = _rel(got, want)
    print(f"{case.name} {route.strip()}: rel_l2={rel:.3e} against float64")
    oracle.assert_close_elementwise(got, want.astype(np.float32), ATOL, RTOL, f"{case.name} ({route.strip()})")
    assert rel <= F64_BAR, (route, rel)
    if case.before:
        setenv(SWITCH, "1")
        before = single_channel_sum(run, case, x, h, want.size)
        rel = _rel(got, before)
        print(f"{case.name} {route.strip()}: rel_l2={rel:.3e} against the sum of {case.C} single-channel plans")
        assert rel <= PARITY_BAR, (route, rel)
    return got


def _tile_cases(real, shape):
    """both modes x the three linear boundaries on the 64-point tile, batch 2, C = 3, K = 2"""
    return [Case(f"{'real' if real else 'complex'}_{shape[0]}x{shape[1]}_k9x5_{mode[:4]}_{boundary[7:]}", real, shape, (9, 5), 2, 3, K=2, mode=mode, boundary=boundary, P=64, tile=64)
            for mode in MODES for boundary in BOUNDARIES]


ZERO_PAD = {"read": {"start": [3, 5], "end": [120, 70]}, "write": {"start": [20, 10], "end": [130, 95]}}      # the boxes of the tile tables' zeroPad case

TILE_CASES = [
    # 1: L = 56 x 60 on the domain 158 x 104: 3 x 2 ragged tiles an image, batch 2, C = 3, K = 2, complex and real
    *_tile_cases(False, (150, 100)), *_tile_cases(True, (150, 100)),
    # 2: the domain 158 x 134: nb_1 = 3, the last pair of every row has no partner, in every channel
    *[Case(f"real_150x130_k9x5_{mode[:4]}_absent_partner", True, (150, 130), (9, 5), 2, 3, K=2, mode=mode, P=64, tile=64) for mode in MODES],
    # 4: one tile, many channels: the channel index in the input line and in the spectrum offset
    *[Case(f"{'real' if real else 'complex'}_20x30_k9x9_C17_single_tile", real, (20, 30), (9, 9), 3, 17, boundary="linear-full", P=64, tile=64) for real in (False, True)],
    # 5: zeroPad boxes that cut tiles on both axes (read: every channel; write: the sum), three kernels, correlation, batch-major lanes
    *[Case(f"{'real' if real else 'complex'}_130x90_k9x9_K3_zero_pad", real, (130, 90), (9, 9), 2, 2, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
           zero_pad=ZERO_PAD, P=64, tile=64) for real in (False, True)],
    # 8: the planner's own rule, no switch
    *[Case(f"{'real' if real else 'complex'}_default_300x200_k9x9_C4", real, (300, 200), (9, 9), 1, 4, K=2, tile=64, kernel_list=not real) for real in (False, True)],
]

COMPOSED_CASES = [
    # 7: kernels of 18 .. 33 points have no sum instance (a P = 128 one does not fit in registers): the composed routes, whatever the switch forces
    *[Case(f"{'real' if real else 'complex'}_200x140_k33x17_composed", real, (200, 140), (33, 17), 1, 2, P=128) for real in (False, True)],
    # 10: rank 1, rank 2 circular, rank 3
    *[Case(f"{'real' if real else 'complex'}_1000_k31_same", real, (1000,), (31,), 2, 3, K=2) for real in (False, True)],
    *[Case(f"{'real' if real else 'complex'}_64x48_k5x5_circular", real, (64, 48), (5, 5), 2, 3, boundary="circular") for real in (False, True)],
    *[Case(f"{'real' if real else 'complex'}_20x12x10_k3x3x3", real, (20, 12, 10), (3, 3, 3), 2, 2) for real in (False, True)],
    # 10 (last line): the switch at 0 on the requests of case 1
    *[Case(f"{'real' if real else 'complex'}_150x100_k9x5_switch_0", real, (150, 100), (9, 5), 2, 3, K=2, P=0) for real in (False, True)],
]

# 3: C = 1 is the request without the option: (real, shape, ks, batch, K, boundary, switches)
C1_CASES = [
    (False, (150, 100), (9, 5), 2, 2, "linear-same", {"CONV_OLS2D": "64"}),
    (True, (150, 130), (9, 5), 2, 2, "linear-same", {"RCONV_OLS2D": "64"}),
    (False, (1000,), (31,), 3, 2, "linear-same", {}),
    (True, (1000,), (31,), 3, 2, "linear-same", {}),
    (False, (64, 48), (5, 5), 2, 1, "circular", {}),
]


# ---- 6: strided lanes on both sides: the scaffold's STRIDED geometry with C = 2; the input batch stride is the step between consecutive LINES ----
STRIDED_C = 2


def strided_request(real):
    """(opts, physical input, kernels, float64 reference [K][batch][out], output floats, index arrays of the output lanes in elements)"""
    g = _route(real).strided
    shape, ks, batch, K, si, so, ioff, ooff, kst = (g[k] for k in ("shape", "ks", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
    C = STRIDED_C
    ibs, obs = shape[-1] * si[-1] + 11, shape[-1] * so[-1] + 7
    layout = {"inputStrides": list(si), "outputStrides": list(so), "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    if real:
        opts = real_opts(list(shape), list(ks), batch, K=K, boundary="linear-same", layout=layout, outputKernelStrideElements=kst, inputChannels=C)
    else:
        opts = s.options(shape, ks, batch, K)
        opts["layout"] = dict(layout, interleavedComplex=True)
        opts["fftConv"].update(outputKernelStrideElements=kst, inputChannels=C)
    index = np.meshgrid(*(np.arange(n) for n in shape[::-1]), indexing="ij")[::-1]
    ipos, opos = sum(i * st for i, st in zip(index, si)), sum(i * st for i, st in zip(index, so))
    width = () if real else (2,)
    key = ("strided", real)
    if key not in _DATA:
        rand = _route(real).rand
        n, kn = int(np.prod(shape)), int(np.prod(ks))
        dense, h = rand(n * batch * C, SEED + 0xA1), rand(kn * K * C, SEED + 0xA2)
        phys = rand(ioff + (batch * C - 1) * ibs + int(ipos.max()) + 1, SEED + 0xA3).reshape((-1,) + width)
        for line in range(batch * C):
            phys[ioff + line * ibs + ipos] = dense.reshape((batch * C,) + shape[::-1] + width)[line]
        want = reference(real, shape, ks, batch, C, K, "convolution", "linear-same", None, dense, h).reshape((K, batch) + shape[::-1] + width)
        phys = phys.reshape(-1)
        for a in (phys, h, want):
            a.setflags(write=False)
        _DATA[key] = (phys, h, want)
    phys, h, want = _DATA[key]
    out_elems = ooff + (K - 1) * kst + (batch - 1) * obs + int(opos.max()) + 1
    lanes = {(k, b): ooff + k * kst + b * obs + opos for k in range(K) for b in range(batch)}
    return opts, phys, h, want, out_elems * (1 if real else 2), lanes


def strided_tag(real):
    g = _route(real).strided
    return tile_tag(real, g["P"], g["ks"], STRIDED_C)


def check_strided(run, setenv, oracle, real):
    """the output starts as 777.0 everywhere and every element outside the lanes keeps it"""
    opts, phys, h, want, out_floats, lanes = strided_request(real)
    K = _route(real).strided["K"]
    setenv(SWITCH, "64")
    sentinel = np.full(out_floats, 777.0, np.float32)
    got, route, launches = run(opts, phys, out_floats, h, sentinel)
    assert strided_tag(real) in route and launches == 1 + K, (route, launches)
    got = np.asarray(got) if real else np.asarray(got).reshape(-1, 2)
    touched = np.zeros(len(got), bool)
    for (k, b), idx in lanes.items():
        assert not touched[idx].any(), "the lanes of the request overlap"
        touched[idx] = True
        oracle.assert_close_elementwise(got[idx].reshape(-1), want[k, b].astype(np.float32).reshape(-1), ATOL, RTOL, f"{route.strip()} kernel {k} image {b}")
        assert _rel(got[idx], want[k, b]) <= F64_BAR
    assert np.all(got[~touched] == 777.0), "stores outside the output lanes"


def strided_contract_oracle(real):
    """exec_contract_cases oracle of the strided request: NaN where the plan's contract leaves the output alone"""
    def f(oracle, o):
        _, phys, h, want, out_floats, lanes = strided_request(real)
        full = np.full(out_floats, np.nan)
        full = full if real else full.reshape(-1, 2)
        for (k, b), idx in lanes.items():
            full[idx] = want[k, b]
        return phys, h, full.reshape(-1)
    return f


def dense_oracle(real, seed):
    """exec_contract_cases oracle of a dense request against the float64 reference, in the plan's output layout"""
    def f(oracle, o):
        fc, shape, batch = o["fftConv"], o["shape"], o["batch"]
        ks, K, C = fc["kernelShape"], fc["kernelCount"], fc["inputChannels"]
        rand = _route(real).rand
        x, h = rand(int(np.prod(shape)) * batch * C, seed), rand(int(np.prod(ks)) * K * C, seed + 1)
        return x, h, in_layout(reference(real, tuple(shape), tuple(ks), batch, C, K, fc["mode"], fc["boundary"], o.get("zeroPad"), x, h), fc["outputLayout"])
    return f


# ---- 11: exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("sum_tiles_dense_150x100_k9x5_C3", options(False, (150, 100), (9, 5), 2, 3, K=2), tile_tag(False, 64, (9, 5), 3), dense_oracle(False, SEED + 0xC0), t.TOL_CONV,
           env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("sum_rtiles_dense_150x130_k9x5_C3", options(True, (150, 130), (9, 5), 2, 3, K=2), tile_tag(True, 64, (9, 5), 3), dense_oracle(True, SEED + 0xC2), t.TOL_RCONV,
           env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("sum_tiles_strided_150x100_k9x5_C2", strided_request(False)[0], strided_tag(False), strided_contract_oracle(False), t.TOL_CONV,
           env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("sum_composed_1000_k31_C3", options(False, (1000,), (31,), 2, 3, K=2), composed_tag(False, 2, 3), dense_oracle(False, SEED + 0xC4), t.TOL_CONV,
           starts=False, replay=True),
]
