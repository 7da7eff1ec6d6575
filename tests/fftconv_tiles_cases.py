"""Shared by test_emu_fftconv_tiles.py and test_gpu_fftconv_tiles.py: one table of requests for the overlap-save tile route of rank-2 complex
fftconv (tiles-spectrum[N=PxP] tiles-conv-ols[N=PxP,L=L0xL1]: plan.cpp build_fftconv, kern_tiles.hpp fft_tiles_conv_ols_kernel) and the checks
both tiers run on it.

A case names the request and the tile edge P the switch forces (names without their prefix: the GPU tier sets MI355FFT_CONV_OLS2D, the
emulation tier MI355_EMU_CONV_OLS2D); P = None leaves the planner's own rule and `rule` is the P that rule names.  Geometry per axis a (axis 0
fastest): M_a = kernelShape[a], L_a = P - (M_a - 1) results a tile, nb_a = ceil((shape[a] + M_a - 1) / L_a) tiles.

Reference: numpy float64, np.fft.fft2 on the exact linear domain shape + kernelShape - 1, the conjugated kernel spectrum for a correlation,
zeroPad.read applied to the data and zeroPad.write to the logical result, cropped per boundary.  Bars (the project's own for complex
fftconv, exec_contract_cases.TOL_CONV): elementwise 4e-3 / 4e-3 and rel_l2 <= 1e-5 against that reference, and rel_l2 <= 1e-5 (the parity bar
of DESIGN.md section 3) against the same request planned with the switch at 0: the routes the planner had before this one.  Every case asserts
the exact route tag and 1 + K launches."""
import numpy as np

import exec_contract_cases as t
from test_emu_fftconv_real import _rel

SWITCH = "CONV_OLS2D"
TAG = "tiles-conv-ols["
FORBIDDEN = ("bluestein", "mixed", "columns", "fftconv[")


def options(shape, ks, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None):
    opts = {"type": "fftconv", "shape": list(shape), "batch": batch,
            "fftConv": {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": list(ks), "outputLayout": out_layout}}
    if zero_pad:
        opts["zeroPad"] = zero_pad
    return opts


def geometry(shape, ks, boundary):
    """per axis: (logical FFT length, output length, output offset on the logical domain)"""
    geo = []
    for n, kn in zip(shape, ks):
        fn = n + kn - 1
        geo.append({"linear-full": (fn, fn, 0), "linear-same": (fn, n, (kn - 1) // 2), "linear-valid": (fn, n - kn + 1, kn - 1)}[boundary])
    return geo


def _box(zr, dom):
    """a zeroPad range as a boolean mask over the domain (numpy order: axis 1, axis 0)"""
    keep = np.zeros((dom[1], dom[0]), bool)
    keep[max(0, zr["start"][1]):max(0, zr["end"][1]), max(0, zr["start"][0]):max(0, zr["end"][0])] = True
    return keep


def reference(shape, ks, batch, K, mode, boundary, zero_pad, x, h):
    """float64 reference [K][batch][os1][os0][2] of dense data x [batch][n1][n0] and kernels h [K][m1][m0] (interleaved f32, axis 0 fastest)"""
    (f0, o0, c0), (f1, o1, c1) = geometry(shape, ks, boundary)
    xc = np.asarray(x, np.float64).reshape(batch, shape[1], shape[0], 2)
    xc = xc[..., 0] + 1j * xc[..., 1]
    if zero_pad and zero_pad.get("read"):
        xc = np.where(_box(zero_pad["read"], shape), xc, 0)
    hc = np.asarray(h, np.float64).reshape(K, ks[1], ks[0], 2)
    hc = hc[..., 0] + 1j * hc[..., 1]
    X = np.fft.fft2(xc, s=(f1, f0))
    want = np.empty((K, batch, o1, o0, 2))
    for k in range(K):
        H = np.fft.fft2(hc[k], s=(f1, f0))
        y = np.fft.ifft2(X * (np.conj(H) if mode == "correlation" else H))
        if zero_pad and zero_pad.get("write"):
            y = np.where(_box(zero_pad["write"], (f0, f1)), y, 0)
        y = y[:, c1:c1 + o1, c0:c0 + o0]
        want[k, ..., 0], want[k, ..., 1] = y.real, y.imag
    return want


class TilesCase:
    def __init__(self, name, shape, ks, P, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None, rule=None):
        self.name, self.shape, self.ks, self.P, self.batch, self.K = name, tuple(shape), tuple(ks), P, batch, K
        self.mode, self.boundary, self.out_layout, self.zero_pad, self.rule = mode, boundary, out_layout, zero_pad, rule

    @property
    def tag(self):
        P = self.P or self.rule
        return f"{TAG}N={P}x{P},L={P - self.ks[0] + 1}x{P - self.ks[1] + 1}]"

    @property
    def opts(self):
        return options(self.shape, self.ks, self.batch, self.K, self.mode, self.boundary, self.out_layout, self.zero_pad)

    def __repr__(self):
        return self.name


MODES = ("convolution", "correlation")
BOUNDARIES = ("linear-full", "linear-same", "linear-valid")

CASES = [
    # L = 56 x 60 (55 x 60 for the even kernel) on the domain 158 x 104: 3 x 2 tiles an image, ragged last tiles on both axes, batch 3
    *[TilesCase(f"150x100_k{k0}x5_{mode[:4]}_{boundary[7:]}", (150, 100), (k0, 5), 64, 3, mode=mode, boundary=boundary)
      for k0 in (9, 8) for mode in MODES for boundary in BOUNDARIES],
    # L = 32 x 48: the crop of the correlation holds negative and positive lags on both axes
    TilesCase("100x70_k33x17_corr_same", (100, 70), (33, 17), 64, 2, mode="correlation"),
    TilesCase("90x80_k1x1_no_overlap", (90, 80), (1, 1), 64, 2),
    TilesCase("20x30_k9x9_single_tile", (20, 30), (9, 9), 64, 3, boundary="linear-full"),
    # the longest kernel a tile takes on one axis: L0 = 2
    TilesCase("70x200_k63x3_L2", (70, 200), (63, 3), 64, 1),
    # zeroPad boxes that cut tiles on both axes (L = 56 x 56 on the domain 138 x 98), three kernels, batch-major lanes
    TilesCase("130x90_k9x9_K3_zero_pad", (130, 90), (9, 9), 64, 2, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
              zero_pad={"read": {"start": [3, 5], "end": [120, 70]}, "write": {"start": [20, 10], "end": [130, 95]}}),
    # the 128-point tile: L = 96 x 112 on the domain 232 x 156, 3 x 2 tiles
    TilesCase("200x140_k33x17_P128", (200, 140), (33, 17), 128, 2),
    # the planner's own rule
    *[TilesCase(f"default_300x200_k31x17_{mode[:4]}", (300, 200), (31, 17), None, 1, K=2, mode=mode, rule=128) for mode in MODES],
    *[TilesCase(f"default_300x200_k9x9_{mode[:4]}", (300, 200), (9, 9), None, 1, K=2, mode=mode, rule=64) for mode in MODES],
]

_WANT = {}


def _rand(n, seed):
    """n complex elements, interleaved f32"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, 2 * n).astype(np.float32)


def data(case):
    """(x, h, float64 reference in the plan's output layout, flat) of a case, computed once per process and read-only"""
    if case.name not in _WANT:
        n, kn = case.shape[0] * case.shape[1], case.ks[0] * case.ks[1]
        x, h = _rand(n * case.batch, 0x71E0 + n + kn), _rand(kn * case.K, 0x71E1 + kn)
        want = reference(case.shape, case.ks, case.batch, case.K, case.mode, case.boundary, case.zero_pad, x, h)
        if case.out_layout != "kernel-major":
            want = want.transpose(1, 0, 2, 3, 4)
        want = np.ascontiguousarray(want).reshape(-1)
        for a in (x, h, want):
            a.setflags(write=False)
        _WANT[case.name] = (x, h, want)
    return _WANT[case.name]


def assert_route(case, route, launches):
    assert case.tag in route, (route, case.tag)
    assert launches == 1 + case.K, (route, launches)
    assert not any(f in route for f in FORBIDDEN), route


def check_case(run, setenv, oracle, case):
    """run(opts, x, out_floats, kernel) -> (got, route, launches) plans and runs under the environment; setenv(name, value) sets the tier's
    form of a planner switch"""
    from test_gpu_parity import check
    x, h, want = data(case)
    if case.P is not None:
        setenv(SWITCH, str(case.P))
    got, route, launches = run(case.opts, x, want.size, h)
    assert_route(case, route, launches)
    print(f"{route.strip()}: rel_l2={_rel(got, want):.3e}")
    check(oracle, got, want.astype(np.float32), f"{case.name} ({route.strip()})", *t.TOL_CONV[1:])
    assert _rel(got, want) <= 1e-5
    setenv(SWITCH, "0")
    ref, route0, _ = run(case.opts, x, want.size, h)
    assert TAG not in route0, route0
    rel = _rel(got, ref)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= 1e-5, (route, route0)


# ---- strided lanes on both sides: rank-2 strides, offsets and batch strides, kernel lanes kst apart ----------------------------------------
STRIDED = dict(shape=(150, 100), ks=(9, 5), batch=2, K=2, P=64, si=(2, 310), so=(3, 460), ioff=5, ooff=7, kst=1)


def strided_request():
    """(opts, physical input, kernels, float64 reference [K][batch][n1][n0][2], output floats, index arrays of the lanes in complex elements)"""
    s = STRIDED
    (n0, n1), ks, batch, K, si, so, ioff, ooff, kst = (s[k] for k in ("shape", "ks", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
    ibs, obs = n1 * si[1] + 11, n1 * so[1] + 7
    layout = {"interleavedComplex": True, "inputStrides": list(si), "outputStrides": list(so), "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    opts = options((n0, n1), ks, batch, K)
    opts["layout"] = layout
    opts["fftConv"]["outputKernelStrideElements"] = kst
    i1, i0 = np.meshgrid(np.arange(n1), np.arange(n0), indexing="ij")
    if "strided" not in _WANT:
        dense, h = _rand(n0 * n1 * batch, 0x71A1), _rand(ks[0] * ks[1] * K, 0x71A2)
        phys = _rand(ioff + (batch - 1) * ibs + (n1 - 1) * si[1] + (n0 - 1) * si[0] + 1, 0x71A3).reshape(-1, 2)
        for b in range(batch):
            phys[ioff + b * ibs + i1 * si[1] + i0 * si[0]] = dense.reshape(batch, n1, n0, 2)[b]
        want = reference((n0, n1), ks, batch, K, "convolution", "linear-same", None, dense, h)
        phys = phys.reshape(-1)
        for a in (phys, h, want):
            a.setflags(write=False)
        _WANT["strided"] = (phys, h, want)
    phys, h, want = _WANT["strided"]
    out_elems = ooff + (K - 1) * kst + (batch - 1) * obs + (n1 - 1) * so[1] + (n0 - 1) * so[0] + 1
    lanes = {(k, b): ooff + k * kst + b * obs + i1 * so[1] + i0 * so[0] for k in range(K) for b in range(batch)}
    return opts, phys, h, want, 2 * out_elems, lanes


def strided_tag():
    s = STRIDED
    return f"{TAG}N={s['P']}x{s['P']},L={s['P'] - s['ks'][0] + 1}x{s['P'] - s['ks'][1] + 1}]"


def check_strided(run, setenv, oracle):
    """run(opts, x, out_floats, kernel, out_init) as above; the output starts as 777.0 everywhere and every element outside the lanes keeps it"""
    from test_emu_fftconv import _close
    opts, phys, h, want, out_floats, lanes = strided_request()
    K = STRIDED["K"]
    setenv(SWITCH, str(STRIDED["P"]))
    sentinel = np.full(out_floats, 777.0, np.float32)
    got, route, launches = run(opts, phys, out_floats, h, sentinel)
    assert strided_tag() in route and launches == 1 + K, (route, launches)
    setenv(SWITCH, "0")
    ref, route0, _ = run(opts, phys, out_floats, h, sentinel)
    assert TAG not in route0, route0
    got2, ref2 = np.asarray(got).reshape(-1, 2), np.asarray(ref).reshape(-1, 2)
    touched = np.zeros(out_floats // 2, bool)
    for (k, b), idx in lanes.items():
        assert not touched[idx].any(), "the lanes of the request overlap"
        touched[idx] = True
        _close(got2[idx].reshape(-1), want[k, b].astype(np.float32).reshape(-1), 4e-3, 4e-3, f"{route.strip()} kernel {k} image {b}")
        assert _rel(got2[idx], want[k, b]) <= 1e-5
    assert np.all(got2[~touched] == 777.0), "stores outside the output lanes"
    rel = _rel(got2[touched], ref2[touched])
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= 1e-5, (route, route0)


def strided_contract_oracle(oracle, o):
    """exec_contract_cases oracle of the strided request: NaN where the plan's contract leaves the output alone"""
    _, phys, h, want, out_floats, lanes = strided_request()
    full = np.full((out_floats // 2, 2), np.nan)
    for (k, b), idx in lanes.items():
        full[idx] = want[k, b]
    return phys, h, full.reshape(-1)


def _dense_oracle(seed):
    """a dense rank-2 linear request against reference(), in the plan's output layout"""
    def f(oracle, o):
        fc, shape, batch = o["fftConv"], o["shape"], o["batch"]
        ks, K = fc["kernelShape"], fc["kernelCount"]
        x, h = _rand(shape[0] * shape[1] * batch, seed), _rand(ks[0] * ks[1] * K, seed + 1)
        want = reference(shape, ks, batch, K, fc["mode"], fc["boundary"], o.get("zeroPad"), x, h)
        if fc["outputLayout"] != "kernel-major":
            want = want.transpose(1, 0, 2, 3, 4)
        return x, h, np.ascontiguousarray(want).reshape(-1)
    return f


# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("tiles_dense_150x100_k9x5", t._fc([150, 100], 3, [9, 5], 1, boundary="linear-same"), "tiles-conv-ols[N=64x64,L=56x60]", _dense_oracle(0x71C0), t.TOL_CONV,
           env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("tiles_strided_150x100_k9x5", strided_request()[0], strided_tag(), strided_contract_oracle, t.TOL_CONV,
           env={SWITCH: "64"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure sizes fftconv domains of any rank) ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("tiles_default_300x200_k31x17", t._fc([300, 200], 1, [31, 17], 2, boundary="linear-same"), TAG + "N=", _dense_oracle(0x71D0), t.TOL_CONV, starts=False),
]


# ---- direct sums in float64 (the capability test: windows of a request whose float64 FFT reference is not worth its time) ----
def direct_same_conv(x, h, shape, ks, lo, hi):
    """outputs [lo0, hi0) x [lo1, hi1) of the linear-same convolution of one image: complex128 [hi1 - lo1][hi0 - lo0]"""
    (n0, n1), (m0, m1) = shape, ks
    xc = np.asarray(x, np.float64).reshape(n1, n0, 2)
    xc = xc[..., 0] + 1j * xc[..., 1]
    hc = np.asarray(h, np.float64).reshape(m1, m0, 2)
    hc = hc[..., 0] + 1j * hc[..., 1]
    c0, c1 = (m0 - 1) // 2, (m1 - 1) // 2
    out = np.zeros((hi[1] - lo[1], hi[0] - lo[0]), complex)
    for r1 in range(m1):
        for r0 in range(m0):           # y[o] = sum_r h[r] x[o + c - r]
            a1, a0 = np.arange(lo[1], hi[1]) + c1 - r1, np.arange(lo[0], hi[0]) + c0 - r0
            ok1, ok0 = (a1 >= 0) & (a1 < n1), (a0 >= 0) & (a0 < n0)
            blk = np.zeros_like(out)
            blk[np.ix_(ok1, ok0)] = xc[np.ix_(a1[ok1], a0[ok0])]
            out += hc[r1, r0] * blk
    return out
