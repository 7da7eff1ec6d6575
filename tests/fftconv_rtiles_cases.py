"""Shared by test_emu_fftconv_rtiles.py and test_gpu_fftconv_rtiles.py: one table of requests for the overlap-save tile route of rank-2 REAL
fftconv (tiles-rspectrum[N=PxP] tiles-rconv-ols[N=PxP,L=L0xL1]: plan.cpp build_fftconv_real, kern_tiles.hpp fft_tiles_conv_ols_kernel on an
RTileCfg) and the checks both tiers run on it.

A case names the request and the tile edge P the switch forces (names without their prefix: the GPU tier sets MI355FFT_RCONV_OLS2D, the
emulation tier MI355_EMU_RCONV_OLS2D); P = None leaves the planner's own rule and `rule` is the P that rule names.  Geometry per axis a (axis 0
fastest): M_a = kernelShape[a], L_a = P - (M_a - 1) results a tile, nb_a = ceil((shape[a] + M_a - 1) / L_a) tiles.  A work item of the kernel is
a pair of tiles that are neighbours on axis 1 (one in the real, one in the imaginary parts of a complex tile): with odd nb_1 the last pair of
every row has no second tile.

Reference: numpy float64 on the exact linear domain shape + kernelShape - 1 (test_emu_fftconv_real._want: fft2 of data and kernels, the
conjugated kernel spectrum for a correlation, zeroPad.read applied to the data and zeroPad.write to the logical result, cropped per boundary).
Bars (the project's own for real fftconv and for the tile table): elementwise 4e-3 / 4e-3 and rel_l2 <= 1e-5 against that reference (_check),
rel_l2 <= 1e-5 against the same request planned with the switch at 0 (the routes the planner had before this one), and rel_l2 <= 1e-5 against
the real parts of the complex plan on the same data with zero imaginary parts.  Every case asserts the exact route tag, 1 + K launches and
that the route names no Bluestein, mixed-radix, column or rconv[K] launch."""
import numpy as np

import exec_contract_cases as t
from test_emu_fftconv_real import _check, _opts, _rand, _rel, _want

SWITCH = "RCONV_OLS2D"
COMPLEX_SWITCH = "CONV_OLS2D"
TAG = "tiles-rconv-ols["
FORBIDDEN = ("bluestein", "mixed", "columns", "rconv[")
UNSUPPORTED = "Unsupported: strided layouts on real fftconv outside the one-launch line route"


def tag_of(P, ks):
    return f"{TAG}N={P}x{P},L={P - ks[0] + 1}x{P - ks[1] + 1}]"


class RTilesCase:
    def __init__(self, name, shape, ks, P, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None, rule=None):
        self.name, self.shape, self.ks, self.P, self.batch, self.K = name, tuple(shape), tuple(ks), P, batch, K
        self.mode, self.boundary, self.out_layout, self.zero_pad, self.rule = mode, boundary, out_layout, zero_pad, rule

    @property
    def tag(self):
        return tag_of(self.P or self.rule, self.ks)

    @property
    def opts(self):
        return _opts(self.shape, self.ks, self.batch, K=self.K, mode=self.mode, boundary=self.boundary, out_layout=self.out_layout, zero_pad=self.zero_pad)

    def __repr__(self):
        return self.name


MODES = ("convolution", "correlation")
BOUNDARIES = ("linear-full", "linear-same", "linear-valid")

CASES = [
    # L = 56 x 60 (55 x 60 for the even kernel) on the domain 158 x 134: 3 x 3 tiles an image, so two pair rows of which the second has no partner;
    # ragged last tiles on both axes, batch 3
    *[RTilesCase(f"150x130_k{k0}x5_{mode[:4]}_{boundary[7:]}", (150, 130), (k0, 5), 64, 3, mode=mode, boundary=boundary)
      for k0 in (9, 8) for mode in MODES for boundary in BOUNDARIES],
    # the domain 158 x 104: nb_1 = 2, every partner is there
    RTilesCase("150x100_k9x5_both_partners", (150, 100), (9, 5), 64, 2),
    # L = 32 x 48: the crop of the correlation holds negative and positive lags on both axes, for both partners
    RTilesCase("100x70_k33x17_corr_same", (100, 70), (33, 17), 64, 2, mode="correlation"),
    RTilesCase("90x80_k1x1_no_overlap", (90, 80), (1, 1), 64, 2),
    # one tile: the partner is absent everywhere
    RTilesCase("20x30_k9x9_single_tile", (20, 30), (9, 9), 64, 3, boundary="linear-full"),
    # the longest kernel a tile takes on one axis: L0 = 2
    RTilesCase("70x200_k63x3_L2", (70, 200), (63, 3), 64, 1),
    # zeroPad boxes that cut tiles and pairs on both axes (L = 56 x 56 on the domain 138 x 98), three kernels, batch-major lanes
    RTilesCase("130x90_k9x9_K3_zero_pad", (130, 90), (9, 9), 64, 2, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
               zero_pad={"read": {"start": [3, 5], "end": [120, 70]}, "write": {"start": [20, 10], "end": [130, 95]}}),
    # the 128-point tile: L = 96 x 112 on the domain 232 x 156, 3 x 2 tiles
    RTilesCase("200x140_k33x17_P128", (200, 140), (33, 17), 128, 2),
    # the planner's own rule
    *[RTilesCase(f"default_300x200_k31x17_{mode[:4]}", (300, 200), (31, 17), None, 1, K=2, mode=mode, rule=128) for mode in MODES],
    *[RTilesCase(f"default_300x200_k9x9_{mode[:4]}", (300, 200), (9, 9), None, 1, K=2, mode=mode, rule=64) for mode in MODES],
]

_WANT = {}


def data(case):
    """(x, h, float64 reference [K][batch][os1][os0]) of a case, computed once per process and read-only"""
    if case.name not in _WANT:
        n, kn = case.shape[0] * case.shape[1], case.ks[0] * case.ks[1]
        x, h = _rand(n * case.batch, 0x7E10 + n + kn), _rand(kn * case.K, 0x7E11 + kn)
        want = _want(x, h, list(case.shape), list(case.ks), case.batch, case.K, case.mode, case.boundary, case.zero_pad)
        for a in (x, h, want):
            a.setflags(write=False)
        _WANT[case.name] = (x, h, want)
    return _WANT[case.name]


def assert_route(case, route, launches):
    assert case.tag in route, (route, case.tag)
    assert launches == 1 + case.K, (route, launches)
    assert not any(f in route for f in FORBIDDEN), route


def widened(opts, x, h):
    """the complex request on the same data with zero imaginary parts: (opts, interleaved data, interleaved kernels)"""
    o = dict(opts, layout={"interleavedComplex": True})
    xc = np.zeros(2 * x.size, np.float32)
    xc[0::2] = x
    hc = np.zeros(2 * h.size, np.float32)
    hc[0::2] = h
    return o, xc, hc


def check_case(run, setenv, oracle, case):
    """run(opts, x, out_floats, kernel) -> (got, route, launches) plans and runs under the environment; setenv(name, value) sets the tier's
    form of a planner switch"""
    x, h, want = data(case)
    if case.P is not None:
        setenv(SWITCH, str(case.P))
    got, route, launches = run(case.opts, x, want.size, h)
    assert_route(case, route, launches)
    _check(oracle, got, want, case.batch, case.K, case.out_layout, route)
    assert _rel(np.asarray(got).reshape(-1), _in_layout(want, case)) <= 1e-5
    # the complex plan (its own tile route where the case forces one) on the same data with zero imaginary parts: what a user could do before
    if case.P is not None:
        setenv(COMPLEX_SWITCH, str(case.P))
    oc, xc, hc = widened(case.opts, x, h)
    cgot, croute, _ = run(oc, xc, 2 * want.size, hc)
    rel = _rel(got, np.asarray(cgot)[0::2])
    print(f"{route.strip()} vs complex {croute.strip()}: rel_l2={rel:.3e}")
    assert rel <= 1e-5, (route, croute)
    setenv(SWITCH, "0")
    ref, route0, _ = run(case.opts, x, want.size, h)
    assert TAG not in route0 and "rconv[K=" in route0, route0
    rel = _rel(got, ref)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= 1e-5, (route, route0)


def _in_layout(want, case):
    w = want.reshape(case.K, case.batch, -1)
    if case.out_layout != "kernel-major":
        w = w.transpose(1, 0, 2)
    return np.ascontiguousarray(w).reshape(-1)


# ---- strided lanes on both sides: rank-2 strides, offsets and batch strides in f32 elements, kernel lanes kst apart; odd strides and offsets,
# ---- so that no element is 8-byte aligned by construction.  nb = 3 x 3 tiles: the second pair row has no partner ----------------------------
STRIDED = dict(shape=(150, 130), ks=(9, 5), batch=2, K=2, P=64, si=(3, 455), so=(5, 761), ioff=5, ooff=7, kst=1)


def strided_request():
    """(opts, physical input, kernels, float64 reference [K][batch][n1][n0], output floats, index arrays of the lanes in f32 elements)"""
    s = STRIDED
    (n0, n1), ks, batch, K, si, so, ioff, ooff, kst = (s[k] for k in ("shape", "ks", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
    ibs, obs = n1 * si[1] + 11, n1 * so[1] + 7
    layout = {"inputStrides": list(si), "outputStrides": list(so), "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    opts = _opts([n0, n1], list(ks), batch, K=K, boundary="linear-same", layout=layout, outputKernelStrideElements=kst)
    i1, i0 = np.meshgrid(np.arange(n1), np.arange(n0), indexing="ij")
    if "strided" not in _WANT:
        dense, h = _rand(n0 * n1 * batch, 0x7EA1), _rand(ks[0] * ks[1] * K, 0x7EA2)
        phys = _rand(ioff + (batch - 1) * ibs + (n1 - 1) * si[1] + (n0 - 1) * si[0] + 1, 0x7EA3)
        for b in range(batch):
            phys[ioff + b * ibs + i1 * si[1] + i0 * si[0]] = dense.reshape(batch, n1, n0)[b]
        want = _want(dense, h, [n0, n1], list(ks), batch, K, "convolution", "linear-same")
        for a in (phys, h, want):
            a.setflags(write=False)
        _WANT["strided"] = (phys, h, want)
    phys, h, want = _WANT["strided"]
    out_floats = ooff + (K - 1) * kst + (batch - 1) * obs + (n1 - 1) * so[1] + (n0 - 1) * so[0] + 1
    lanes = {(k, b): ooff + k * kst + b * obs + i1 * so[1] + i0 * so[0] for k in range(K) for b in range(batch)}
    return opts, phys, h, want, out_floats, lanes


def strided_tag():
    return tag_of(STRIDED["P"], STRIDED["ks"])


def check_strided(run, setenv, oracle, unsupported):
    """run(opts, x, out_floats, kernel, out_init) as above; the output starts as 777.0 everywhere and every element outside the lanes keeps it.
    unsupported(opts): asserts that planning the request fails with UNSUPPORTED (the switch at 0: the planner before this route)"""
    from test_emu_fftconv import _close
    opts, phys, h, want, out_floats, lanes = strided_request()
    K = STRIDED["K"]
    setenv(SWITCH, str(STRIDED["P"]))
    sentinel = np.full(out_floats, 777.0, np.float32)
    got, route, launches = run(opts, phys, out_floats, h, sentinel)
    got = np.asarray(got)
    assert strided_tag() in route and launches == 1 + K, (route, launches)
    touched = np.zeros(out_floats, bool)
    for (k, b), idx in lanes.items():
        assert not touched[idx].any(), "the lanes of the request overlap"
        touched[idx] = True
        _close(got[idx].reshape(-1), want[k, b].astype(np.float32).reshape(-1), 4e-3, 4e-3, f"{route.strip()} kernel {k} image {b}")
        assert _rel(got[idx], want[k, b]) <= 1e-5
    assert np.all(got[~touched] == 777.0), "stores outside the output lanes"
    setenv(SWITCH, "0")
    unsupported(opts)


def strided_contract_oracle(oracle, o):
    """exec_contract_cases oracle of the strided request: NaN where the plan's contract leaves the output alone"""
    _, phys, h, want, out_floats, lanes = strided_request()
    full = np.full(out_floats, np.nan)
    for (k, b), idx in lanes.items():
        full[idx] = want[k, b]
    return phys, h, full


# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("rtiles_dense_150x130_k9x5", t._rc([150, 130], [9, 5], 3, boundary="linear-same"), tag_of(64, (9, 5)), t._rconv(0x7EC0), t.TOL_RCONV,
           env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("rtiles_strided_150x130_k9x5", strided_request()[0], strided_tag(), strided_contract_oracle, t.TOL_RCONV,
           env={SWITCH: "64"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure sizes fftconv domains of any rank): one forced and one default case ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("rtiles_default_300x200_k31x17", t._rc([300, 200], [31, 17], 1, K=2, boundary="linear-same"), TAG + "N=", t._rconv(0x7ED0), t.TOL_RCONV, starts=False),
]


# ---- direct sums in float64 (the capability test: windows of a request whose float64 FFT reference is not worth its time) ----
def direct_same_conv(x, h, shape, ks, lo, hi):
    """outputs [lo0, hi0) x [lo1, hi1) of the linear-same convolution of one real image: float64 [hi1 - lo1][hi0 - lo0]"""
    (n0, n1), (m0, m1) = shape, ks
    xr = np.asarray(x, np.float64).reshape(n1, n0)
    hr = np.asarray(h, np.float64).reshape(m1, m0)
    c0, c1 = (m0 - 1) // 2, (m1 - 1) // 2
    out = np.zeros((hi[1] - lo[1], hi[0] - lo[0]))
    for r1 in range(m1):
        for r0 in range(m0):           # y[o] = sum_r h[r] x[o + c - r]
            a1, a0 = np.arange(lo[1], hi[1]) + c1 - r1, np.arange(lo[0], hi[0]) + c0 - r0
            ok1, ok0 = (a1 >= 0) & (a1 < n1), (a0 >= 0) & (a0 < n0)
            blk = np.zeros_like(out)
            blk[np.ix_(ok1, ok0)] = xr[np.ix_(a1[ok1], a0[ok0])]
            out += hr[r1, r0] * blk
    return out
