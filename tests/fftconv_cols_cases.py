"""Shared by test_emu_fftconv_cols.py and test_gpu_fftconv_cols.py: one table of requests for the overlap-save route of complex fftconv
(lines-conv-ols[N=P,L=L]: plan.cpp build_fftconv, kern_lines.hpp fft_lines_conv_ols_kernel) and the checks both tiers run on it.

A case names the request and the block length P the switch forces (names without their prefix: the GPU tier sets MI355FFT_CONV_OLS, the
emulation tier MI355_EMU_CONV_OLS); P = None leaves the planner's own rule.  Block geometry: M = kernelShape, L = P - (M - 1) results a
block, nb = ceil((shape + M - 1) / L) blocks a line.

Bars (the project's own for complex fftconv, exec_contract_cases.TOL_CONV): rel_l2 and rel_max <= 1e-5 and elementwise 4e-3 / 4e-3 against
numpy float64 (fftconv_linear_cases.reference), and rel_l2 <= 1e-5 (the parity bar of DESIGN.md section 3) against the same request planned
with the switch at 0: the routes the planner had before this one, Bluestein among them.  Every case asserts the route tag and 1 + K launches."""
import numpy as np

import exec_contract_cases as t
import fftconv_linear_cases as lin
from fftconv_ols_cases import STRIDED
from test_emu_fftconv_real import _rel

SWITCH = "CONV_OLS"
TAG = "lines-conv-ols["
FORBIDDEN = ("pad[", "bluestein", "xcd-")


class ColsCase:
    def __init__(self, name, n, kn, P, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None):
        self.name, self.n, self.kn, self.P, self.batch, self.K = name, n, kn, P, batch, K
        self.mode, self.boundary, self.out_layout, self.zero_pad = mode, boundary, out_layout, zero_pad

    @property
    def lin(self):
        """the request as a case tuple of fftconv_linear_cases.py"""
        return (self.n, self.kn, self.boundary, self.mode, self.K, self.out_layout, self.zero_pad)

    @property
    def L(self):
        return self.P - (self.kn - 1)

    @property
    def opts(self):
        return lin.options(self.lin, self.batch)

    def __repr__(self):
        return self.name


MODES = ("convolution", "correlation")
BOUNDARIES = ("linear-full", "linear-same", "linear-valid")

CASES = [
    # 23 blocks a line, odd and even kernel length (L = 226 / 225); batch 37: 851 block-lines, a ragged last tile of 8
    *[ColsCase(f"n5000_k{kn}_{mode[:4]}_{boundary[7:]}", 5000, kn, 256, 37, mode=mode, boundary=boundary)
      for kn in (31, 32) for mode in MODES for boundary in BOUNDARIES],
    # L = 128: the crop of the correlation holds negative and positive lags
    ColsCase("n999_k129_corr_same", 999, 129, 256, 3, mode="correlation"),
    ColsCase("n1000_k1_no_overlap", 1000, 1, 128, 3, boundary="linear-full"),
    ColsCase("n50_k31_single_block", 50, 31, 128, 3, mode="correlation", boundary="linear-full"),
    # zeroPad ranges that cut blocks (L = 64), three kernels, batch-major lanes
    ColsCase("n700_k65_K3_zero_pad", 700, 65, 128, 5, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
             zero_pad={"read": {"start": [3], "end": [650]}, "write": {"start": [20], "end": [700]}}),
    # the three-stage instance, one line per workgroup; the longest kernel of the default rule
    ColsCase("n9000_k513_P4096", 9000, 513, 4096, 3),
    # the planner's own rule
    *[ColsCase(f"default_n20000_k65_{mode[:4]}", 20000, 65, None, 8, K=2, mode=mode) for mode in MODES],
]

_WANT = {}


def _rand(n, seed):
    """n complex elements, interleaved f32"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, 2 * n).astype(np.float32)


def data(case):
    """(x, h, float64 reference in the plan's output layout, flat) of a case, computed once per process and read-only"""
    if case.name not in _WANT:
        x, h = _rand(case.n * case.batch, 0x0C50 + case.n + case.kn), _rand(case.kn * case.K, 0x0C51 + case.kn)
        want = lin.reference(case.lin, x, h, case.batch)                  # [K][batch][on][2]
        if case.out_layout != "kernel-major":
            want = want.transpose(1, 0, 2, 3)
        want = np.ascontiguousarray(want).reshape(-1)
        for a in (x, h, want):
            a.setflags(write=False)
        _WANT[case.name] = (x, h, want)
    return _WANT[case.name]


def assert_route(case, route, launches):
    tag = TAG + "N=" if case.P is None else f"{TAG}N={case.P},L={case.L}]"
    assert tag in route, route
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
    assert _rel(got, want) < 1e-5
    setenv(SWITCH, "0")
    ref, route0, _ = run(case.opts, x, want.size, h)
    assert TAG not in route0, route0
    rel = _rel(got, ref)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= 1e-5, (route, route0)


# ---- strided lanes on both sides: the STRIDED request of fftconv_ols_cases.py in complex elements (5000 (*) 31 linear-same, P = 256) -----------
def strided_request():
    """(opts, physical input, kernels, float64 reference [K][batch][n][2], output floats, lane slices in complex elements)"""
    s = STRIDED
    n, kn, batch, K, si, so, ioff, ooff, kst = (s[k] for k in ("n", "kn", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
    ibs, obs = n * si + 11, n * so + 7
    layout = {"interleavedComplex": True, "inputStrides": [si], "outputStrides": [so], "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    opts = lin.options((n, kn, "linear-same", "convolution", K, "kernel-major", None), batch)
    opts["layout"] = layout
    opts["fftConv"]["outputKernelStrideElements"] = kst
    if "strided" not in _WANT:
        dense, h = _rand(n * batch, 0x0CA1), _rand(kn * K, 0x0CA2)
        phys = _rand(ioff + (batch - 1) * ibs + (n - 1) * si + 1, 0x0CA3).reshape(-1, 2)
        for b in range(batch):
            phys[ioff + b * ibs: ioff + b * ibs + n * si: si] = dense.reshape(-1, 2)[b * n:(b + 1) * n]
        want = lin.reference((n, kn, "linear-same", "convolution", K, "kernel-major", None), dense, h, batch)
        phys = phys.reshape(-1)
        for a in (phys, h, want):
            a.setflags(write=False)
        _WANT["strided"] = (phys, h, want)
    phys, h, want = _WANT["strided"]
    out_elems = ooff + (K - 1) * kst + (batch - 1) * obs + (n - 1) * so + 1
    lanes = {(k, b): slice(ooff + k * kst + b * obs, ooff + k * kst + b * obs + n * so, so) for k in range(K) for b in range(batch)}
    return opts, phys, h, want, 2 * out_elems, lanes


def check_strided(run, setenv, oracle):
    """run(opts, x, out_floats, kernel, out_init) as above; the output starts as 777.0 everywhere and every element outside the lanes keeps it"""
    from test_emu_fftconv import _close
    opts, phys, h, want, out_floats, lanes = strided_request()
    P, K = STRIDED["P"], STRIDED["K"]
    setenv(SWITCH, str(P))
    sentinel = np.full(out_floats, 777.0, np.float32)
    got, route, launches = run(opts, phys, out_floats, h, sentinel)
    assert f"{TAG}N={P},L={P - STRIDED['kn'] + 1}]" in route and launches == 1 + K, (route, launches)
    setenv(SWITCH, "0")
    ref, route0, _ = run(opts, phys, out_floats, h, sentinel)
    assert TAG not in route0, route0
    got2, ref2 = np.asarray(got).reshape(-1, 2), np.asarray(ref).reshape(-1, 2)
    touched = np.zeros(out_floats // 2, bool)
    for (k, b), sl in lanes.items():
        touched[sl] = True
        _close(got2[sl].reshape(-1), want[k, b].astype(np.float32).reshape(-1), 4e-3, 4e-3, f"{route.strip()} kernel {k} line {b}")
        assert _rel(got2[sl], want[k, b]) < 1e-5
    assert np.all(got2[~touched] == 777.0), "stores outside the output lanes"
    rel = _rel(got2[touched], ref2[touched])
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= 1e-5, (route, route0)


def strided_contract_oracle(oracle, o):
    """exec_contract_cases oracle of the strided request: NaN where the plan's contract leaves the output alone"""
    _, phys, h, want, out_floats, lanes = strided_request()
    full = np.full((out_floats // 2, 2), np.nan)
    for (k, b), sl in lanes.items():
        full[sl] = want[k, b]
    return phys, h, full.reshape(-1)


def _dense_oracle(seed):
    """a dense rank-1 linear request against fftconv_linear_cases.reference, in the plan's output layout"""
    def f(oracle, o):
        fc, n, batch = o["fftConv"], o["shape"][0], o["batch"]
        case = (n, fc["kernelShape"][0], fc["boundary"], fc["mode"], fc["kernelCount"], fc["outputLayout"], o.get("zeroPad"))
        x, h = _rand(n * batch, seed), _rand(case[1] * case[4], seed + 1)
        want = lin.reference(case, x, h, batch)
        if case[5] != "kernel-major":
            want = want.transpose(1, 0, 2, 3)
        return x, h, np.ascontiguousarray(want).reshape(-1)
    return f


# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("cols_dense_5000x31", t._fc([5000], 37, [31], 1, boundary="linear-same"), "lines-conv-ols[N=256,L=226]", _dense_oracle(0xEC50), t.TOL_CONV,
           env={SWITCH: "256"}, starts=False, replay=True),
    t.Case("cols_strided_5000x31", strided_request()[0], "lines-conv-ols[N=256,L=226]", strided_contract_oracle, t.TOL_CONV,
           env={SWITCH: "256"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure: three terms at the next power of two >= the logical domain, 4 Y global, 8 Y worst class) ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("cols_default_20000x65", t._fc([20000], 8, [65], 2, boundary="linear-same"), TAG + "N=", _dense_oracle(0xEC60), t.TOL_CONV, starts=False),
]


# ---- direct sums in float64 (the capability test: windows of a request too long for a float64 FFT reference to be worth its time) ----
def direct_same_conv(x, h, n, kn, lo, hi):
    """outputs [lo, hi) of the linear-same convolution of one line: complex128"""
    xc = np.asarray(x, np.float64).reshape(-1, 2)[:n]
    xc = xc[:, 0] + 1j * xc[:, 1]
    hc = np.asarray(h, np.float64).reshape(-1, 2)[:kn]
    hc = hc[:, 0] + 1j * hc[:, 1]
    off = (kn - 1) // 2
    a, b = max(0, lo + off - (kn - 1)), min(n, hi + off)          # the samples the window reads
    full = np.convolve(xc[a:b], hc)                               # full[i] is logical index a + i
    return full[lo + off - a: hi + off - a]
