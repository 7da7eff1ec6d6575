"""Shared by test_emu_fftconv_ols.py and test_gpu_fftconv_ols.py: one table of requests for the overlap-save route of real fftconv
(lines-rconv-ols[N=P,L=L]: plan.cpp build_fftconv_real, kern_lines.hpp fft_lines_rconv_ols_kernel) and the check both tiers run on it.

A case names the request and the block length P the switch forces (names without their prefix: the GPU tier sets MI355FFT_RCONV_OLS, the
emulation tier MI355_EMU_RCONV_OLS); P = None leaves the planner's own rule.  Block geometry: M = kernelShape, e = (M - 1) & 1,
L = (P - (M - 1) - e) & ~1 results a block, nb = ceil((shape + M - 1) / L) blocks a line.

Bars (the project's own for real fftconv): elementwise 4e-3 / 4e-3 and rel_l2 < 1e-5 against numpy float64 (check_against_f64), and
rel_l2 < 1e-6 against the same request planned with the switch at 0 (the routes the planner had before this one).  Every case asserts the
route tag and 1 + K launches."""
import numpy as np

import exec_contract_cases as t
from test_emu_fftconv_real import _check, _opts, _rand, _rel, _want


class OlsCase:
    def __init__(self, name, n, kn, P, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None,
                 kernel_list=False):
        self.name, self.n, self.kn, self.P, self.batch, self.K = name, n, kn, P, batch, K
        self.mode, self.boundary, self.out_layout, self.zero_pad, self.kernel_list = mode, boundary, out_layout, zero_pad, kernel_list

    @property
    def L(self):
        pre = (self.kn - 1) + ((self.kn - 1) & 1)
        return (self.P - pre) & ~1

    @property
    def opts(self):
        return _opts([self.n], [self.kn], self.batch, K=self.K, mode=self.mode, boundary=self.boundary, out_layout=self.out_layout,
                     zero_pad=self.zero_pad)

    def __repr__(self):
        return self.name


MODES = ("convolution", "correlation")
BOUNDARIES = ("linear-full", "linear-same", "linear-valid")

CASES = [
    # 23 blocks a line, odd and even kernel length (L = 226 / 224); batch 37: 851 block-lines, a ragged last tile of 32
    *[OlsCase(f"n5000_k{kn}_{mode[:4]}_{boundary[7:]}", 5000, kn, 256, 37, mode=mode, boundary=boundary)
      for kn in (31, 32) for mode in MODES for boundary in BOUNDARIES],
    # L = 128: the largest kernel a 256-point block takes; the crop of the correlation holds negative and positive lags
    OlsCase("n999_k129_corr_same", 999, 129, 256, 3, mode="correlation"),
    OlsCase("n1000_k1_no_overlap", 1000, 1, 128, 3, boundary="linear-full"),
    OlsCase("n50_k31_single_block", 50, 31, 128, 3, mode="correlation", boundary="linear-full"),
    # zeroPad ranges that cut blocks (L = 64), three kernels given as a list, batch-major lanes
    OlsCase("n700_k65_K3_zero_pad", 700, 65, 128, 5, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
            zero_pad={"read": {"start": [3], "end": [650]}, "write": {"start": [20], "end": [700]}}, kernel_list=True),
    # the planner's own rule
    *[OlsCase(f"default_n20000_k65_{mode[:4]}", 20000, 65, None, 8, K=2, mode=mode) for mode in MODES],
]

_WANT = {}


def data(case):
    """(x, h, float64 reference [K][batch][out]) of a case, computed once per process and read-only"""
    if case.name not in _WANT:
        x, h = _rand(case.n * case.batch, 0x0150 + case.n + case.kn), _rand(case.kn * case.K, 0x0151 + case.kn)
        want = _want(x, h, [case.n], [case.kn], case.batch, case.K, case.mode, case.boundary, case.zero_pad)
        for a in (x, h, want):
            a.setflags(write=False)
        _WANT[case.name] = (x, h, want)
    return _WANT[case.name]


def assert_route(case, route, launches):
    tag = "lines-rconv-ols[N=" if case.P is None else f"lines-rconv-ols[N={case.P},L={case.L}]"
    assert tag in route, route
    assert launches == 1 + case.K, (route, launches)
    assert "pad[" not in route and "bluestein" not in route, route


def check_case(run, setenv, oracle, case):
    """run(opts, x, out_floats, kernel) -> (got, route, launches) plans and runs under the environment; setenv(name, value) sets the tier's
    form of a planner switch"""
    x, h, want = data(case)
    out_floats = want.size
    kernel = [h[k * case.kn:(k + 1) * case.kn] for k in range(case.K)] if case.kernel_list else h
    if case.P is not None:
        setenv("RCONV_OLS", str(case.P))
    got, route, launches = run(case.opts, x, out_floats, kernel)
    assert_route(case, route, launches)
    _check(oracle, got, want, case.batch, case.K, case.out_layout, route)
    setenv("RCONV_OLS", "0")
    ref, route0, launches0 = run(case.opts, x, out_floats, kernel)
    assert "lines-rconv-ols" not in route0, route0
    rel = _rel(got, ref)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel < 1e-6, (route, route0)


# ---- strided lanes on both sides: 5000 (*) 31 linear-same, P = 256 (the values of test_route1_strided_lanes_on_both_sides) ---------
STRIDED = dict(n=5000, kn=31, batch=5, K=2, si=3, so=2, ioff=5, ooff=3, kst=1, P=256)


def strided_request():
    """(opts, physical input, kernels, dense float64 reference [K][batch][n], output floats, lane slices)"""
    s = STRIDED
    n, kn, batch, K, si, so, ioff, ooff, kst = (s[k] for k in ("n", "kn", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
    ibs, obs = n * si + 11, n * so + 7
    layout = {"inputStrides": [si], "outputStrides": [so], "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    opts = _opts([n], [kn], batch, K=K, boundary="linear-same", layout=layout, outputKernelStrideElements=kst)
    if "strided" not in _WANT:
        dense, h = _rand(n * batch, 0x01A1), _rand(kn * K, 0x01A2)
        phys = _rand(ioff + (batch - 1) * ibs + (n - 1) * si + 1, 0x01A3)
        for b in range(batch):
            phys[ioff + b * ibs: ioff + b * ibs + n * si: si] = dense[b * n:(b + 1) * n]
        want = _want(dense, h, [n], [kn], batch, K, "convolution", "linear-same")
        for a in (phys, h, want):
            a.setflags(write=False)
        _WANT["strided"] = (phys, h, want)
    phys, h, want = _WANT["strided"]
    out_floats = ooff + (K - 1) * kst + (batch - 1) * obs + (n - 1) * so + 1
    lanes = {(k, b): slice(ooff + k * kst + b * obs, ooff + k * kst + b * obs + n * so, so) for k in range(K) for b in range(batch)}
    return opts, phys, h, want, out_floats, lanes


def check_strided(run, setenv, oracle):
    """run(opts, x, out_floats, kernel, out_init) as above; the output starts as 777.0 everywhere and every element outside the lanes keeps it"""
    from test_emu_fftconv import _close
    opts, phys, h, want, out_floats, lanes = strided_request()
    setenv("RCONV_OLS", str(STRIDED["P"]))
    sentinel = np.full(out_floats, 777.0, np.float32)
    got, route, launches = run(opts, phys, out_floats, h, sentinel)
    assert f"lines-rconv-ols[N={STRIDED['P']},L=226]" in route and launches == 1 + STRIDED["K"], (route, launches)
    setenv("RCONV_OLS", "0")
    ref, route0, _ = run(opts, phys, out_floats, h, sentinel)
    assert "lines-rconv-ols" not in route0, route0
    touched = np.zeros(out_floats, bool)
    for (k, b), sl in lanes.items():
        touched[sl] = True
        _close(got[sl], want[k, b].astype(np.float32), 4e-3, 4e-3, f"{route.strip()} kernel {k} line {b}")
        assert _rel(got[sl], want[k, b]) < 1e-5
    assert np.all(got[~touched] == 777.0), "stores outside the output lanes"
    rel = _rel(got[touched], ref[touched])
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel < 1e-6, (route, route0)


def strided_contract_oracle(oracle, o):
    """exec_contract_cases oracle of the strided request: NaN where the plan's contract leaves the output alone"""
    _, phys, h, want, out_floats, lanes = strided_request()
    full = np.full(out_floats, np.nan)
    for (k, b), sl in lanes.items():
        full[sl] = want[k, b]
    return phys, h, full


# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("ols_dense_5000x31", t._rc([5000], [31], 37, boundary="linear-same"), "lines-rconv-ols[N=256,L=226]", t._rconv(0xEC90), t.TOL_RCONV,
           env={"RCONV_OLS": "256"}, starts=False, replay=True),
    t.Case("ols_strided_5000x31", strided_request()[0], "lines-rconv-ols[N=256,L=226]", strided_contract_oracle, t.TOL_RCONV,
           env={"RCONV_OLS": "256"}, starts=False, replay=True),
]
