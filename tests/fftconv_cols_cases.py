"""The tables of test_emu_fftconv_cols.py and test_gpu_fftconv_cols.py: the overlap-save route of complex fftconv (lines-conv-ols[N=P,L=L]:
plan.cpp build_fftconv, kern_lines.hpp fft_lines_conv_ols_kernel).  The checks both tiers run on them are fftconv_ols_scaffold.py's.

Bars (the project's own for complex fftconv, exec_contract_cases.TOL_CONV): elementwise 4e-3 / 4e-3 and rel_l2 < 1e-5 against numpy float64
(fftconv_linear_cases.reference), and rel_l2 <= 1e-5 (the parity bar of DESIGN.md section 3) against the same request planned with the switch
at 0: the routes the planner had before this one, Bluestein among them."""
import exec_contract_cases as t
import fftconv_ols_scaffold as s
from fftconv_ols_cases import STRIDED       # the same strided request in complex elements (5000 (*) 31 linear-same, P = 256)
from fftconv_ols_scaffold import BOUNDARIES, MODES

ROUTE = s.Route("CONV_OLS", "lines-conv-ols[", ("pad[", "bluestein", "xcd-"), rank=1, real=False, f64=s.below(1e-5), parity=s.at_most(1e-5),
                seed=0x0C50, strided_seed=0x0CA1, strided=STRIDED)

CASES = [
    # 23 blocks a line, odd and even kernel length (L = 226 / 225); batch 37: 851 block-lines, a ragged last tile of 8
    *[ROUTE.case(f"n5000_k{kn}_{mode[:4]}_{boundary[7:]}", (5000,), (kn,), 256, 37, mode=mode, boundary=boundary)
      for kn in (31, 32) for mode in MODES for boundary in BOUNDARIES],
    # L = 128: the crop of the correlation holds negative and positive lags
    ROUTE.case("n999_k129_corr_same", (999,), (129,), 256, 3, mode="correlation"),
    ROUTE.case("n1000_k1_no_overlap", (1000,), (1,), 128, 3, boundary="linear-full"),
    ROUTE.case("n50_k31_single_block", (50,), (31,), 128, 3, mode="correlation", boundary="linear-full"),
    # zeroPad ranges that cut blocks (L = 64), three kernels, batch-major lanes
    ROUTE.case("n700_k65_K3_zero_pad", (700,), (65,), 128, 5, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
               zero_pad={"read": {"start": [3], "end": [650]}, "write": {"start": [20], "end": [700]}}),
    # the three-stage instance, one line per workgroup; the longest kernel of the default rule
    ROUTE.case("n9000_k513_P4096", (9000,), (513,), 4096, 3),
    # the planner's own rule
    *[ROUTE.case(f"default_n20000_k65_{mode[:4]}", (20000,), (65,), None, 8, K=2, mode=mode) for mode in MODES],
]

# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("cols_dense_5000x31", t._fc([5000], 37, [31], 1, boundary="linear-same"), "lines-conv-ols[N=256,L=226]", ROUTE.dense_oracle(0xEC50), t.TOL_CONV,
           env={"CONV_OLS": "256"}, starts=False, replay=True),
    t.Case("cols_strided_5000x31", ROUTE.strided_request()[0], "lines-conv-ols[N=256,L=226]", ROUTE.strided_contract_oracle, t.TOL_CONV,
           env={"CONV_OLS": "256"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure: three terms at the next power of two >= the logical domain, 4 Y global, 8 Y worst class) ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("cols_default_20000x65", t._fc([20000], 8, [65], 2, boundary="linear-same"), ROUTE.tag + "N=", ROUTE.dense_oracle(0xEC60), t.TOL_CONV, starts=False),
]
