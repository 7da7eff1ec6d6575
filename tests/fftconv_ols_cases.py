"""The tables of test_emu_fftconv_ols.py and test_gpu_fftconv_ols.py: the overlap-save route of real fftconv (lines-rconv-ols[N=P,L=L]:
plan.cpp build_fftconv_real, kern_lines.hpp fft_lines_rconv_ols_kernel).  The checks both tiers run on them are fftconv_ols_scaffold.py's.

Bars (the project's own for real fftconv): elementwise 4e-3 / 4e-3 and rel_l2 < 1e-5 against numpy float64 (check_against_f64), and
rel_l2 < 1e-6 against the same request planned with the switch at 0 (the routes the planner had before this one)."""
import exec_contract_cases as t
import fftconv_ols_scaffold as s
from fftconv_ols_scaffold import BOUNDARIES, MODES

# strided lanes on both sides: 5000 (*) 31 linear-same, P = 256 (the values of test_route1_strided_lanes_on_both_sides)
STRIDED = dict(shape=(5000,), ks=(31,), batch=5, K=2, P=256, si=(3,), so=(2,), ioff=5, ooff=3, kst=1)

ROUTE = s.Route("RCONV_OLS", "lines-rconv-ols[", ("pad[", "bluestein"), rank=1, real=True, f64=s.below(1e-5), parity=s.below(1e-6),
                seed=0x0150, strided_seed=0x01A1, strided=STRIDED)

CASES = [
    # 23 blocks a line, odd and even kernel length (L = 226 / 224); batch 37: 851 block-lines, a ragged last tile of 32
    *[ROUTE.case(f"n5000_k{kn}_{mode[:4]}_{boundary[7:]}", (5000,), (kn,), 256, 37, mode=mode, boundary=boundary)
      for kn in (31, 32) for mode in MODES for boundary in BOUNDARIES],
    # L = 128: the largest kernel a 256-point block takes; the crop of the correlation holds negative and positive lags
    ROUTE.case("n999_k129_corr_same", (999,), (129,), 256, 3, mode="correlation"),
    ROUTE.case("n1000_k1_no_overlap", (1000,), (1,), 128, 3, boundary="linear-full"),
    ROUTE.case("n50_k31_single_block", (50,), (31,), 128, 3, mode="correlation", boundary="linear-full"),
    # zeroPad ranges that cut blocks (L = 64), three kernels given as a list, batch-major lanes
    ROUTE.case("n700_k65_K3_zero_pad", (700,), (65,), 128, 5, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
               zero_pad={"read": {"start": [3], "end": [650]}, "write": {"start": [20], "end": [700]}}, kernel_list=True),
    # the planner's own rule
    *[ROUTE.case(f"default_n20000_k65_{mode[:4]}", (20000,), (65,), None, 8, K=2, mode=mode) for mode in MODES],
]

# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("ols_dense_5000x31", t._rc([5000], [31], 37, boundary="linear-same"), "lines-rconv-ols[N=256,L=226]", ROUTE.dense_oracle(0xEC90), t.TOL_RCONV,
           env={"RCONV_OLS": "256"}, starts=False, replay=True),
    t.Case("ols_strided_5000x31", ROUTE.strided_request()[0], "lines-rconv-ols[N=256,L=226]", ROUTE.strided_contract_oracle, t.TOL_RCONV,
           env={"RCONV_OLS": "256"}, starts=False, replay=True),
]
