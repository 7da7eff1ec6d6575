"""The tables of test_emu_fftconv_tiles.py and test_gpu_fftconv_tiles.py: the overlap-save tile route of rank-2 complex fftconv
(tiles-spectrum[N=PxP] tiles-conv-ols[N=PxP,L=L0xL1]: plan.cpp emit_tiles_ols, kern_tiles.hpp fft_tiles_conv_ols_kernel).  The checks both
tiers run on them are fftconv_ols_scaffold.py's.

Bars (the project's own for complex fftconv, exec_contract_cases.TOL_CONV): elementwise 4e-3 / 4e-3 and rel_l2 <= 1e-5 against numpy float64
(np.fft.fft2 on the exact linear domain), and rel_l2 <= 1e-5 (the parity bar of DESIGN.md section 3) against the same request planned with
the switch at 0: the routes the planner had before this one."""
import exec_contract_cases as t
import fftconv_ols_scaffold as s
from fftconv_ols_scaffold import BOUNDARIES, MODES

# strided lanes on both sides: rank-2 strides, offsets and batch strides, kernel lanes kst apart
STRIDED = dict(shape=(150, 100), ks=(9, 5), batch=2, K=2, P=64, si=(2, 310), so=(3, 460), ioff=5, ooff=7, kst=1)

ROUTE = s.Route("CONV_OLS2D", "tiles-conv-ols[", ("bluestein", "mixed", "columns", "fftconv["), rank=2, real=False, f64=s.at_most(1e-5), parity=s.at_most(1e-5),
                seed=0x71E0, strided_seed=0x71A1, strided=STRIDED)

CASES = [
    # L = 56 x 60 (55 x 60 for the even kernel) on the domain 158 x 104: 3 x 2 tiles an image, ragged last tiles on both axes, batch 3
    *[ROUTE.case(f"150x100_k{k0}x5_{mode[:4]}_{boundary[7:]}", (150, 100), (k0, 5), 64, 3, mode=mode, boundary=boundary)
      for k0 in (9, 8) for mode in MODES for boundary in BOUNDARIES],
    # L = 32 x 48: the crop of the correlation holds negative and positive lags on both axes
    ROUTE.case("100x70_k33x17_corr_same", (100, 70), (33, 17), 64, 2, mode="correlation"),
    ROUTE.case("90x80_k1x1_no_overlap", (90, 80), (1, 1), 64, 2),
    ROUTE.case("20x30_k9x9_single_tile", (20, 30), (9, 9), 64, 3, boundary="linear-full"),
    # the longest kernel a tile takes on one axis: L0 = 2
    ROUTE.case("70x200_k63x3_L2", (70, 200), (63, 3), 64, 1),
    # zeroPad boxes that cut tiles on both axes (L = 56 x 56 on the domain 138 x 98), three kernels, batch-major lanes
    ROUTE.case("130x90_k9x9_K3_zero_pad", (130, 90), (9, 9), 64, 2, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
               zero_pad={"read": {"start": [3, 5], "end": [120, 70]}, "write": {"start": [20, 10], "end": [130, 95]}}),
    # the 128-point tile: L = 96 x 112 on the domain 232 x 156, 3 x 2 tiles
    ROUTE.case("200x140_k33x17_P128", (200, 140), (33, 17), 128, 2),
    # the planner's own rule
    *[ROUTE.case(f"default_300x200_k31x17_{mode[:4]}", (300, 200), (31, 17), None, 1, K=2, mode=mode, rule=128) for mode in MODES],
    *[ROUTE.case(f"default_300x200_k9x9_{mode[:4]}", (300, 200), (9, 9), None, 1, K=2, mode=mode, rule=64) for mode in MODES],
]

# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("tiles_dense_150x100_k9x5", t._fc([150, 100], 3, [9, 5], 1, boundary="linear-same"), "tiles-conv-ols[N=64x64,L=56x60]", ROUTE.dense_oracle(0x71C0), t.TOL_CONV,
           env={"CONV_OLS2D": "64"}, starts=False, replay=True),
    t.Case("tiles_strided_150x100_k9x5", ROUTE.strided_request()[0], ROUTE.strided_tag(), ROUTE.strided_contract_oracle, t.TOL_CONV,
           env={"CONV_OLS2D": "64"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure sizes fftconv domains of any rank) ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("tiles_default_300x200_k31x17", t._fc([300, 200], 1, [31, 17], 2, boundary="linear-same"), ROUTE.tag + "N=", ROUTE.dense_oracle(0x71D0), t.TOL_CONV, starts=False),
]
