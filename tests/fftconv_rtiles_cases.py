"""The tables of test_emu_fftconv_rtiles.py and test_gpu_fftconv_rtiles.py: the overlap-save tile route of rank-2 REAL fftconv
(tiles-rspectrum[N=PxP] tiles-rconv-ols[N=PxP,L=L0xL1]: plan.cpp emit_tiles_ols, kern_tiles.hpp fft_tiles_conv_ols_kernel on an RTileCfg).
The checks both tiers run on them are fftconv_ols_scaffold.py's.

A work item of the kernel is a pair of tiles that are neighbours on axis 1 (one in the real, one in the imaginary parts of a complex tile):
with odd nb_1 the last pair of every row has no second tile.

Bars (the project's own for real fftconv and for the tile table): elementwise 4e-3 / 4e-3 and rel_l2 <= 1e-5 against numpy float64
(test_emu_fftconv_real._want), rel_l2 <= 1e-5 against the same request planned with the switch at 0 (the routes the planner had before this
one: rconv[K]), and rel_l2 <= 1e-5 against the real parts of the complex plan on the same data with zero imaginary parts, CONV_OLS2D forced
alike.  The route names no Bluestein, mixed-radix, column or rconv[K] launch.  The strided request has no plan at all with the switch at 0."""
import exec_contract_cases as t
import fftconv_ols_scaffold as s
from fftconv_ols_scaffold import BOUNDARIES, MODES

UNSUPPORTED = "Unsupported: strided layouts on real fftconv outside the one-launch line route"

# strided lanes on both sides: rank-2 strides, offsets and batch strides in f32 elements, kernel lanes kst apart; odd strides and offsets, so that
# no element is 8-byte aligned by construction.  nb = 3 x 3 tiles: the second pair row has no partner
STRIDED = dict(shape=(150, 130), ks=(9, 5), batch=2, K=2, P=64, si=(3, 455), so=(5, 761), ioff=5, ooff=7, kst=1)

ROUTE = s.Route("RCONV_OLS2D", "tiles-rconv-ols[", ("bluestein", "mixed", "columns", "rconv["), rank=2, real=True, f64=s.at_most(1e-5), parity=s.at_most(1e-5),
                seed=0x7E10, strided_seed=0x7EA1, strided=STRIDED, route0_has="rconv[K=", complex_switch="CONV_OLS2D", unsupported=UNSUPPORTED)

CASES = [
    # L = 56 x 60 (55 x 60 for the even kernel) on the domain 158 x 134: 3 x 3 tiles an image, so two pair rows of which the second has no partner;
    # ragged last tiles on both axes, batch 3
    *[ROUTE.case(f"150x130_k{k0}x5_{mode[:4]}_{boundary[7:]}", (150, 130), (k0, 5), 64, 3, mode=mode, boundary=boundary)
      for k0 in (9, 8) for mode in MODES for boundary in BOUNDARIES],
    # the domain 158 x 104: nb_1 = 2, every partner is there
    ROUTE.case("150x100_k9x5_both_partners", (150, 100), (9, 5), 64, 2),
    # L = 32 x 48: the crop of the correlation holds negative and positive lags on both axes, for both partners
    ROUTE.case("100x70_k33x17_corr_same", (100, 70), (33, 17), 64, 2, mode="correlation"),
    ROUTE.case("90x80_k1x1_no_overlap", (90, 80), (1, 1), 64, 2),
    # one tile: the partner is absent everywhere
    ROUTE.case("20x30_k9x9_single_tile", (20, 30), (9, 9), 64, 3, boundary="linear-full"),
    # the longest kernel a tile takes on one axis: L0 = 2
    ROUTE.case("70x200_k63x3_L2", (70, 200), (63, 3), 64, 1),
    # zeroPad boxes that cut tiles and pairs on both axes (L = 56 x 56 on the domain 138 x 98), three kernels, batch-major lanes
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
    t.Case("rtiles_dense_150x130_k9x5", t._rc([150, 130], [9, 5], 3, boundary="linear-same"), ROUTE.tag_of(64, (9, 5)), ROUTE.dense_oracle(0x7EC0), t.TOL_RCONV,
           env={"RCONV_OLS2D": "64"}, starts=False, replay=True),
    t.Case("rtiles_strided_150x130_k9x5", ROUTE.strided_request()[0], ROUTE.strided_tag(), ROUTE.strided_contract_oracle, t.TOL_RCONV,
           env={"RCONV_OLS2D": "64"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure sizes fftconv domains of any rank): one forced and one default case ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("rtiles_default_300x200_k31x17", t._rc([300, 200], [31, 17], 1, K=2, boundary="linear-same"), ROUTE.tag + "N=", ROUTE.dense_oracle(0x7ED0), t.TOL_RCONV, starts=False),
]
