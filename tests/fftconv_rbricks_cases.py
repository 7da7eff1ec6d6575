"""The tables of test_emu_fftconv_rbricks.py and test_gpu_fftconv_rbricks.py: the overlap-save brick route of rank-3 REAL fftconv
(bricks-rspectrum[N=16x16x16] bricks-rconv-ols[N=16x16x16,L=L0xL1xL2]: plan.cpp emit_bricks_ols, kern_bricks.hpp fft_bricks_conv_ols_kernel on
an RBrickCfg).  The checks both tiers run on them are fftconv_ols_scaffold.py's; the shapes are fftconv_bricks_cases.table's.

A work item of the kernel is a pair of bricks that are neighbours on axis 2 (one in the real, one in the imaginary parts of a complex brick):
with odd nb_2 the last pair of every column of bricks has no second brick.

Bars (the project's own for real fftconv): elementwise 4e-3 / 4e-3 and rel_l2 <= 1e-5 against numpy float64 (test_emu_fftconv_real._want, any
rank), rel_l2 <= 1e-5 against the same request planned with the switch at 0 (rconv[K]), and rel_l2 <= 1e-5 against the real parts of the
complex plan on the same data with zero imaginary parts, CONV_OLS3D forced alike.  The route names no Bluestein, mixed-radix, column or
rconv[K] launch.  The strided request has no plan at all with the switch at 0."""
import exec_contract_cases as t
import fftconv_bricks_cases as bricks
import fftconv_ols_scaffold as s
from fftconv_bricks_cases import P

UNSUPPORTED = "Unsupported: strided layouts on real fftconv outside the one-launch line route"

# strided lanes on both sides: rank-3 strides, offsets and batch strides in f32 elements, all odd and non-unit on axis 0, so that no element is 8-byte
# aligned by construction; kernel lanes kst apart.  nb = 3 x 2 x 2 bricks
STRIDED = dict(shape=(30, 20, 18), ks=(5, 3, 4), batch=2, K=2, P=P, si=(3, 95, 1911), so=(5, 153, 3075), ioff=5, ooff=7, kst=1)

ROUTE = bricks.BrickRoute("RCONV_OLS3D", "bricks-rconv-ols[", ("bluestein", "mixed", "columns", "fftconv[", "rconv["), rank=3, real=True, f64=s.at_most(1e-5),
                          parity=s.at_most(1e-5), seed=0x4B31, strided_seed=0x4BA1, strided=STRIDED, route0_has="rconv[K=", complex_switch="CONV_OLS3D",
                          unsupported=UNSUPPORTED)

CASES = bricks.table(ROUTE)

# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("rbricks_dense_30x20x18_k5x3x4", t._rc([30, 20, 18], [5, 3, 4], 2, boundary="linear-same"), ROUTE.tag_of(P, (5, 3, 4)), ROUTE.dense_oracle(0x4BC0), t.TOL_RCONV,
           env={"RCONV_OLS3D": "16"}, starts=False, replay=True),
    t.Case("rbricks_strided_30x20x18_k5x3x4", ROUTE.strided_request()[0], ROUTE.strided_tag(), ROUTE.strided_contract_oracle, t.TOL_RCONV,
           env={"RCONV_OLS3D": "16"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure sizes fftconv domains of any rank): one forced and one default case ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("rbricks_default_40x36x34_k3x3x3", t._rc([40, 36, 34], [3, 3, 3], 1, K=2, boundary="linear-same"), ROUTE.tag + "N=", ROUTE.dense_oracle(0x4BD0), t.TOL_RCONV,
           starts=False),
]
