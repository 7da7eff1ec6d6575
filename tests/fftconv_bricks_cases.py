"""The tables of test_emu_fftconv_bricks.py and test_gpu_fftconv_bricks.py: the overlap-save brick route of rank-3 complex fftconv
(bricks-spectrum[N=16x16x16] bricks-conv-ols[N=16x16x16,L=L0xL1xL2]: plan.cpp emit_bricks_ols, kern_bricks.hpp fft_bricks_conv_ols_kernel).
The checks both tiers run on them are fftconv_ols_scaffold.py's.

Bars (the project's own for complex fftconv, exec_contract_cases.TOL_CONV): elementwise 4e-3 / 4e-3 and rel_l2 <= 1e-5 against numpy float64
(np.fft.fftn on the exact linear domain shape + kernelShape - 1), and rel_l2 <= 1e-5 (the parity bar of DESIGN.md section 3) against the same
request planned with the switch at 0: the routes the planner had before this one.

The shapes are the smallest at which each index path of the kernel can go wrong; the brick is 16 points an axis, so L_a = 17 - M_a."""
import numpy as np

import exec_contract_cases as t
import fftconv_linear_cases as lin
import fftconv_ols_scaffold as s
from fftconv_ols_scaffold import BOUNDARIES, MODES

P = 16
# the longest kernel edge the planner's default rule gives to the brick (plan.cpp CONV_BRICKS_MAX_KERNEL / RCONV_BRICKS_MAX_KERNEL, as measured:
# profiles/fftconv_bricks_ab.log, profiles/fftconv_rbricks_ab.log); beyond it the switch alone
RULE_MAX_KERNEL = 9


class BrickRoute(s.Route):
    """rank 3: the tag names three block lengths, and complex data have a float64 reference over three axes"""
    def tag_of(self, P, ks):
        return f"{self.tag}N={P}x{P}x{P},L={P - ks[0] + 1}x{P - ks[1] + 1}x{P - ks[2] + 1}]"

    def reference(self, shape, ks, batch, K, mode, boundary, zero_pad, x, h):
        if self.real:
            return super().reference(shape, ks, batch, K, mode, boundary, zero_pad, x, h)
        return reference3d(shape, ks, batch, K, mode, boundary, zero_pad, x, h)


def _box(zr, dom):
    """a zeroPad range as a boolean mask over the domain (numpy order: axis 2, axis 1, axis 0)"""
    keep = np.zeros(tuple(dom)[::-1], bool)
    keep[tuple(slice(max(0, a), max(0, b)) for a, b in zip(zr["start"][::-1], zr["end"][::-1]))] = True
    return keep


def reference3d(shape, ks, batch, K, mode, boundary, zero_pad, x, h):
    """float64 reference [K][batch][os2][os1][os0][2] of dense complex data x [batch][n2][n1][n0] and kernels h [K][m2][m1][m0] (interleaved f32)"""
    geo = [lin.geometry((n, kn, boundary)) for n, kn in zip(shape, ks)]
    fs, os_, cs = ([g[i] for g in geo] for i in range(3))
    xc = np.asarray(x, np.float64).reshape((batch,) + tuple(shape)[::-1] + (2,))
    xc = xc[..., 0] + 1j * xc[..., 1]
    if zero_pad and zero_pad.get("read"):
        xc = np.where(_box(zero_pad["read"], shape), xc, 0)
    hc = np.asarray(h, np.float64).reshape((K,) + tuple(ks)[::-1] + (2,))
    hc = hc[..., 0] + 1j * hc[..., 1]
    X = np.fft.fftn(xc, s=fs[::-1], axes=(1, 2, 3))
    want = np.empty((K, batch) + tuple(os_)[::-1] + (2,))
    for k in range(K):
        H = np.fft.fftn(hc[k], s=fs[::-1], axes=(0, 1, 2))
        y = np.fft.ifftn(X * (np.conj(H) if mode == "correlation" else H), axes=(1, 2, 3))
        if zero_pad and zero_pad.get("write"):
            y = np.where(_box(zero_pad["write"], fs), y, 0)
        y = y[(slice(None),) + tuple(slice(c, c + o) for c, o in zip(cs[::-1], os_[::-1]))]
        want[k, ..., 0], want[k, ..., 1] = y.real, y.imag
    return want


# strided lanes on both sides: rank-3 strides, offsets and batch strides, all odd and non-unit on axis 0, kernel lanes kst apart
STRIDED = dict(shape=(30, 20, 18), ks=(5, 3, 4), batch=2, K=2, P=P, si=(3, 95, 1911), so=(5, 153, 3075), ioff=5, ooff=7, kst=1)

ROUTE = BrickRoute("CONV_OLS3D", "bricks-conv-ols[", ("bluestein", "mixed", "columns", "fftconv["), rank=3, real=False, f64=s.at_most(1e-5),
                   parity=s.at_most(1e-5), seed=0xB31C, strided_seed=0xB3A1, strided=STRIDED)

ZERO_PAD = {"read": {"start": [3, 5, 2], "end": [24, 18, 17]}, "write": {"start": [6, 4, 5], "end": [27, 25, 21]}}


def table(route):
    """the case table of a route: the same shapes serve complex and real data"""
    c = route.case
    return [
        # L = 12 x 14 x 13 (11 for the even kernel) on the domain 34 x 22 x 21: 3 x 2 x 2 bricks a volume, ragged last bricks on every axis, nb_2 = 2
        # (real data: both partners present), batch 2
        *[c(f"30x20x18_k{k0}x3x4_{mode[:4]}_{boundary[7:]}", (30, 20, 18), (k0, 3, 4), P, 2, mode=mode, boundary=boundary)
          for k0 in (5, 4) for mode in MODES for boundary in BOUNDARIES],
        # the domain 34 x 22 x 33: nb_2 = 3, the last pair of real bricks has no partner
        c("30x20x30_k5x3x4_odd_nb2", (30, 20, 30), (5, 3, 4), P, 2),
        # L = 8: 4 x 3 x 3 bricks; on axis 2 the last brick's partner is absent
        c("20x12x10_k9x9x9_full", (20, 12, 10), (9, 9, 9), P, 2, boundary="linear-full"),
        c("24x24x24_k1x1x1_no_overlap", (24, 24, 24), (1, 1, 1), P, 2),
        # the longest kernel a brick takes on one axis: L0 = 2
        c("20x40x20_k15x3x3_L2", (20, 40, 20), (15, 3, 3), P, 1),
        # L = 8 x 12 x 14: the crop of the correlation holds negative and positive lags on all axes (real data: for both partners)
        c("28x22x20_k9x5x3_corr_same", (28, 22, 20), (9, 5, 3), P, 2, mode="correlation"),
        # zeroPad boxes that cut bricks and pairs on all three axes (L = 12 on the domain 30 x 26 x 24), three kernels, batch-major lanes
        c("26x22x20_k5x5x5_K3_zero_pad", (26, 22, 20), (5, 5, 5), P, 2, K=3, mode="correlation", boundary="linear-full", out_layout="batch-major",
          zero_pad=ZERO_PAD),
        # kernels given as a list of K arrays (the scaffold cuts the list in f32 elements: real data)
        *([c("30x20x18_k5x3x4_kernel_list", (30, 20, 18), (5, 3, 4), P, 2, K=2, kernel_list=True)] if route.real else []),
        # the planner's own rule
        *[c(f"default_40x36x34_k3x3x3_{mode[:4]}", (40, 36, 34), (3, 3, 3), None, 1, K=2, mode=mode, rule=P) for mode in MODES],
    ]


CASES = table(ROUTE)

# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules) ----
CONTRACT_CASES = [
    t.Case("bricks_dense_30x20x18_k5x3x4", t._fc([30, 20, 18], 2, [5, 3, 4], 1, boundary="linear-same"), ROUTE.tag_of(P, (5, 3, 4)), ROUTE.dense_oracle(0xB3C0),
           t.TOL_CONV, env={"CONV_OLS3D": "16"}, starts=False, replay=True),
    t.Case("bricks_strided_30x20x18_k5x3x4", ROUTE.strided_request()[0], ROUTE.strided_tag(), ROUTE.strided_contract_oracle, t.TOL_CONV,
           env={"CONV_OLS3D": "16"}, starts=False, replay=True),
]

# ---- accuracy ladder (accuracy_cases.measure sizes fftconv domains of any rank) ----
ACCURACY_CASES = [
    CONTRACT_CASES[0],
    t.Case("bricks_default_40x36x34_k3x3x3", t._fc([40, 36, 34], 1, [3, 3, 3], 2, boundary="linear-same"), ROUTE.tag + "N=", ROUTE.dense_oracle(0xB3D0), t.TOL_CONV,
           starts=False),
]
