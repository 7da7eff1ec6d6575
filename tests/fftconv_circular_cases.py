"""The tables of test_emu_fftconv_circular.py and test_gpu_fftconv_circular.py: boundary "circular" on the six overlap-save routes of fftconv
(lines-conv-ols, lines-rconv-ols, tiles-conv-ols, tiles-rconv-ols, bricks-conv-ols, bricks-rconv-ols with ",wrap" as the last field of the tag:
plan.cpp ols_axis / ols_circular_take, the kernels' WRAP instances).  The checks both tiers run on them are fftconv_ols_scaffold.py's.

One switch serves the six routes: OLS_CIRCULAR (0: the plans the planner had before, 1: the default rule, 2: power-of-two domains as well).  No case
forces a block: a circular request runs on the block its route's own rule names (Case.rule), and the route's own switch forced to a block does not
move it.  Geometry per axis: N = shape, L as for the linear route, nb = ceil(N / L); the route is taken where shape >= 2 P on every axis.

References are numpy float64 circular convolutions / correlations on the exact domain (the scaffold's, which take "circular").  The bars are the
linear routes' own (each CircularRoute copies them from the Route object of the same kernel): the arithmetic between the first load and the last
store is the same.

The shapes are the smallest that exercise each instance and each way the seam can go wrong: a head that wraps (convolution), a tail that wraps,
a last block cut at N, odd N on real lines (sample pairs across the seam, the parity flip behind it), an absent partner of a real pair (odd nb
on the paired axis), corner tiles and bricks that wrap on every axis at once."""
import numpy as np

import exec_contract_cases as t
import fftconv_bricks_cases as bricks
import fftconv_cols_cases as cols
import fftconv_ols_cases as ols
import fftconv_ols_scaffold as s
import fftconv_rbricks_cases as rbricks
import fftconv_rtiles_cases as rtiles
import fftconv_tiles_cases as tiles
from fftconv_ols_scaffold import MODES
from test_emu_fftconv_real import _opts

SWITCH = "OLS_CIRCULAR"
UNSUPPORTED = rtiles.UNSUPPORTED


class _Circular:
    """the linear Route of the same kernel with what it hard-codes for linear boundaries replaced: the tag's last field, the boundary of a case
    and of the strided request, and the switch (which takes 0 / 1 / 2, not a block)"""
    def tag_of(self, P, ks):
        return super().tag_of(P, ks)[:-1] + ",wrap]"

    def case(self, name, shape, ks, rule, batch, **kw):
        return s.Case(self, name, shape, ks, None, batch, boundary="circular", rule=rule, **kw)

    def strided_request(self):
        """Route.strided_request with boundary "circular": (opts, physical input, kernels, float64 reference [K][batch][out], output floats, lanes)"""
        d = self.strided
        shape, ks, batch, K, si, so, ioff, ooff, kst = (d[k] for k in ("shape", "ks", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
        ibs, obs = shape[-1] * si[-1] + 11, shape[-1] * so[-1] + 7
        layout = {"inputStrides": list(si), "outputStrides": list(so), "inputOffsetElements": ioff, "outputOffsetElements": ooff,
                  "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
        if self.real:
            opts = _opts(list(shape), list(ks), batch, K=K, boundary="circular", layout=layout, outputKernelStrideElements=kst)
        else:
            opts = s.options(shape, ks, batch, K, boundary="circular")
            opts["layout"] = dict(layout, interleavedComplex=True)
            opts["fftConv"]["outputKernelStrideElements"] = kst
        index = np.meshgrid(*(np.arange(n) for n in shape[::-1]), indexing="ij")[::-1]       # per axis, in numpy order
        ipos, opos = sum(i * st for i, st in zip(index, si)), sum(i * st for i, st in zip(index, so))
        width = () if self.real else (2,)
        if "strided" not in self._want:
            n, kn = int(np.prod(shape)), int(np.prod(ks))
            dense, h = self.rand(n * batch, self.strided_seed), self.rand(kn * K, self.strided_seed + 1)
            phys = self.rand(ioff + (batch - 1) * ibs + int(ipos.max()) + 1, self.strided_seed + 2).reshape((-1,) + width)
            for b in range(batch):
                phys[ioff + b * ibs + ipos] = dense.reshape((batch,) + shape[::-1] + width)[b]
            want = self.reference(shape, ks, batch, K, "convolution", "circular", None, dense, h)
            phys = phys.reshape(-1)
            for a in (phys, h, want):
                a.setflags(write=False)
            self._want["strided"] = (phys, h, want)
        phys, h, want = self._want["strided"]
        out_elems = ooff + (K - 1) * kst + (batch - 1) * obs + int(opos.max()) + 1
        lanes = {(k, b): ooff + k * kst + b * obs + opos for k in range(K) for b in range(batch)}
        return opts, phys, h, want, out_elems * (1 if self.real else 2), lanes

    def check_strided(self, run, setenv, oracle, unsupported=None):
        """the scaffold's check with the switch at 1 where it would force the block"""
        super().check_strided(run, lambda name, value: setenv(name, value if value == "0" else "1"), oracle, unsupported)


def circular(base, seed, strided, unsupported=None):
    """the circular form of the linear Route `base`: its class, tag, bars, forbidden launches and route0_has"""
    cls = type("Circular" + type(base).__name__, (_Circular, type(base)), {})
    return cls(SWITCH, base.tag, base.forbidden, rank=base.rank, real=base.real, f64=base.f64, parity=base.parity, seed=seed, strided_seed=seed + 0x100,
               strided=strided, route0_has=base.route0_has, complex_switch=SWITCH if base.real else None, unsupported=unsupported)


# strided lanes on both sides (strides, offsets and batch strides in elements, all odd or non-unit on axis 0; kernel lanes kst apart) on the table's
# smallest shapes: every axis wraps, the real pairs have an absent partner (nb = 3 on the paired axis)
LINES = circular(cols.ROUTE, 0xC1C0, dict(shape=(16411,), ks=(65,), batch=2, K=2, P=2048, si=(3,), so=(2,), ioff=5, ooff=3, kst=1))
RLINES = circular(ols.ROUTE, 0xC1D0, dict(shape=(8193,), ks=(31,), batch=3, K=2, P=1024, si=(3,), so=(2,), ioff=5, ooff=3, kst=1), UNSUPPORTED)      # (an odd strided line: no plan with the switch at 0)
TILES = circular(tiles.ROUTE, 0xC1E0, dict(shape=(150, 130), ks=(9, 5), batch=2, K=2, P=64, si=(2, 310), so=(3, 460), ioff=5, ooff=7, kst=1))
RTILES = circular(rtiles.ROUTE, 0xC1F0, dict(shape=(150, 130), ks=(9, 5), batch=2, K=2, P=64, si=(3, 455), so=(5, 761), ioff=5, ooff=7, kst=1), UNSUPPORTED)
BRICKS = circular(bricks.ROUTE, 0xC200, dict(shape=(40, 36, 34), ks=(5, 3, 4), batch=2, K=2, P=16, si=(3, 125, 4511), so=(5, 203, 7315), ioff=5, ooff=7, kst=1))
RBRICKS = circular(rbricks.ROUTE, 0xC210, dict(shape=(40, 36, 34), ks=(5, 3, 4), batch=2, K=2, P=16, si=(3, 125, 4511), so=(5, 203, 7315), ioff=5, ooff=7, kst=1),
                   UNSUPPORTED)
ROUTES = (LINES, RLINES, TILES, RTILES, BRICKS, RBRICKS)


def _zero_pad(shape):
    """ranges that a seam block cuts on every axis: read [5, N - 3), write [0, N - 7)"""
    return {"read": {"start": [5] * len(shape), "end": [n - 3 for n in shape]}, "write": {"start": [0] * len(shape), "end": [n - 7 for n in shape]}}


def _both(route, name, shape, ks, rule, batch, **kw):
    return [route.case(f"{name}_{mode[:4]}", shape, ks, rule, batch, mode=mode, **kw) for mode in MODES]


def _lines(r):
    real = r.real
    return [
        *((  # real lines, P = 1024: odd N: sample pairs across the seam, the parity flip behind it; L = 994, nb = 9
            *_both(r, "n8193_k31", (8193,), (31,), 1024, 3, K=2),
            # P = 2048, odd pre - 1 (e = 1: pre = 200, L = 1848) with odd N
            r.case("n9001_k200_e1", (9001,), (200,), 2048, 2),
            r.case("n9001_k200_e1_corr", (9001,), (200,), 2048, 1, mode="correlation"),
            # P = 8192: the shape just above 2 P, L = 7892, nb = 3
            r.case("n16385_k300_P8192", (16385,), (300,), 8192, 1),
            r.case("n8200_k1_no_halo", (8200,), (1,), 1024, 2),
            r.case("n8946_k31_multiple_of_L", (8946,), (31,), 1024, 2),                                       # 9 x 994
            *_both(r, "n8193_k31_zero_pad", (8193,), (31,), 1024, 2, zero_pad=_zero_pad((8193,)), out_layout="batch-major"),
        ) if real else (
            # complex lines, P = 2048: the head wraps (convolution), the tail wraps, the last block is cut at N; L = 1984, nb = 9
            *_both(r, "n16411_k65", (16411,), (65,), 2048, 3, K=2),
            # P = 4096: a larger halo, L = 3797, nb = 5
            r.case("n16500_k300_P4096_corr", (16500,), (300,), 4096, 2, mode="correlation", out_layout="batch-major"),
            r.case("n16500_k300_P4096_conv", (16500,), (300,), 4096, 1),
            r.case("n16400_k1_no_halo", (16400,), (1,), 2048, 2),
            r.case("n17856_k65_multiple_of_L", (17856,), (65,), 2048, 2),                                     # 9 x 1984
            *_both(r, "n16411_k65_zero_pad", (16411,), (65,), 2048, 2, zero_pad=_zero_pad((16411,)), out_layout="batch-major"),
        )),
    ]


def _tiles(r):
    return [
        # P = 64, L = 56 x 60: nb = 3 x 3 (real: the last pair has no partner) and 3 x 4; both axes wrap, the corner tiles on both at once
        *_both(r, "150x130_k9x5", (150, 130), (9, 5), 64, 2),
        *_both(r, "150x200_k9x5", (150, 200), (9, 5), 64, 2, K=2),
        # P = 128, L = 98 x 112: nb = 4 x 3: the instance at its register limit
        *_both(r, "300x260_k31x17_P128", (300, 260), (31, 17), 128, 1),
        r.case("150x130_k1x1_no_halo", (150, 130), (1, 1), 64, 2),
        r.case("168x180_k9x5_multiple_of_L", (168, 180), (9, 5), 64, 1),                                      # 3 x 56, 3 x 60
        *_both(r, "150x130_k9x5_zero_pad", (150, 130), (9, 5), 64, 2, zero_pad=_zero_pad((150, 130)), out_layout="batch-major"),
    ]


def _bricks(r):
    return [
        # L = 14^3: nb = 3 x 3 x 3 (real: the last pair on axis 2 has no partner); L = 12 x 14 x 13: nb = 4 x 3 x 4.  Three wrapping axes
        *_both(r, "40x36x34_k3x3x3", (40, 36, 34), (3, 3, 3), 16, 2),
        *_both(r, "40x36x50_k5x3x4", (40, 36, 50), (5, 3, 4), 16, 1, K=2),
        r.case("40x36x34_k1x1x1_no_halo", (40, 36, 34), (1, 1, 1), 16, 1),
        r.case("42x42x42_k3x3x3_multiple_of_L", (42, 42, 42), (3, 3, 3), 16, 1),                              # 3 x 14
        *_both(r, "40x36x34_k3x3x3_zero_pad", (40, 36, 34), (3, 3, 3), 16, 1, zero_pad=_zero_pad((40, 36, 34)), out_layout="batch-major"),
    ]


CASES = [(r, c) for r, table in ((LINES, _lines), (RLINES, _lines), (TILES, _tiles), (RTILES, _tiles), (BRICKS, _bricks), (RBRICKS, _bricks))
         for c in table(r)]


def case_id(rc):
    route, case = rc
    return f"{route.tag[:-1]}:{case.name}"


# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay (the harnesses of the two exec-contract modules): one dense and
# one strided request per route, on the default rule ----
def _dense(route, name, shape, ks, batch, rule, seed):
    opts = t._rc(list(shape), list(ks), batch) if route.real else t._fc(list(shape), batch, list(ks), 1)
    return t.Case(name, opts, route.tag_of(rule, ks), route.dense_oracle(seed), t.TOL_RCONV if route.real else t.TOL_CONV, env={SWITCH: "1"}, starts=False, replay=True)


def _strided(route, name):
    return t.Case(name, route.strided_request()[0], route.strided_tag(), route.strided_contract_oracle, t.TOL_RCONV if route.real else t.TOL_CONV,
                  env={SWITCH: "1"}, starts=False, replay=True)


CONTRACT_CASES = [
    _dense(LINES, "circular_lines_dense_16411x65", (16411,), (65,), 3, 2048, 0xC300), _strided(LINES, "circular_lines_strided_16411x65"),
    _dense(RLINES, "circular_rlines_dense_8193x31", (8193,), (31,), 3, 1024, 0xC310), _strided(RLINES, "circular_rlines_strided_8193x31"),
    _dense(TILES, "circular_tiles_dense_150x130_k9x5", (150, 130), (9, 5), 2, 64, 0xC320), _strided(TILES, "circular_tiles_strided_150x130_k9x5"),
    _dense(RTILES, "circular_rtiles_dense_150x130_k9x5", (150, 130), (9, 5), 2, 64, 0xC330), _strided(RTILES, "circular_rtiles_strided_150x130_k9x5"),
    _dense(BRICKS, "circular_bricks_dense_40x36x34_k3x3x3", (40, 36, 34), (3, 3, 3), 2, 16, 0xC340), _strided(BRICKS, "circular_bricks_strided_40x36x34_k5x3x4"),
    _dense(RBRICKS, "circular_rbricks_dense_40x36x34_k3x3x3", (40, 36, 34), (3, 3, 3), 2, 16, 0xC350), _strided(RBRICKS, "circular_rbricks_strided_40x36x34_k5x3x4"),
]
