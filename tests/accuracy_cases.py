"""Shared by test_gpu_accuracy.py and test_emu_accuracy.py: the rounding error of every route against a float64 transform of the same f32
input, held to a multiple of the f32 oracle's own error.

The parity bars (rel_l2, rel_max <= 1e-5) sit 40 - 100 times above the kernels and cannot see a lost digit.  Here every case is compared
with numpy's float64 FFT of its input (exact(case, x, kern): the plan's normalisation, layout, ioView and zeroPad applied in float64; NaN
where the plan's contract leaves the output alone), and the bound is built from one measured quantity:

  y(P)  the rel_l2 of the pow2 oracle (radix 2, an f32 store after every butterfly: oracle.c2c_ref_batch) against float64 at the power of
        two P, forward, unnormalised, on seeded random_complex_batch input of at least 2^16 points.  Measured per P, once per process, and
        guarded: y(P) <= 0.5 * 2^-24 * sqrt(log2 P) for P >= 8 (measured 0.43 - 0.48), so a degraded oracle cannot loosen the bars.
  Y     sqrt(sum y(P_i)^2) over the FFT passes a result goes through (terms()):
          c2c, r2c, c2r of any rank or length   one term, P = the next power of two >= prod(shape)
          Bluestein                             three terms at the M of the route tag (two transforms and the inverse of the convolution)
          fftconv, complex or real              three terms at the next power of two >= the logical FFT domain (data, kernel, inverse)
          DCT, DST                              two terms at the next power of two >= 2N (transform and phase pass)
        A case may add derived terms (Case.extra: multiples of one f32 rounding, 2^-24 / sqrt(3) rms relative); the derivation stands beside
        the case.  No case needs one.

  global      rel_l2(got, exact) <= 4 Y          (4: the ratio test_gpu_parity.test_accuracy_against_f64 uses against the same oracle)
  worst class rms of the error over a class / rms of exact over everything <= 8 Y.  The classes: every batch line, and for rank-1 lines
              of L >= 4096 points the sets k mod s and k div s with s from both factors of the route's N1xN2 tag (none: s = 2^floor(log2(L) / 2)).
              For every case of rank > 1 that is no fftconv, for every axis a of the output (the packed axis of r2c has N0 / 2 + 1 indices)
              and every index i, the written elements with index i on axis a: one column-tile lane, one ragged last tile, one index of a
              strided axis (logged as [axis a idx i]).
              Classes of fewer than 256 written real values are left out (256 values scatter by less than 20 %).

Both metrics run over the elements the plan writes.  f16-storage plans are not here: their error is the final binary16 rounding, which
test_*_f16_storage.py own."""
import re

import numpy as np

import exec_contract_cases as t
import fftconv_ols_cases as ols
from exec_contract_cases import FOUR_STEP, FUSED, REAL, Case, _o

U = 2.0 ** -24
GLOBAL_FACTOR, CLASS_FACTOR, MIN_CLASS = 4.0, 8.0, 256


def _pow2_at_least(n):
    return 1 << max(1, int(n - 1).bit_length())


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
_Y = {}


def y(oracle, P):
    """the oracle's own rel_l2 against float64 at the power of two P (cached per process)"""
    if P not in _Y:
        assert P >= 2 and P & (P - 1) == 0, P
        batch = max(1, (1 << 16) // P)
        x = oracle.random_complex_batch(P, batch, 0xACC00000 + P)
        exact = np.fft.fft(x.astype(np.float64).view(np.complex128), axis=1).view(np.float64)
        v = float(oracle.rel_l2(oracle.c2c_ref_batch(x.reshape(-1), [P], batch, "forward", "none").reshape(batch, -1), exact))
        lg = P.bit_length() - 1
        assert v > 0.0 and (P < 8 or v <= 0.5 * U * np.sqrt(lg)), f"the oracle's own error at P = 2^{lg} is {v:.3e}: the yardstick is degraded"
        _Y[P] = v
    return _Y[P]


def terms(case, route):
    """the powers of two of the FFT passes a result of `case` goes through on `route`"""
    o = case.opts
    if o["type"] == "fftconv":
        ks = o["fftConv"].get("kernelShape") or o["shape"]
        dom = o["shape"] if o["fftConv"].get("boundary", "circular") == "circular" else [s + k - 1 for s, k in zip(o["shape"], ks)]
        return [_pow2_at_least(int(np.prod(dom)))] * 3
    if o["type"][:3] in ("dct", "dst"):
        return [_pow2_at_least(2 * int(np.prod(o["shape"])))] * 2
    if "bluestein" in route:
        m = re.search(r"bluestein[^\[]*\[[^\]]*M=(\d+)", route)
        assert m, route
        return [int(m.group(1))] * 3
    return [_pow2_at_least(int(np.prod(o["shape"])))]


def yardstick(oracle, case, route):
    return float(np.sqrt(sum(y(oracle, P) ** 2 for P in terms(case, route)) + sum((c * U / np.sqrt(3.0)) ** 2 for c in getattr(case, "extra", ()))))


# ---- float64 references -------------------------------------------------------------------------------------------------------------
def _scale(o, n):
    norm, inverse = o.get("normalize", "none"), o["direction"] == "inverse"
    return {"none": 1.0, "unitary": 1.0 / np.sqrt(n), "backward": 1.0 / n if inverse else 1.0}[norm]


def _cplx(x, lead, shape):
    """interleaved f32 -> complex128 [lead, *reversed(shape)] (axis 0 of the plan is the fastest)"""
    c = np.asarray(x, np.float64).reshape(lead, *reversed(shape), 2)
    return c[..., 0] + 1j * c[..., 1]


def _inter(c):
    return np.stack([c.real, c.imag], axis=-1)


def _window(shape, view_shape, offset):
    """slices (logical, view) of the part of a view that lies on the logical domain: view coordinate v is logical coordinate v + offset"""
    lo = [max(0, -offset[d]) for d in range(len(shape))]
    hi = [min(view_shape[d], shape[d] - offset[d]) for d in range(len(shape))]
    view = tuple(slice(lo[d], max(lo[d], hi[d])) for d in reversed(range(len(shape))))
    logical = tuple(slice(lo[d] + offset[d], max(lo[d], hi[d]) + offset[d]) for d in reversed(range(len(shape))))
    return logical, view


def _box_mask(shape, box):
    m = np.zeros(tuple(reversed(shape)), bool)
    m[tuple(slice(box["start"][d], box["end"][d]) for d in reversed(range(len(shape))))] = True
    return m


def exact_c2c(o, x):
    # the resolved view offsets and zeroPad boxes come from the project's own resolver, so a resolver bug would be shared with the plan;
    # test_emu_accuracy.test_view_and_fftconv_references_are_the_tables_oracles holds these references to the tables' hand-written oracles
    from mi355fft.layout import resolve_plan_options
    if _lanes(o):       # channel lanes: [batch][channels][n] on both sides, the plan's lane transformed, the others untouched
        channels, cidx = _lanes(o)
        n, batch = o["shape"][0], o["batch"]
        assert len(o["shape"]) == 1 and not o.get("ioView") and not o.get("zeroPad")
        dense = dict(o, layout={"interleavedComplex": True})
        out = np.full((batch, channels, 2 * n), np.nan)
        out[:, cidx] = exact_c2c(dense, np.asarray(x).reshape(batch, channels, 2 * n)[:, cidx]).reshape(batch, 2 * n)
        return out.reshape(-1)
    r = resolve_plan_options(o)
    shape, batch, n = o["shape"], o["batch"], int(np.prod(o["shape"]))
    vin, vout = r["io_view"]["input"], r["io_view"]["output"]
    zr, zw = r["zero_pad"]["read"], r["zero_pad"]["write"]
    axes = tuple(range(1, len(shape) + 1))
    if vin:
        logical = np.zeros((batch, *reversed(shape)), np.complex128)
        lg, vw = _window(shape, vin["shape"], vin["offset"])
        logical[(slice(None), *lg)] = _cplx(x, batch, vin["shape"])[(slice(None), *vw)]
    else:
        logical = _cplx(x, batch, shape)
    if zr:
        logical = logical * _box_mask(shape, zr)
    w = (np.fft.fftn(logical, axes=axes) if o["direction"] == "forward" else np.fft.ifftn(logical, axes=axes) * n) * _scale(o, n)
    if zw:
        w = w * _box_mask(shape, zw)
    if not vout:
        return _inter(w).reshape(-1)
    out = np.full((batch, *reversed(vout["shape"]), 2), 0.0 if vout.get("clearOutside") else np.nan)
    lg, vw = _window(shape, vout["shape"], vout["offset"])
    out[(slice(None), *vw)] = _inter(w[(slice(None), *lg)])
    return out.reshape(-1)


def exact_r2c(o, x):
    shape, batch, n = o["shape"], o["batch"], int(np.prod(o["shape"]))
    assert not o.get("ioView") and not o.get("zeroPad")
    r = np.asarray(x, np.float64).reshape(batch, *reversed(shape))
    w = np.fft.rfftn(r, axes=tuple(range(1, len(shape) + 1))) * _scale(o, n)      # the halved axis is numpy's last: the plan's axis 0
    return _inter(w).reshape(-1)


def exact_c2r(o, x):
    """any rank without views: numpy's irfftn over the plan's axes of the packed spectrum (the halved axis is numpy's last: the plan's
    axis 0).  rank 1 also with ioView as test_r2c_c2r_ioview_and_zeropad uses it (the first bins in, a window of a larger real array out)"""
    shape, batch = o["shape"], o["batch"]
    assert not o.get("zeroPad")
    view = o.get("ioView")
    if len(shape) > 1:
        assert not view
        n = int(np.prod(shape))
        spec = _cplx(x, batch, [shape[0] // 2 + 1] + list(shape[1:]))
        sig = np.fft.irfftn(spec, s=tuple(reversed(shape)), axes=tuple(range(1, len(shape) + 1))) * n * _scale(o, n)
        return sig.reshape(-1)
    n = shape[0]
    bins = view["input"]["shape"][0] if view else n // 2 + 1
    spec = np.zeros((batch, n // 2 + 1), np.complex128)
    spec[:, :bins] = _cplx(x, batch, [bins])
    sig = np.fft.irfft(spec, n=n, axis=1) * n * _scale(o, n)
    if not view:
        return sig.reshape(-1)
    on, lead = view["output"]["shape"][0], -view["output"]["offset"][0]
    out = np.full((batch, on), 0.0 if view["output"].get("clearOutside") else np.nan)
    out[:, lead:lead + n] = sig
    return out.reshape(-1)


# DCT / DST I - IV as the float64 FFT of the symmetric extension.  Every kind is sum_n c_n x_n f(2 pi i_n j_k / M) with f = cos or sin on a
# grid fine enough for the half-sample shifts (M = 4N for the types II / III, 8N for IV, 2(N -/+ 1) for I): the even (cos) or odd (sin)
# extension z[i_n] = c_n x_n / 2, z[M - i_n] = +/- c_n x_n / 2 has the transform sum_n c_n x_n cos(...) or -i sum_n c_n x_n sin(...).
# kinds as oracle.trig_kind: the typeKind table of the oracle's trig1d_ref.
def _trig_grid(kind, N):
    n = np.arange(N)
    c = np.ones(N)
    if kind == 0:
        c[1:N - 1] = 2.0
        return 2 * (N - 1), n, n, c
    if kind in (1, 5):
        return 4 * N, 2 * n + 1, n + (kind == 5), c
    if kind == 2:
        c[0] = 0.5
        return 4 * N, n, 2 * n + 1, c
    if kind == 6:
        c[N - 1] = 0.5
        return 4 * N, n + 1, 2 * n + 1, c
    if kind == 4:
        return 2 * (N + 1), n + 1, n + 1, c
    return 8 * N, 2 * n + 1, 2 * n + 1, c


def trig1d_exact(x, kind):
    """[lines, N] float64 -> [lines, N]"""
    x = np.asarray(x, np.float64)
    N = x.shape[-1]
    M, i_in, j_out, c = _trig_grid(kind, N)
    sine = kind >= 4
    z = np.zeros((x.shape[0], M))
    np.add.at(z, (slice(None), i_in % M), 0.5 * c * x)
    np.add.at(z, (slice(None), (M - i_in) % M), (-0.5 if sine else 0.5) * c * x)
    Z = np.fft.fft(z, axis=1)
    return -Z.imag[:, j_out] if sine else Z.real[:, j_out]


def exact_trig(oracle, o, x):
    """any rank: trig1d_exact along every axis in turn, one final scale by prod(shape) (as oracle.trig_ref_batch, without its f32 stores)"""
    shape, batch, n = o["shape"], o["batch"], int(np.prod(o["shape"]))
    kind = oracle.trig_kind(o["type"], o["direction"])
    v = np.asarray(x, np.float64).reshape(batch, *reversed(shape))
    for a in range(len(shape)):
        m = np.moveaxis(v, len(shape) - a, -1)          # the plan's axis a, last
        v = np.moveaxis(trig1d_exact(m.reshape(-1, shape[a]), kind).reshape(m.shape), -1, len(shape) - a)
    return (v * _scale(o, n)).reshape(-1)


def exact_fftconv(o, x, kern):
    """fftconv through float64 FFTs on the logical domain (circular: shape, linear: shape + kernelShape - 1), complex or real, any rank:
    [K][batch][out] or, batch-major, [batch][K][out]"""
    from mi355fft.layout import resolve_plan_options
    fc, shape, batch = o["fftConv"], o["shape"], o["batch"]       # (resolve_plan_options: see exact_c2c)
    real = o.get("layout", {}).get("interleavedComplex") is False
    ks, K = list(fc.get("kernelShape") or shape), fc.get("kernelCount", 1)
    boundary, rank = fc.get("boundary", "circular"), len(shape)
    fs = list(shape) if boundary == "circular" else [s + k - 1 for s, k in zip(shape, ks)]
    os_ = {"circular": shape, "linear-full": fs, "linear-same": shape, "linear-valid": [s - k + 1 for s, k in zip(shape, ks)]}[boundary]
    off = {"linear-same": [(k - 1) // 2 for k in ks], "linear-valid": [k - 1 for k in ks]}.get(boundary, [0] * rank)
    zp = resolve_plan_options(o)["zero_pad"]

    def load(a, lead, sh):
        if real:
            return np.asarray(a, np.float64).reshape(lead, *reversed(sh)).astype(np.complex128)
        return _cplx(a, lead, sh)

    def embed(a, lead, sh):
        p = np.zeros((lead, *reversed(fs)), np.complex128)
        p[(slice(None), *(slice(0, s) for s in reversed(sh)))] = a
        return p

    axes = tuple(range(1, rank + 1))
    xp = embed(load(x, batch, shape), batch, shape)
    if zp.get("read"):
        xp = xp * _box_mask(fs, zp["read"])
    X, H = np.fft.fftn(xp, axes=axes), np.fft.fftn(embed(load(kern, K, ks), K, ks), axes=axes)
    if fc.get("mode", "convolution") == "correlation":
        H = np.conj(H)
    crop = (slice(None), *(slice(f, f + n) for f, n in zip(reversed(off), reversed(os_))))
    out = []
    for k in range(K):
        v = np.fft.ifftn(X * H[k], axes=axes)
        if zp.get("write"):
            v = v * _box_mask(fs, zp["write"])
        v = v[crop].reshape(batch, -1)
        out.append(v.real if real else _inter(v).reshape(batch, -1))
    out = np.stack(out)
    if fc.get("outputLayout", "kernel-major") != "kernel-major":
        out = out.transpose(1, 0, 2)
    return np.ascontiguousarray(out).reshape(-1)


def exact(oracle, case, x, kern):
    o = case.opts
    typ = o["type"]
    if typ == "c2c":
        return exact_c2c(o, x)
    if typ == "r2c":
        return exact_r2c(o, x)
    if typ == "c2r":
        return exact_c2r(o, x)
    if typ == "fftconv":
        return exact_fftconv(o, x, kern)
    return exact_trig(oracle, o, x)


# ---- inputs of the cases added here (the table's own cases keep theirs: exec_contract_cases.data) -------------------------------------
def _in_c2c(seed):
    return lambda oracle, o: (oracle.random_complex_batch(int(np.prod(o["shape"])), o["batch"], seed).reshape(-1), None)


def _in_real(seed):
    return lambda oracle, o: (oracle.random_real_batch(int(np.prod(o["shape"])), o["batch"], seed).reshape(-1), None)


def _in_spectrum(seed):
    """the float64 spectrum of seeded real noise, scaled to the signal's rms and rounded to f32: Hermitian input of a c2r plan"""
    def f(oracle, o):
        shape, batch, n = o["shape"], o["batch"], int(np.prod(o["shape"]))
        sig = oracle.random_real_batch(n, batch, seed).astype(np.float64).reshape(batch, *reversed(shape))
        spec = np.fft.rfftn(sig, axes=tuple(range(1, len(shape) + 1))) / np.sqrt(n)      # any rank; the halved axis is the plan's axis 0
        return _inter(spec).astype(np.float32).reshape(-1), None
    return f


def _lanes(o):
    w = (o.get("layout") or {}).get("whdcn")
    return (w["channels"], w["channelIndex"]) if w else None


def _in_lanes(seed):
    """dense seeded lines in lane channelIndex of a [batch][channels][n] buffer, 9.0 in the other lanes"""
    def f(oracle, o):
        n, batch = o["shape"][0], o["batch"]
        channels, cidx = _lanes(o)
        phys = np.full((batch, channels, 2 * n), 9.0, np.float32)
        phys[:, cidx] = oracle.random_complex_batch(n, batch, seed)
        return phys.reshape(-1), None
    return f


class ACase(Case):
    """a case of this module: Case with make(oracle, opts) -> (x, kernel) in the oracle's place (no f32 oracle is computed)"""

    def __init__(self, name, opts, route, make, env=None, emu_env=None, emu=True, starts=True, extra=()):
        super().__init__(name, opts, route, None, None, env=env, emu_env=emu_env, emu=emu, starts=starts)
        self.make, self.extra = make, tuple(extra)


_EMU_POINTS = 3 << 19       # cases above this many points take more than a few seconds under emulation


def _emu(opts):
    return int(np.prod(opts["shape"])) * opts["batch"] <= _EMU_POINTS


def _ragged_batch(lg):
    """the smallest batch that leaves a ragged last tile (lines a workgroup: line_kernels.def) or group; at most 3 from 2^17 up"""
    return 65 if lg <= 5 else 33 if lg <= 7 else 9 if lg <= 10 else 3 if lg <= 20 else 2 if lg == 21 else 1


def _default_route(lg):
    if lg <= 12 or lg == 14:
        return f"lines[N={1 << lg}]"
    return {13: "line-reg[N=8192]", 15: "line32k[N=32768]", 16: "xcd-solo[", 20: "xcd-fused-rt32[", 22: "xcd-fused-rt["}.get(lg, "xcd-fused[")


DIRECTIONS = (("forward", "none"), ("inverse", "backward"))
NEW = []

# c2c at every power of two on its default route
for _lg in range(1, 23):
    for _d, _nm in DIRECTIONS:
        _opts = _o("c2c", [1 << _lg], _ragged_batch(_lg), _d, _nm)
        NEW.append(ACase(f"c2c_2p{_lg}_{_d}", _opts, _default_route(_lg), _in_c2c(0xAC100 + _lg), emu_env=FUSED, emu=_emu(_opts)))

# every alternative instance of xcd_kernels.def / line_kernels.def that the switches reach: the grid of test_c2c_two_pass
GRID = dict(FOUR_STEP, SOLO_MAX_KB="1024")
for _fused in (0, 1, 2, 3, 4):
    for _lg in range(13, 23):
        if _fused and _lg < 15 or (_fused == 2 and _lg != 20) or (_fused >= 3 and _lg != 21):
            continue
        _env = dict(GRID, XCD_FUSED=str(min(_fused, 1)), XCD_RT={2: "0", 3: "2", 4: "3"}.get(_fused, "1"), XCD_HX="0" if _fused == 2 else "2")
        _tag = ("two-pass[" if not _fused else "xcd-solo[" if _lg <= 17 else "xcd-fused-rt[" if (_lg == 22 and _fused == 1) or _fused == 3
                else "xcd-fused-rt32[" if (_lg == 20 and _fused == 1) or _fused == 4 else "xcd-fused[")
        for _d, _nm in DIRECTIONS:
            _opts = _o("c2c", [1 << _lg], 3 if _lg <= 18 else 2 if _lg <= 21 else 1, _d, _nm)
            NEW.append(ACase(f"grid{_fused}_2p{_lg}_{_d}", _opts, _tag, _in_c2c(0xAC200 + 32 * _fused + _lg), env=_env, emu=_emu(_opts)))
# 2^20 on the opt-in forms: two workgroups per CU, 16-line register tiles twice, the XCD-resident kernel
for _name, _env, _tag in (("hx1", {"XCD_HX": "1"}, "xcd-fused-2wg[N=1024x1024]"), ("hx3", {"XCD_HX": "3"}, "xcd-fused-rt16x2[N=1024x1024]"),
                          ("res", {"XCD_RES": "1"}, "xcd-resident[N=1024x1024,")):
    for _d, _nm in DIRECTIONS:
        NEW.append(ACase(f"{_name}_2p20_{_d}", _o("c2c", [1 << 20], 3, _d, _nm), _tag, _in_c2c(0xAC300), env=_env, emu=False))

# LINE32K=2: the register line at 2^14 and 2^12; LINE32K=0 with the default MAX_LINE: 2^13 in LDS, its last stage table read from global
# memory.  Batches: more lines than the emulator's grid (2 CUs x 2 / 8 workgroups), so the kernels' loop over lines runs there; on the
# device test_c2c_single_workgroup_long_lines runs it with 1500 lines
for _name, _n, _b, _env, _tag in (("line_reg16384", 16384, 5, {"LINE32K": "2"}, "line-reg[N=16384]"), ("line_reg4096", 4096, 17, {"LINE32K": "2"}, "line-reg[N=4096]"),
                                  ("lines8192", 8192, 3, {"LINE32K": "0"}, "lines[N=8192]")):
    for _d, _nm in DIRECTIONS:
        NEW.append(ACase(f"{_name}_{_d}", _o("c2c", [_n], _b, _d, _nm), _tag, _in_c2c(0xAC380 + _b), env=_env))

# channel lanes (layout.whdcn): lane 2 of 4, the line kernel and the fused four-step kernels with the two pitches, and the gather / scatter
# pair of the other lengths.  The physical buffers hold 4 lanes a batch item; the plan reads and writes one
LANES = {"interleavedComplex": True, "whdcn": {"channels": 4, "channelIndex": 2}}
for _name, _n, _tag, _kw in (("lanes_64", 64, ("lines[N=64,pitch=256/256]",), {}), ("lanes_60", 60, ("gather", "scatter"), {"starts": False}),
                             ("lanes_2p18", 1 << 18, ("lanes[pitch=",), {"starts": False, "emu_env": FUSED}),
                             ("lanes_2p20", 1 << 20, ("lanes[pitch=",), {"starts": False, "emu": False})):
    for _d, _nm in DIRECTIONS:
        NEW.append(ACase(f"{_name}_{_d}", _o("c2c", [_n], 3, _d, _nm, layout=dict(LANES)), _tag, _in_lanes(0xAC3C0 + _n % 251), **_kw))

# r2c / c2r on the fused and register-tile real routes
for _lg in range(17, 23):
    _b = 3 if _lg <= 20 else 2 if _lg == 21 else 1
    _opts = _o("r2c", [1 << _lg], _b)
    NEW.append(ACase(f"r2c_2p{_lg}", _opts, "xcd-r2c-rt[" if _lg >= 21 else "xcd-r2c[N=", _in_real(0xAC400 + _lg), emu_env=FUSED, emu=_emu(_opts)))
    _opts = _o("c2r", [1 << _lg], _b, "inverse", "backward")
    NEW.append(ACase(f"c2r_2p{_lg}", _opts, "xcd-c2r-rt[" if _lg >= 21 else "xcd-c2r-solo[" if _lg == 17 else "xcd-c2r[N=", _in_spectrum(0xAC440 + _lg),
                     emu_env=FUSED, emu=_emu(_opts)))

# DCT / DST: the paths that call sincospif on the GPU
for _typ in ("dct2", "dct3", "dst2", "dst3"):
    for _n in (128, 4096, 32768):
        NEW.append(ACase(f"lines_{_typ}_{_n}", _o(_typ, [_n], 3, layout=dict(REAL)), f"lines-{_typ}[N={_n}]", _in_real(0xAC500 + _n)))
NEW += [
    ACase("trig_real_dst4_256", _o("dst4", [256], 5, "inverse", "backward", layout=dict(REAL)), "trig-real[", _in_real(0xAC520)),
    ACase("trig_real_dst1_255", _o("dst1", [255], 5, layout=dict(REAL)), "trig-real[", _in_real(0xAC521)),
    ACase("trig_real_dct3_256", _o("dct3", [256], 5, layout=dict(REAL)), "trig-real[", _in_real(0xAC522), env={"TRIG_FUSED": "0"}),
    ACase("trig_dct2_256", _o("dct2", [256], 5, layout=dict(REAL)), "trig[", _in_real(0xAC523), env={"TRIG_REAL": "0", "TRIG_FUSED": "0"}, starts=False),
    ACase("trig_dct1_257", _o("dct1", [257], 5, "inverse", "backward", layout=dict(REAL)), "trig[", _in_real(0xAC524),
          env={"TRIG_REAL": "0", "TRIG_FUSED": "0"}, starts=False),
    ACase("trig_dct4_17", _o("dct4", [17], 37, layout=dict(REAL)), "trig[", _in_real(0xAC525), starts=False),
    ACase("trig_dst3_17", _o("dst3", [17], 37, "inverse", "backward", layout=dict(REAL)), "trig[", _in_real(0xAC526), starts=False),
    ACase("trig_real_dst1_17", _o("dst1", [17], 37, layout=dict(REAL)), "trig-real[", _in_real(0xAC527)),
]

# unitary once per kernel family (the table has it for lines, xcd-2d, columns, mixed-ct and the mapped lines)
_U = ("forward", "unitary")
NEW += [
    ACase("unitary_line_reg8192", _o("c2c", [8192], 3, *_U), "line-reg[N=8192]", _in_c2c(0xAC600)),
    ACase("unitary_line32k", _o("c2c", [1 << 15], 3, "inverse", "unitary"), "line32k[N=32768]", _in_c2c(0xAC601)),
    ACase("unitary_xcd_solo_2p16", _o("c2c", [1 << 16], 3, *_U), "xcd-solo[", _in_c2c(0xAC602), emu_env=FUSED),
    ACase("unitary_xcd_fused_2p17", _o("c2c", [1 << 17], 2, "inverse", "unitary"), "xcd-fused[", _in_c2c(0xAC603), emu_env=FUSED),
    ACase("unitary_xcd_fused_rt32_2p20", _o("c2c", [1 << 20], 2, *_U), "xcd-fused-rt32[", _in_c2c(0xAC604), emu=False),
    ACase("unitary_xcd_fused_rt_2p22", _o("c2c", [1 << 22], 1, "inverse", "unitary"), "xcd-fused-rt[", _in_c2c(0xAC605), emu=False),
    ACase("unitary_two_pass_2p17", _o("c2c", [1 << 17], 2, *_U), "two-pass[", _in_c2c(0xAC606), env={"XCD_FUSED": "0"}),
    ACase("unitary_stages_3x4096", _o("c2c", [3 * 4096], 3, *_U), "stages[", _in_c2c(0xAC607), env={"MIXED_CT": "0"}),
    ACase("unitary_mixed_lines1001", _o("c2c", [1001], 5, "inverse", "unitary"), "mixed-lines[", _in_c2c(0xAC608), env={"MIXED_LINES": "2", "MIXED_CT": "0"}),
    ACase("unitary_bluestein_lines2039", _o("c2c", [2039], 3, *_U), "bluestein-lines[", _in_c2c(0xAC609), env={"FUSE_VIEWS": "1"}),
    ACase("unitary_lines_r2c256", _o("r2c", [256], 37, *_U), "lines-r2c[N=", _in_real(0xAC60A)),
    ACase("unitary_lines_c2r256", _o("c2r", [256], 37, "inverse", "unitary"), "lines-c2r[N=", _in_spectrum(0xAC60B)),
    ACase("unitary_xcd_r2c_2p17", _o("r2c", [1 << 17], 2, *_U), "xcd-r2c[N=", _in_real(0xAC60C), emu_env=FUSED),
    ACase("unitary_xcd_c2r_2p18", _o("c2r", [1 << 18], 1, "inverse", "unitary"), "xcd-c2r[N=", _in_spectrum(0xAC60D), emu_env=FUSED),
    ACase("unitary_lines_dct2_128", _o("dct2", [128], 5, *_U, layout=dict(REAL)), "lines-dct2[N=128]", _in_real(0xAC60E)),
    ACase("unitary_trig_real_dct4_256", _o("dct4", [256], 5, "inverse", "unitary", layout=dict(REAL)), "trig-real[", _in_real(0xAC60F)),
]

TABLE = [c for c in t.CASES + ols.CONTRACT_CASES[:1] if not c.f16]
CASES = TABLE + NEW
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_DATA = {}


def data(oracle, case):
    """(x, kernel or None, exact float64 in the plan's output layout, untouched mask) of a case, computed once per process and read-only"""
    if case.name not in _DATA:
        x, kern = case.make(oracle, case.opts) if isinstance(case, ACase) else t.data(oracle, case)[:2]
        x = np.ascontiguousarray(x, np.float32)
        kern = None if kern is None else np.ascontiguousarray(kern, np.float32)
        want = np.asarray(exact(oracle, case, x, kern), np.float64).reshape(-1)
        keep = np.isnan(want)
        for a in (x, kern, want, keep):
            if a is not None:
                a.setflags(write=False)
        _DATA[case.name] = (x, kern, want, keep)
    return _DATA[case.name]


def forget(case):
    """drops a case's cached arrays (the 2^20 ... 2^22 cases are used by one test each)"""
    _DATA.pop(case.name, None)


# ---- the metrics --------------------------------------------------------------------------------------------------------------------
def _out_shape(o):
    """the shape of a batch item of the output of a plan that is no fftconv: the output view's, the packed one of r2c, else the plan's"""
    view = (o.get("ioView") or {}).get("output")
    return list(view["shape"] if view else [o["shape"][0] // 2 + 1] + list(o["shape"][1:]) if o["type"] == "r2c" else o["shape"])


def _line_geometry(case):
    """(lines, points a line, reals a point, rank-1) of the plan's output"""
    o = case.opts
    typ, rank1 = o["type"], len(o["shape"]) == 1
    if typ == "fftconv":
        fc = o["fftConv"]
        ks, b = fc.get("kernelShape") or o["shape"], fc.get("boundary", "circular")
        shape = {"circular": o["shape"], "linear-same": o["shape"], "linear-full": [s + k - 1 for s, k in zip(o["shape"], ks)],
                 "linear-valid": [s - k + 1 for s, k in zip(o["shape"], ks)]}[b]
        return o["batch"] * fc.get("kernelCount", 1), int(np.prod(shape)), 1 if o.get("layout", {}).get("interleavedComplex") is False else 2, rank1
    shape = _out_shape(o)
    if _lanes(o):       # every lane of the buffer is a line; the untouched ones hold no written value and form no class
        return o["batch"] * _lanes(o)[0], int(np.prod(shape)), 2, rank1
    return o["batch"], int(np.prod(shape)), 2 if typ in ("c2c", "r2c") else 1, rank1


def _splits(route, L):
    m = re.search(r"\[(?:N=)?(\d+)x(\d+)", route)       # the tag's own factors: not the 16x2 of xcd-fused-rt16x2[N=1024x1024]
    if m:
        return sorted({int(m.group(1)), int(m.group(2))})
    return [1 << ((L.bit_length() - 1) // 2)]


def measure(oracle, case, route, got, want, keep, prefix=""):
    """asserts both bounds; returns the log line of the case (prefix: what a caller's log puts in front of it)"""
    what = f"{case.name} ({route.strip()})"
    a = np.asarray(got, np.float32).astype(np.float64)
    w = ~keep
    assert np.isfinite(a[w]).all(), f"{what}: the output is not finite"
    err2 = np.where(w, a - np.where(w, want, 0.0), 0.0) ** 2
    count = int(np.count_nonzero(w))
    ref_ms = float(np.sum(np.where(w, want, 0.0) ** 2)) / count
    assert ref_ms > 0.0, what
    rel = float(np.sqrt(np.sum(err2) / count / ref_ms))
    lines, L, per, rank1 = _line_geometry(case)
    assert lines * L * per == want.size, (case.name, lines, L, per, want.size)
    e3, w3 = err2.reshape(lines, L, per), w.reshape(lines, L, per)
    groups = [("line", e3.sum(axis=(1, 2)), w3.sum(axis=(1, 2)))]
    if rank1 and L >= 4096:
        for s in _splits(route, L):
            pad = -L % s
            e2 = np.pad(e3.sum(axis=(0, 2)), (0, pad)).reshape(-1, s)
            n2 = np.pad(w3.sum(axis=(0, 2)), (0, pad)).reshape(-1, s)
            groups += [(f"k mod {s}", e2.sum(axis=0), n2.sum(axis=0)), (f"k div {s}", e2.sum(axis=1), n2.sum(axis=1))]
    if not rank1 and case.opts["type"] != "fftconv":       # every index of every axis of the output, over the batch and the other axes
        oshape = _out_shape(case.opts)
        eN, wN = err2.reshape(lines, *reversed(oshape), per), w.reshape(lines, *reversed(oshape), per)
        for a in range(len(oshape)):
            others = tuple(d for d in range(eN.ndim) if d != len(oshape) - a)
            groups.append((f"axis {a} idx", eN.sum(axis=others), wN.sum(axis=others)))
    worst, where = 0.0, "-"
    for name, e, n in groups:
        ok = n >= MIN_CLASS
        if ok.any():
            v = np.sqrt(e[ok] / n[ok] / ref_ms)
            i = int(np.argmax(v))
            if float(v[i]) > worst:
                worst, where = float(v[i]), f"{name}{' ' if name.endswith('idx') else '='}{int(np.flatnonzero(ok)[i])}"
    Y = yardstick(oracle, case, route)
    line = (f"{prefix}accuracy {case.name}: route={route.strip()} rel_l2={rel:.3e} worst_class={worst:.3e} [{where}] Y={Y:.3e} "
            f"global={rel / Y:.2f} class={worst / Y:.2f}")
    print(line)
    assert rel <= GLOBAL_FACTOR * Y, line
    assert worst <= CLASS_FACTOR * Y, line
    return line
