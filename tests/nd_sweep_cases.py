"""Shared by test_emu_nd_sweep.py and test_gpu_nd_sweep.py: the float64 bar of accuracy_cases.py (rel_l2 <= 4 Y, every class <= 8 Y, the
per-axis index classes of rank > 1 among them) on everything that runs on a strided axis and on the request space around the kernels.

TABLE   one ACase per strided-axis kernel instance and per shape at which the planner takes another route for the higher axes: every
        LINE_PASS_A and LINE_COL_RAGGED size of line_kernels.def as a c2c column axis (test_emu_nd_sweep.test_every_column_instance_has_a_case
        reads the list), the stage / mixed-radix / Bluestein forms of a strided axis, unit axes, N-D r2c, c2r and all eight DCT / DST types.
        Every case pins the route fragment of its strided axes; both tiers plan them alike.
draw()  three seeded families of requests, one per integer seed, every seed plannable:
          V  c2c with ioView.input / .output (shapes within +-50 % of the logical one, offsets mostly within +-3, else anywhere the window
             still covers half the axis; clearOutside either way), zeroPad.read / .write boxes, FUSE_VIEWS 0 or 1
          S  c2c with a permuted, padded stride order on either or both sides, offsets, batch strides with slack, sometimes zeroPad.read;
             the physical input holds 9.0 off the lanes
          P  c2c out of place and in place, r2c, c2r and the eight DCT / DST types, dense
        Axis lengths come from DIMS with 1024 <= prod(shape) <= 16384.  On every axis the window a side reads or writes (view, domain and
        zeroPad box together) keeps at least half of the axis, so a request writes at least 256 non-zero reals.
check() per request: untouched output elements keep their NaN, the elements the reference holds as exact zeros (outside zeroPad.write,
        clearOutside) are exactly zero, the rest is finite and held to accuracy_cases.measure on the dense request."""
import numpy as np

import accuracy_cases as acc
from accuracy_cases import DIRECTIONS, ACase, _in_c2c, _in_real, _in_spectrum, _ragged_batch
from exec_contract_cases import FUSED, REAL, _o

TRIG_TYPES = ("dct1", "dct2", "dct3", "dct4", "dst1", "dst2", "dst3", "dst4")

# ---- the instance table ---------------------------------------------------------------------------------------------------------------
TABLE = []


def _lg(n):
    return int(n).bit_length() - 1


def _add(name, opts, route, make, **kw):
    """batch: at least the one given, odd, and large enough that the index classes of the output's longest axis hold MIN_CLASS reals
    (accuracy_cases.measure leaves smaller classes out: a lost digit at one index of that axis would go unseen)"""
    oshape = acc._out_shape(opts)
    need = -(-acc.MIN_CLASS * max(oshape) // ((2 if opts["type"] in ("c2c", "r2c") else 1) * int(np.prod(oshape))))
    opts["batch"] = max(opts["batch"], need) | 1
    TABLE.append(ACase(name, opts, route, make, starts=False, emu=acc._emu(opts), **kw))


def _name(shape):
    return "x".join(str(s) for s in shape)


_C2C = (
    # columns[N=...]: every LINE_PASS_A size at S = T, the smallest width that takes it; batches that leave a ragged last workgroup (and see _add)
    [([64, n], f"columns[N={n},S=64]", _ragged_batch(_lg(n))) for n in (2, 4, 8, 16, 32)]
    + [([16, n], f"columns[N={n},S=16]", _ragged_batch(_lg(n))) for n in (64, 128, 256, 512, 1024)]
    + [([8, 2048], "columns[N=2048,S=8]", _ragged_batch(11))]
    # ... at other widths and behind the other kinds of lower axes
    + [([16, 2048], "columns[N=2048,S=16]", 3),
       ([40, 2048], ("mixed-lines[N=40,", "columns[N=2048,S=40]"), 3),
       ([128, 2, 128], ("columns[N=2,S=128]", "columns[N=128,S=256]"), 3),
       ([16, 16, 16], ("mixed-lines[N=16,S=16,", "columns[N=16,S=256]"), 3),
       ([16, 4, 64], ("stages[N=4,S=16,", "columns[N=64,S=64]"), 3)]
    # columns-ragged[N=...]: every LINE_COL_RAGGED size below a c2c axis 0 that is no multiple of the tile (S = T + 8, and others)
    + [([24, n], f"columns-ragged[N={n},S=24]", 3) for n in (64, 128, 256, 512, 1024)]
    + [([17, 256], ("bluestein-lines[N=17,", "columns-ragged[N=256,S=17]"), 3),
       ([33, 1024], "columns-ragged[N=1024,S=33]", 3),
       ([1000, 1024], ("mixed-ct[N=1000,", "columns-ragged[N=1024,S=1000]"), 1)]
    # widths below the tile that have no ragged instance, and the strided axes that are no column kernel at all
    + [([4, 2048], "stages[N=2048,S=4,", 3),
       ([5, 1024], "stages[N=1024,S=5,", 3),
       ([2, 2, 2048], ("stages[N=2,S=2,", "stages[N=2048,S=4,"), 3),
       ([3, 64], "mixed-lines[N=64,S=3,", 5),
       ([64, 100], "mixed-lines[N=100,S=64,", 3),
       ([32, 3000], "stages[N=3000,S=32,", 1),
       ([64, 4096], "stages[N=4096,S=64,", 1),
       ([64, 17], "bluestein[N=17,", 3),
       ([1, 512], "lines[N=512]", 3),
       ([512, 1, 4], "columns[N=4,S=512]", 3)]
)
for _i, (_shape, _tag, _b) in enumerate(_C2C):
    for _d, _nm in DIRECTIONS:
        _add(f"nd_c2c_{_name(_shape)}_{_d}", _o("c2c", _shape, _b, _d, _nm), _tag, _in_c2c(0xAD000 + _i))
for _d, _nm in DIRECTIONS:      # the ladder has the 256 and 512 planes
    _add(f"nd_xcd_2d_1024x1024_{_d}", _o("c2c", [1024, 1024], 1, _d, _nm), "xcd-2d[1024x1024]", _in_c2c(0xAD0F0), env={"XCD_2D": "1"}, emu_env=FUSED)

_REAL = (([256, 256], "columns-ragged[N=256,S=129]"), ([30, 64], "columns[N=64,S=16]"), ([6, 2048], "stages[N=2048,S=4,"),
         ([62, 512], "columns[N=512,S=32]"), ([2, 1024], "stages[N=1024,S=2,"), ([128, 6], "mixed-lines[N=6,S=65,"),
         ([9, 64], "mixed-lines[N=64,S=5,"),
         # c2r only
         ([64, 64, 8], ("columns-ragged[N=64,S=33]", "columns[N=8,S=2112]")), ([2048, 8], "stages[N=8,S=1025,"), ([16, 2048], "stages[N=2048,S=9,"))
for _i, (_shape, _tag) in enumerate(_REAL):
    if _i < 7:
        _add(f"nd_r2c_{_name(_shape)}", _o("r2c", _shape, 3), _tag, _in_real(0xAD100 + _i))
    _add(f"nd_c2r_{_name(_shape)}", _o("c2r", _shape, 3, "inverse", "backward"), _tag, _in_spectrum(0xAD140 + _i))

# DCT / DST: all eight types, the directions alternating over the shapes (every kind of oracle.trig_kind occurs)
for _t, _typ in enumerate(TRIG_TYPES):
    for _i, _shape in enumerate(([32, 24], [64, 64, 3], [17, 256], [256, 17])):
        _d, _nm = DIRECTIONS[(_i + _t) % 2]
        _add(f"nd_{_typ}_{_name(_shape)}_{_d}", _o(_typ, _shape, 3, _d, _nm, layout=dict(REAL)), "kind=", _in_real(0xAD200 + 8 * _t + _i))

BY_NAME = {c.name: c for c in TABLE}
assert len(BY_NAME) == len(TABLE) and not set(BY_NAME) & set(acc.BY_NAME)

# ---- the seeded sweep -----------------------------------------------------------------------------------------------------------------
DIMS = (1, 2, 3, 4, 5, 8, 12, 16, 17, 24, 32, 60, 64, 100, 128, 256, 1024)
MIN_POINTS, MAX_POINTS = 1024, 16384
SEEDS = {"V": 200, "S": 200, "P": 100}
BASE = {"V": 0x5EED1000, "S": 0x5EED2000, "P": 0x5EED3000}
P_KINDS = ("c2c", "c2c-in-place", "r2c", "c2r") + TRIG_TYPES


class Draw:
    """one request of the sweep: plan options, the FUSE_VIEWS setting of both tiers, and the seed of its input"""

    def __init__(self, family, seed, opts, env):
        self.family, self.seed, self.opts, self.env = family, seed, opts, env
        self.case = ACase(f"{family}{seed:03d}", opts, "", None, env=env, starts=False)
        self.prefix = f"sweep {family} seed={seed} "

    def __repr__(self):
        return self.case.name


def _shape(rng, least=(1, 1, 1)):
    """rank 1 - 3, lengths from DIMS (axis d at least least[d]), MIN_POINTS <= prod <= MAX_POINTS"""
    while True:
        rank = int(rng.integers(1, 4))
        shape = [int(rng.choice(DIMS)) for _ in range(rank)]
        if MIN_POINTS <= int(np.prod(shape)) <= MAX_POINTS and all(s >= m for s, m in zip(shape, least)):
            return shape


def _view_axis(rng, L):
    """(view length, offset, window) on an axis of L points: the length within +-50 %, the window [a, b) of logical indices the view
    covers at least (L + 1) // 2 long; view index v is logical index v + offset"""
    need = (L + 1) // 2
    V = int(rng.integers(need, max(need, (3 * L) // 2) + 1))
    lo, hi = need - V, L - need          # the offsets that leave `need` indices of the domain under the view
    near = rng.random() < 0.8
    off = int(np.clip(rng.integers(-3, 4), lo, hi)) if near else int(rng.integers(lo, hi + 1))
    return V, off, (max(0, off), min(L, off + V))


def _box_axis(rng, L, window):
    """a zeroPad range [s, e) of an axis that keeps at least (L + 1) // 2 indices of `window`"""
    a, b = window
    c = int(rng.integers((L + 1) // 2, b - a + 1))
    cs = int(rng.integers(a, b - c + 1))
    return int(rng.integers(0, cs + 1)), int(rng.integers(cs + c, L + 1))


def _side(rng, shape, view, box, clear=None):
    """(ioView side or None, zeroPad stage or None) of one side"""
    windows, v = [(0, L) for L in shape], None
    if view:
        axes = [_view_axis(rng, L) for L in shape]
        v = {"shape": [a[0] for a in axes], "offset": [a[1] for a in axes]}
        if clear is not None:
            v["clearOutside"] = clear
        windows = [a[2] for a in axes]
    z = None
    if box:
        ranges = [_box_axis(rng, L, w) for L, w in zip(shape, windows)]
        z = {"start": [r[0] for r in ranges], "end": [r[1] for r in ranges]}
    return v, z


def _direction(rng):
    return str(rng.choice(["forward", "inverse"])), str(rng.choice(["none", "backward", "unitary"]))


def _strides(rng, shape):
    """a side's layout: the axes nested in a random order, padding between them, a non-unit innermost stride now and then"""
    acc_, strides = int(rng.choice([1, 1, 1, 2, 3])), [0] * len(shape)
    for a in rng.permutation(len(shape)):
        strides[int(a)] = acc_
        acc_ = acc_ * shape[int(a)] + int(rng.integers(0, 4))
    span = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
    return {"strides": strides, "offset": int(rng.integers(0, 5)), "batch_stride": span + int(rng.integers(0, 8))}


def draw(family, seed):
    """the request of `seed` in `family`: a pure function of both"""
    rng = np.random.default_rng(BASE[family] + seed)
    batch = int(rng.integers(1, 4))
    env = {"FUSE_VIEWS": str(int(rng.integers(0, 2)))}
    if family == "V":
        shape = _shape(rng)
        direction, normalize = _direction(rng)
        flags = [rng.random() < p for p in (0.6, 0.6, 0.4, 0.4)]          # ioView.input, .output, zeroPad.read, .write
        if not any(flags):
            flags[int(rng.integers(0, 4))] = True
        vin, zr = _side(rng, shape, flags[0], flags[2])
        vout, zw = _side(rng, shape, flags[1], flags[3], clear=bool(rng.integers(0, 2)))
        opts = _o("c2c", shape, batch, direction, normalize)
        if vin or vout:
            opts["ioView"] = {k: v for k, v in (("input", vin), ("output", vout)) if v}
        if zr or zw:
            opts["zeroPad"] = {k: v for k, v in (("read", zr), ("write", zw)) if v}
        return Draw(family, seed, opts, env)
    if family == "S":
        shape = _shape(rng)
        direction, normalize = _direction(rng)
        sides = ("input", "output", "both")[int(rng.integers(0, 3))]
        layout = {"interleavedComplex": True}
        for side in ("input", "output"):
            if sides in (side, "both"):
                lay = _strides(rng, shape)
                layout.update({side + "Strides": lay["strides"], side + "OffsetElements": lay["offset"], side + "BatchStrideElements": lay["batch_stride"]})
        opts = _o("c2c", shape, batch, direction, normalize, layout=layout)
        if rng.random() < 0.3:
            opts["zeroPad"] = {"read": _side(rng, shape, False, True)[1]}
        return Draw(family, seed, opts, env)
    assert family == "P"
    kind = P_KINDS[seed % len(P_KINDS)]
    direction, normalize = _direction(rng)
    if kind in TRIG_TYPES:
        return Draw(family, seed, _o(kind, _shape(rng, (2, 2, 2)), batch, direction, normalize, layout=dict(REAL)), env)
    if kind in ("r2c", "c2r"):
        return Draw(family, seed, _o(kind, _shape(rng, (2, 1, 1)), batch, "forward" if kind == "r2c" else "inverse", normalize), env)
    opts = _o("c2c", _shape(rng), batch, direction, normalize)
    if kind == "c2c-in-place":
        opts["inPlace"] = True
    return Draw(family, seed, opts, env)


# ---- inputs, references and checks of a draw -----------------------------------------------------------------------------------------
def _side_index(lay, shape, batch):
    """the physical element of every (batch item, logical element) of a strided side, in dense order (axis 0 fastest)"""
    idx = lay["offset"] + lay["batch_stride"] * np.arange(batch, dtype=np.int64)
    for d in reversed(range(len(shape))):
        idx = idx[..., None] + lay["strides"][d] * np.arange(shape[d], dtype=np.int64)
    return idx.reshape(-1)


def _extent(lay, shape, batch):
    return lay["offset"] + (batch - 1) * lay["batch_stride"] + sum((s - 1) * st for s, st in zip(shape, lay["strides"])) + 1


class Data:
    """x: the physical input; init: what the output buffer holds before the run (None: anything); want / keep: the float64 reference in
    the physical output layout and the elements the contract leaves alone; dense: (indices of the dense output in the physical one, dense
    reference, dense keep) of a strided output"""


def data(oracle, d):
    from mi355fft.layout import resolve_plan_options
    o, r = d.opts, resolve_plan_options(d.opts)
    typ, shape, batch = o["type"], o["shape"], o["batch"]
    packed = [shape[0] // 2 + 1] + list(shape[1:])
    vin = r["io_view"]["input"]
    in_shape = vin["shape"] if vin else packed if typ == "c2r" else shape
    seed = BASE[d.family] + d.seed
    if typ == "c2c":
        x = oracle.random_complex_batch(int(np.prod(in_shape)), batch, seed).reshape(-1)
    elif typ == "c2r":
        x = _in_spectrum(seed)(oracle, o)[0]
    else:
        x = oracle.random_real_batch(int(np.prod(in_shape)), batch, seed).reshape(-1)
    x = np.ascontiguousarray(x, np.float32)
    want = np.asarray(acc.exact(oracle, d.case, x, None), np.float64).reshape(-1)
    keep = np.isnan(want)
    out = Data()
    out.dense_want, out.dense_keep, out.index = want, keep, None
    li, lo = r["input_layout"], r["output_layout"]
    if li:      # 9.0 wherever no lane lies
        phys = np.full((_extent(li, in_shape, batch), 2), 9.0, np.float32)
        phys[_side_index(li, in_shape, batch)] = x.reshape(-1, 2)
        x = phys.reshape(-1)
    if lo:
        out.index = _side_index(lo, shape, batch)
        w2 = np.full((_extent(lo, shape, batch), 2), np.nan)
        w2[out.index] = want.reshape(-1, 2)
        want = w2.reshape(-1)
        keep = np.isnan(want)
    out.x, out.want, out.keep = x, want, keep
    out.init = np.full(want.size, np.nan, np.float32) if keep.any() else None
    out.zeros = (want == 0.0) if (o.get("ioView") or o.get("zeroPad")) else None
    return out


def check(oracle, d, route, got, dat):
    """every per-request check on the physical output `got`; returns the log line"""
    what = f"{d.prefix}{d.opts} ({route.strip()})"
    got = np.asarray(got, np.float32)[:dat.want.size]
    assert np.isnan(got[dat.keep]).all(), f"{what}: {int(np.count_nonzero(~np.isnan(got[dat.keep])))} elements outside the plan's stores were written"
    assert np.isfinite(got[~dat.keep]).all(), f"{what}: the output is not finite"
    if dat.zeros is not None:
        bad = dat.zeros & (got != 0.0)
        assert not bad.any(), f"{what}: {int(np.count_nonzero(bad))} elements outside zeroPad.write / under clearOutside are not exactly zero"
    dense = got if dat.index is None else got.reshape(-1, 2)[dat.index].reshape(-1)
    return acc.measure(oracle, d.case, route, dense, dat.dense_want, dat.dense_keep, prefix=d.prefix)
