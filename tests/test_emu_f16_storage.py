"""CPU tier: precision "f16-storage" (binary16 sides, f32 arithmetic) under host emulation.

Every case runs the f16 plan on binary16 bytes and the f32 plan of the same options on the decoded input; the f32 result
rounded to binary16 by numpy (round to nearest even) is the expected output.  Conversion routes (f32 plan on staging regions)
must match it bit for bit, the fused one-launch line routes within 1 binary16 ulp.  Both are also held against a float64
numpy transform of the decoded input."""
import ctypes

import numpy as np
import pytest

import emu_harness as emu
from mi355fft import _abi
from mi355fft.layout import resolve_plan_options


def _opts(opts):
    return dict({"direction": "inverse" if opts["type"] == "c2r" else "forward"}, **opts)


def _desc(opts):
    r = resolve_plan_options(_opts(opts))
    return _abi.make_desc(r["type"], r["shape"], r["batch"], r["direction"], r["normalize"], r["inPlace"], r["input_layout"], r["output_layout"],
                          r["conv"], r["io_view"], r["zero_pad"], r.get("axes"), r.get("precision", "f32"))


def _run_raw(desc, inp, out_bytes, out_init=None):
    """emu_run_plan on raw byte buffers (binary16 sides): returns (output bytes, route, launches)."""
    inp = np.ascontiguousarray(inp).view(np.uint8).copy()
    out = np.zeros(out_bytes, np.uint8) if out_init is None else np.ascontiguousarray(out_init).view(np.uint8).copy()
    err = ctypes.create_string_buffer(1024)
    route = ctypes.create_string_buffer(1024)
    launches = ctypes.c_int(0)
    outp = None if desc.in_place else out.ctypes.data
    rc = emu.lib().emu_run_plan(ctypes.byref(desc), inp.ctypes.data, inp.nbytes, outp, 0 if desc.in_place else out.nbytes, None, 0, 0, 0,
                                err, 1024, route, 1024, ctypes.byref(launches))
    if rc != 0:
        raise emu.EmuError(rc, err.value.decode())
    return (inp if desc.in_place else out), route.value.decode(), launches.value


def _need(desc, side):
    """Byte extent the plan asks of one side (probed through the harness's size check)."""
    big = np.zeros(1 << 24, np.uint8)
    err = ctypes.create_string_buffer(1024)
    route = ctypes.create_string_buffer(1024)
    launches = ctypes.c_int(0)
    args = (0, big.ctypes.data, big.nbytes) if side == "input" else (big.nbytes, big.ctypes.data, 0)
    rc = emu.lib().emu_run_plan(ctypes.byref(desc), big.ctypes.data, args[0], args[1], args[2], None, 0, 0, 0, err, 1024, route, 1024,
                                ctypes.byref(launches))
    assert rc == (100 if side == "input" else 101), err.value.decode()
    return int(err.value.decode().rsplit(" ", 1)[1])


def _f16(rng, n, scale=1.0):
    return (rng.standard_normal(n) * scale).astype(np.float16)


def _pad4(h):
    return np.concatenate([h, np.zeros(1, np.float16)]) if h.size % 2 else h


def _run_pair(opts, x16, out_scalars, out_init16=None):
    """(f16 plan output as float16 scalars, expected = f32 plan on the decoded input rounded to binary16, route, launches)."""
    d16 = _desc(dict(opts, precision="f16-storage"))
    d32 = _desc(opts)
    init = None if out_init16 is None else _pad4(out_init16)
    got, route, launches = _run_raw(d16, _pad4(x16), ((out_scalars * 2 + 3) // 4) * 4, init)
    got = got.view(np.float16)[:out_scalars]
    ref, _, _ = emu.run_plan(d32, x16.astype(np.float32), out_scalars, out_init=None if out_init16 is None else out_init16.astype(np.float32))
    with np.errstate(over="ignore"):           # values beyond 65504 round to +-inf, as the plan's stores do
        return got, ref[:out_scalars].astype(np.float16), route, launches


def _ulps(a, b):
    """per-element distance in binary16 ulps (sign-magnitude order); NaN == NaN"""
    def key(h):
        u = h.view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    both_nan = np.isnan(a) & np.isnan(b)
    return np.where(both_nan, 0, np.abs(key(a) - key(b)))


def _c(h):
    f = h.astype(np.float64)
    return f[0::2] + 1j * f[1::2]


def _rel(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


def _scale(norm, inverse, n):
    return 1.0 if norm == "none" else (1.0 / np.sqrt(n) if norm == "unitary" else (1.0 / n if inverse else 1.0))


# ---- fused one-launch line routes ------------------------------------------------------------------------------------

C2C_SIZES = [(8, 6), (64, 5), (1024, 3), (4096, 2), (16384, 1)]


@pytest.mark.parametrize("n,batch", C2C_SIZES)
@pytest.mark.parametrize("direction", ["forward", "inverse"])
@pytest.mark.parametrize("normalize", ["none", "backward", "unitary"])
def test_c2c_lines_fused(n, batch, direction, normalize):
    rng = np.random.default_rng(n * 7 + len(direction) + len(normalize))
    x16 = _f16(rng, 2 * n * batch)
    opts = {"type": "c2c", "shape": [n], "batch": batch, "direction": direction, "normalize": normalize}
    got, want, route, launches = _run_pair(opts, x16, 2 * n * batch)
    assert launches == 1 and route.strip().endswith("f16") and "lines[N=" in route, route
    u = _ulps(got, want)
    assert u.max() <= 1, f"{int((u > 0).sum())} elements differ, max {u.max()} ulp"
    xc = _c(x16).reshape(batch, n)
    ref = (np.fft.fft(xc, axis=1) if direction == "forward" else np.fft.ifft(xc, axis=1) * n) * _scale(normalize, direction == "inverse", n)
    assert _rel(_c(got), ref.reshape(-1)) <= 1e-3


@pytest.mark.parametrize("n,batch", [(128, 5), (2048, 2)])
def test_r2c_lines_fused(n, batch):
    rng = np.random.default_rng(n)
    x16 = _f16(rng, n * batch)
    p = n // 2 + 1
    opts = {"type": "r2c", "shape": [n], "batch": batch, "direction": "forward", "normalize": "unitary"}
    got, want, route, launches = _run_pair(opts, x16, 2 * p * batch)
    assert launches == 1 and route.strip().endswith("f16") and "lines-r2c" in route, route
    assert _ulps(got, want).max() <= 1
    ref = np.fft.rfft(x16.astype(np.float64).reshape(batch, n), axis=1) / np.sqrt(n)
    assert _rel(_c(got), ref.reshape(-1)) <= 1e-3


@pytest.mark.parametrize("n,batch", [(256, 4), (4096, 2)])
def test_c2r_lines_fused(n, batch):
    rng = np.random.default_rng(n + 1)
    p = n // 2 + 1
    spec = np.fft.rfft(rng.standard_normal((batch, n)), axis=1)
    x16 = np.stack([spec.real, spec.imag], -1).reshape(-1).astype(np.float16)
    opts = {"type": "c2r", "shape": [n], "batch": batch, "direction": "inverse", "normalize": "backward"}
    got, want, route, launches = _run_pair(opts, x16, n * batch)
    assert launches == 1 and route.strip().endswith("f16") and "lines-c2r" in route, route
    assert _ulps(got, want).max() <= 1
    ref = np.fft.irfft(_c(x16).reshape(batch, p), n=n, axis=1)
    assert _rel(got.astype(np.float64), ref.reshape(-1)) <= 1e-3


# ---- conversion routes ------------------------------------------------------------------------------------------------

def _dct2(x):
    n = x.shape[-1]
    k = np.arange(n)
    return np.cos(np.pi * np.outer(k, 2 * np.arange(n) + 1) / (2 * n)) @ x.T      # unscaled sum (dct_fft.js)


@pytest.mark.parametrize("opts,count_in,count_out,check", [
    ({"type": "dct2", "shape": [256], "batch": 3, "layout": {"interleavedComplex": False}}, 768, 768, "dct2"),
    ({"type": "c2c", "shape": [16, 8], "batch": 2, "direction": "forward"}, 2 * 128 * 2, 2 * 128 * 2, "c2c2d"),
    ({"type": "c2c", "shape": [1 << 17], "batch": 1, "direction": "inverse", "normalize": "backward"}, 2 << 17, 2 << 17, "c2cbig"),
])
def test_conversion_routes(opts, count_in, count_out, check):
    rng = np.random.default_rng(count_in)
    x16 = _f16(rng, count_in)
    got, want, route, launches = _run_pair(opts, x16, count_out)
    _, l32, _ = emu.plan_only(_desc(opts))
    assert route.startswith("f16-in ") and route.strip().endswith("f16-out") and launches == l32 + 2, (route, launches, l32)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), f"{int((got.view(np.uint16) != want.view(np.uint16)).sum())} elements differ"
    if check == "dct2":
        ref = _dct2(x16.astype(np.float64).reshape(3, 256)).T.reshape(-1)
        assert _rel(got.astype(np.float64), ref) <= 1e-3
    elif check == "c2c2d":
        ref = np.fft.fft2(_c(x16).reshape(2, 8, 16)).reshape(-1)
        assert _rel(_c(got), ref) <= 1e-3
    else:
        ref = np.fft.ifft(_c(x16))
        assert _rel(_c(got), ref) <= 1e-3


def test_c2c_in_place_conversion():
    rng = np.random.default_rng(5)
    n, batch = 256, 3
    x16 = _f16(rng, 2 * n * batch)
    opts = {"type": "c2c", "shape": [n], "batch": batch, "direction": "forward", "inPlace": True}
    d16 = _desc(dict(opts, precision="f16-storage"))
    got, route, launches = _run_raw(d16, x16, 0)
    got = got.view(np.float16)
    ref, _, _ = emu.run_plan(_desc(opts), x16.astype(np.float32), 2 * n * batch)
    assert route.startswith("f16-in ") and launches == emu.plan_only(_desc(opts))[1] + 2
    assert np.array_equal(got.view(np.uint16), ref.astype(np.float16).view(np.uint16))
    assert _rel(_c(got), np.fft.fft(_c(x16).reshape(batch, n), axis=1).reshape(-1)) <= 1e-3


def test_ioview_keep_outside_bit_identical():
    """ioView in/out with clearOutside: false: view elements the transform does not reach keep their exact bytes."""
    rng = np.random.default_rng(11)
    n, batch = 64, 2
    opts = {"type": "c2c", "shape": [n], "batch": batch, "direction": "forward",
            "ioView": {"input": {"shape": [40], "offset": [8]}, "output": {"shape": [96], "offset": [-16], "clearOutside": False}}}
    x16 = _f16(rng, 2 * 40 * batch)
    init = _f16(rng, 2 * 96 * batch, 3.0)
    got, want, route, launches = _run_pair(opts, x16, 2 * 96 * batch, out_init16=init)
    assert route.startswith("f16-in+out ") and launches == emu.plan_only(_desc(opts))[1] + 3, route
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    g = got.reshape(batch, 96, 2)
    i = init.reshape(batch, 96, 2)
    outside = np.r_[0:16, 80:96]
    assert np.array_equal(g[:, outside].view(np.uint16), i[:, outside].view(np.uint16))
    logical = np.zeros((batch, n), complex)
    logical[:, 8:48] = _c(x16).reshape(batch, 40)
    ref = np.fft.fft(logical, axis=1)
    assert _rel(_c(g[:, 16:80].reshape(-1)), ref.reshape(-1)) <= 1e-3


def test_zeropad_conversion():
    rng = np.random.default_rng(12)
    n, batch = 128, 2
    opts = {"type": "c2c", "shape": [n], "batch": batch, "direction": "inverse",
            "zeroPad": {"read": {"start": [4], "end": [100]}, "write": {"start": [0], "end": [64]}}}
    x16 = _f16(rng, 2 * n * batch)
    got, want, route, _ = _run_pair(opts, x16, 2 * n * batch)
    assert route.startswith("f16-in ")
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    xc = _c(x16).reshape(batch, n)
    xc[:, :4] = 0
    xc[:, 100:] = 0
    ref = np.fft.ifft(xc, axis=1) * n
    ref[:, 64:] = 0
    assert _rel(_c(got), ref.reshape(-1)) <= 1e-3


# ---- edge values ------------------------------------------------------------------------------------------------------

def test_dc_overflow_to_inf():
    n = 1024
    x16 = np.zeros(2 * n, np.float16)
    x16[0::2] = np.float16(100.0)             # DC = 102400 > 65504
    got, want, _, _ = _run_pair({"type": "c2c", "shape": [n], "direction": "forward"}, x16, 2 * n)
    assert np.isposinf(got[0]) and got[0].view(np.uint16) == want[0].view(np.uint16)
    assert np.all(np.abs(got[2:].astype(np.float32)) <= 1e-2)


def test_subnormal_inputs():
    n = 64
    rng = np.random.default_rng(3)
    x16 = (rng.integers(1, 1024, 2 * n).astype(np.uint16) | (rng.integers(0, 2, 2 * n).astype(np.uint16) << 15)).view(np.float16)
    assert np.all(np.abs(x16.astype(np.float32)) < 6.2e-5)     # every input a binary16 subnormal
    got, want, _, _ = _run_pair({"type": "c2c", "shape": [n], "direction": "forward"}, x16, 2 * n)
    assert _ulps(got, want).max() <= 1
    assert _rel(_c(got), np.fft.fft(_c(x16))) <= 1e-3


# ---- planner ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opts,in_bytes,out_bytes", [
    ({"type": "c2c", "shape": [1024], "batch": 3}, 1024 * 3 * 4, 1024 * 3 * 4),
    ({"type": "r2c", "shape": [2048], "batch": 1}, 2048 * 2, 1025 * 4),
    ({"type": "c2r", "shape": [4096], "batch": 1, "direction": "inverse"}, 2049 * 4, 4096 * 2),
    ({"type": "dct2", "shape": [7], "batch": 1, "layout": {"interleavedComplex": False}}, 16, 16),      # 14 bytes rounded up to 16
    ({"type": "r2c", "shape": [6], "batch": 3, "layout": {"interleavedComplex": True}}, 36, 48),
    ({"type": "c2r", "shape": [9], "batch": 1, "direction": "inverse"}, 20, 20),                          # 18 -> 20
])
def test_extents_halved(opts, in_bytes, out_bytes):
    d = _desc(dict(opts, precision="f16-storage"))
    assert _need(d, "input") == in_bytes
    assert _need(d, "output") == out_bytes


@pytest.mark.parametrize("opts,fused", [
    ({"type": "c2c", "shape": [1024], "batch": 65536}, True),
    ({"type": "c2c", "shape": [8192], "batch": 4}, True),
    ({"type": "c2c", "shape": [16384], "batch": 4, "direction": "inverse"}, True),
    ({"type": "r2c", "shape": [32768], "batch": 4}, True),
    ({"type": "c2r", "shape": [32768], "batch": 4, "direction": "inverse"}, True),
    ({"type": "c2c", "shape": [1 << 20], "batch": 2}, False),
    ({"type": "c2c", "shape": [1000], "batch": 2}, False),
    ({"type": "c2c", "shape": [256, 256], "batch": 1}, False),
    ({"type": "c2c", "shape": [1024], "batch": 2, "ioView": {"output": {"shape": [512], "offset": [256], "clearOutside": False}}}, False),
])
def test_planner_routes(opts, fused):
    d16 = _desc(dict(opts, precision="f16-storage"))
    route, launches, work = emu.plan_only(d16)
    route32, launches32, work32 = emu.plan_only(_desc(opts))
    if fused:
        assert launches == 1 and route.split()[-1] == "f16" and work == work32, route
        assert "line-reg" not in route
    else:
        keep = "ioView" in opts
        assert launches == launches32 + (3 if keep else 2) and route.startswith("f16-in") and route.split()[-1] == "f16-out", route
        assert work > work32


@pytest.mark.parametrize("opts,msg", [
    ({"type": "c2c", "shape": [8], "layout": {"interleavedComplex": True, "strides": [2]}}, 'custom strides currently support precision:"f32" only'),
    ({"type": "r2c", "shape": [8], "layout": {"interleavedComplex": True, "strides": [2]}}, 'custom strides currently support precision:"f32" only for r2c'),
    ({"type": "c2r", "shape": [8], "direction": "inverse", "layout": {"interleavedComplex": True, "strides": [2]}},
     'custom strides currently support precision:"f32" only for c2r'),
    ({"type": "dct2", "shape": [8], "layout": {"interleavedComplex": False, "strides": [2]}}, 'custom strides for dct/dst currently support precision:"f32" only'),
    ({"type": "fftconv", "shape": [8]}, 'fftconv supports precision:"f32" only in current implementation'),
])
def test_rejections_host(opts, msg):
    with pytest.raises(ValueError) as e:
        resolve_plan_options(_opts(dict(opts, precision="f16-storage")))
    assert str(e.value) == msg


@pytest.mark.parametrize("typ,msg", [
    (_abi.C2C, 'custom strides currently support precision:"f32" only'),
    (_abi.R2C, 'custom strides currently support precision:"f32" only for r2c'),
    (_abi.C2R, 'custom strides currently support precision:"f32" only for c2r'),
    (_abi.TYPE["dst3"], 'custom strides for dct/dst currently support precision:"f32" only'),
])
def test_rejections_abi(typ, msg):
    d = _abi.make_desc(typ, [8], 1, "inverse" if typ == _abi.C2R else "forward", "none", input_layout={"strides": [1]}, precision="f16-storage")
    with pytest.raises(emu.EmuError) as e:
        emu.plan_only(d)
    assert e.value.code == _abi.ERR_INVALID and str(e.value) == msg


def test_fftconv_rejected_abi():
    d = _abi.make_desc("fftconv", [8], 1, conv={}, precision="f16-storage")
    with pytest.raises(emu.EmuError) as e:
        emu.plan_only(d)
    assert e.value.code == _abi.ERR_INVALID and "fftconv supports precision" in str(e.value)


def test_unknown_precision_rejected_abi():
    d = _abi.make_desc("c2c", [8], 1)
    d.precision = 7
    with pytest.raises(emu.EmuError) as e:
        emu.plan_only(d)
    assert e.value.code == _abi.ERR_INVALID and "precision" in str(e.value)


def test_host_accepts_f16_storage():
    r = resolve_plan_options({"type": "c2c", "shape": [64], "direction": "forward", "precision": "f16-storage"})
    assert r["precision"] == "f16-storage"
    assert _desc({"type": "c2c", "shape": [64], "precision": "f16-storage"}).precision == _abi.PRECISION["f16-storage"] == 1


def test_abi_field_changes_extents_and_route():
    d = _abi.make_desc("c2c", [1024], 4)
    d.precision = 1
    route, launches, _ = emu.plan_only(d)
    assert route.split()[-1] == "f16" and launches == 1
    assert _need(d, "input") == 1024 * 4 * 4
