"""GPU tier: precision "f16-storage" on the MI355X through the Python host.

Each case runs the f16 plan on binary16 bytes and the f32 plan of the same options on the decoded input, at device batch
sizes.  The f32 output rounded to binary16 (numpy, nearest even) is the bar: conversion routes match it bit for bit, fused
one-launch line routes within 1 binary16 ulp per element; against a float64 numpy transform the norm-relative error stays
at or below 1e-3."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fft():
    import mi355fft
    return mi355fft


@pytest.fixture(scope="module")
def dev(fft):
    d = fft.Device(0)
    yield d
    d.close()


def _bytes_up(fft, dev, a, size=None):
    a = np.ascontiguousarray(a)
    buf = dev.createBuffer({"size": max(size or a.nbytes, 8)})
    dev.queue.writeBuffer(buf, 0, a)
    return buf


def _read(fft, buf, nbytes, offset=0):
    out = np.empty(nbytes, np.uint8)
    fft._chk(fft.lib().mi355fft_buffer_read(buf._h, offset, out.ctypes.data, nbytes))
    return out


def _exec(fft, dev, plan, inp, out, use_graph=False):
    enc = dev.createCommandEncoder()
    plan.exec(enc, {"input": inp, "output": out} if out is not None else {"input": inp})
    dev.queue.submit([enc.finish(use_graph)])
    dev.queue.onSubmittedWorkDone()


def _pad(h):
    return np.concatenate([h, np.zeros(1, np.float16)]) if h.size % 2 else h


def run_pair(fft, dev, opts, x16, out_scalars, out_init16=None, use_graph=False, env32=None):
    """(f16 output, f32 output rounded to binary16, f16 route, launches); env32: planner switches for the f32 plan only"""
    p16 = fft.createPlan(dev, dict(opts, precision="f16-storage"))
    saved = {k: os.environ.get(k) for k in (env32 or {})}
    os.environ.update(env32 or {})
    try:
        p32 = fft.createPlan(dev, opts)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    ob16 = ((out_scalars * 2 + 3) // 4) * 4
    inp16 = _bytes_up(fft, dev, _pad(x16))
    out16 = None if opts.get("inPlace") else (_bytes_up(fft, dev, _pad(out_init16)) if out_init16 is not None else dev.createBuffer({"size": ob16}))
    _exec(fft, dev, p16, inp16, out16, use_graph)
    got = _read(fft, out16 if out16 is not None else inp16, ob16).view(np.float16)[:out_scalars]
    inp32 = _bytes_up(fft, dev, x16.astype(np.float32))
    out32 = None if opts.get("inPlace") else (_bytes_up(fft, dev, out_init16.astype(np.float32)) if out_init16 is not None
                                            else dev.createBuffer({"size": 4 * out_scalars}))
    _exec(fft, dev, p32, inp32, out32)
    want32 = _read(fft, out32 if out32 is not None else inp32, 4 * out_scalars).view(np.float32)
    route, launches = p16.describe()
    for b in (inp16, out16, inp32, out32):
        if b is not None:
            b.destroy()
    p16.destroy()
    p32.destroy()
    with np.errstate(over="ignore"):
        return got, want32.astype(np.float16), route, launches


def _ulps(a, b):
    def key(h):
        u = h.view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(key(a) - key(b)))


def _c(h):
    f = h.astype(np.float64)
    return f[0::2] + 1j * f[1::2]


def _rel(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _scale(norm, inverse, n):
    return 1.0 if norm == "none" else (1.0 / np.sqrt(n) if norm == "unitary" else (1.0 / n if inverse else 1.0))


@pytest.mark.parametrize("n,batch", [(8, 4096), (64, 2048), (256, 1024), (1024, 512), (4096, 128), (8192, 64), (16384, 32)])
@pytest.mark.parametrize("direction", ["forward", "inverse"])
@pytest.mark.parametrize("normalize", ["none", "backward", "unitary"])
def test_c2c_fused(fft, dev, n, batch, direction, normalize):
    rng = np.random.default_rng(n + batch)
    x16 = rng.standard_normal(2 * n * batch).astype(np.float16)
    opts = {"type": "c2c", "shape": [n], "batch": batch, "direction": direction, "normalize": normalize}
    # N = 8192: the f16 launch is the LDS line kernel; its f32 twin is that instance too (the default f32 route is line-reg)
    got, want, route, launches = run_pair(fft, dev, opts, x16, 2 * n * batch, env32={"MI355FFT_LINE32K": "0"} if n == 8192 else None)
    assert launches == 1 and route.split()[-1] == "f16", route
    u = _ulps(got, want)
    assert u.max() <= 1, f"{int((u > 0).sum())} of {u.size} elements differ (max {u.max()} ulp)"
    xc = _c(x16).reshape(batch, n)[:8]
    ref = (np.fft.fft(xc, axis=1) if direction == "forward" else np.fft.ifft(xc, axis=1) * n) * _scale(normalize, direction == "inverse", n)
    assert _rel(_c(got).reshape(batch, n)[:8], ref) <= 1e-3


@pytest.mark.parametrize("n,batch", [(128, 2048), (2048, 256), (8192, 64), (32768, 16)])
def test_r2c_fused(fft, dev, n, batch):
    rng = np.random.default_rng(n)
    x16 = rng.standard_normal(n * batch).astype(np.float16)
    p = n // 2 + 1
    got, want, route, launches = run_pair(fft, dev, {"type": "r2c", "shape": [n], "batch": batch, "direction": "forward"}, x16, 2 * p * batch)
    assert launches == 1 and route.split()[-1] == "f16", route
    assert _ulps(got, want).max() <= 1
    ref = np.fft.rfft(x16.astype(np.float64).reshape(batch, n)[:4], axis=1)
    assert _rel(_c(got).reshape(batch, p)[:4], ref) <= 1e-3


@pytest.mark.parametrize("n,batch", [(256, 1024), (4096, 128), (16384, 32), (32768, 16)])
def test_c2r_fused(fft, dev, n, batch):
    rng = np.random.default_rng(n + 3)
    p = n // 2 + 1
    spec = np.fft.rfft(rng.standard_normal((batch, n)), axis=1) / np.sqrt(n)
    x16 = np.stack([spec.real, spec.imag], -1).reshape(-1).astype(np.float16)
    got, want, route, launches = run_pair(fft, dev, {"type": "c2r", "shape": [n], "batch": batch, "direction": "inverse", "normalize": "backward"},
                                          x16, n * batch)
    assert launches == 1 and route.split()[-1] == "f16", route
    assert _ulps(got, want).max() <= 1
    ref = np.fft.irfft(_c(x16).reshape(batch, p)[:4], n=n, axis=1)
    assert _rel(got.astype(np.float64).reshape(batch, n)[:4], ref) <= 1e-3


def test_c2c_fused_through_graph(fft, dev):
    rng = np.random.default_rng(77)
    n, batch = 1024, 4096
    x16 = rng.standard_normal(2 * n * batch).astype(np.float16)
    got, want, route, _ = run_pair(fft, dev, {"type": "c2c", "shape": [n], "batch": batch, "direction": "inverse"}, x16, 2 * n * batch, use_graph=True)
    assert route.split()[-1] == "f16" and _ulps(got, want).max() <= 1


@pytest.mark.parametrize("opts,cin,cout", [
    ({"type": "c2c", "shape": [1 << 20], "batch": 2, "direction": "forward"}, 4 << 20, 4 << 20),
    ({"type": "c2c", "shape": [1 << 17], "batch": 3, "direction": "inverse", "normalize": "backward"}, 6 << 17, 6 << 17),
    ({"type": "c2c", "shape": [64, 48], "batch": 5, "direction": "forward"}, 2 * 64 * 48 * 5, 2 * 64 * 48 * 5),
    ({"type": "dct2", "shape": [256], "batch": 64, "layout": {"interleavedComplex": False}}, 256 * 64, 256 * 64),
    ({"type": "dst4", "shape": [100], "batch": 7, "layout": {"interleavedComplex": False}}, 700, 700),
    ({"type": "r2c", "shape": [1000], "batch": 3, "direction": "forward"}, 3000, 2 * 501 * 3),
    ({"type": "c2r", "shape": [1 << 18], "batch": 2, "direction": "inverse"}, 2 * ((1 << 17) + 1) * 2, 2 << 18),
    ({"type": "c2c", "shape": [512], "batch": 9, "direction": "forward", "inPlace": True}, 2 * 512 * 9, 2 * 512 * 9),
])
def test_conversion_routes(fft, dev, opts, cin, cout):
    rng = np.random.default_rng(cin)
    x16 = rng.standard_normal(cin).astype(np.float16)
    got, want, route, _ = run_pair(fft, dev, opts, x16, cout)
    assert route.startswith("f16-in") and route.split()[-1] == "f16-out", route
    diff = got.view(np.uint16) != want.view(np.uint16)
    assert not diff.any(), f"{int(diff.sum())} elements differ"
    if opts["type"] == "c2c" and len(opts["shape"]) == 1:
        n = opts["shape"][0]
        xc = _c(x16).reshape(-1, n)[:2]
        ref = np.fft.fft(xc, axis=1) if opts["direction"] == "forward" else np.fft.ifft(xc, axis=1) * n * _scale(opts.get("normalize", "none"), True, n)
        assert _rel(_c(got).reshape(-1, n)[:2], ref) <= 1e-3


def test_ioview_keep_outside(fft, dev):
    rng = np.random.default_rng(9)
    n, batch = 1024, 64
    opts = {"type": "c2c", "shape": [n], "batch": batch, "direction": "forward",
            "ioView": {"input": {"shape": [700], "offset": [100]}, "output": {"shape": [1100], "offset": [-30], "clearOutside": False}}}
    x16 = rng.standard_normal(2 * 700 * batch).astype(np.float16)
    init = (rng.standard_normal(2 * 1100 * batch) * 5).astype(np.float16)
    got, want, route, _ = run_pair(fft, dev, opts, x16, 2 * 1100 * batch, out_init16=init)
    assert route.startswith("f16-in+out"), route
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    g, i = got.reshape(batch, 1100, 2), init.reshape(batch, 1100, 2)
    outside = np.r_[0:30, 1054:1100]
    assert np.array_equal(g[:, outside].view(np.uint16), i[:, outside].view(np.uint16))


def test_edge_values(fft, dev):
    n, batch = 1024, 256
    x16 = np.zeros(2 * n * batch, np.float16)
    x16[0::2] = np.float16(100.0)                      # DC 102400 -> +inf
    x16[1::4] = np.float16(2.0 ** -20)                 # binary16 subnormals in the imaginary parts
    got, want, _, _ = run_pair(fft, dev, {"type": "c2c", "shape": [n], "batch": batch, "direction": "forward"}, x16, 2 * n * batch)
    assert np.isposinf(got.reshape(batch, 2 * n)[:, 0]).all()
    assert _ulps(got, want).max() <= 1


def test_config2_full_size(fft, dev):
    """c2c 1024 x 65536 (config 2) at full size: first, middle and last transform against the f32 plan."""
    n, batch = 1024, 65536
    rng = np.random.default_rng(2)
    x16 = rng.standard_normal(2 * n * batch, dtype=np.float32).astype(np.float16)
    opts = {"type": "c2c", "shape": [n], "batch": batch, "direction": "forward", "normalize": "none"}
    p16, p32 = fft.createPlan(dev, dict(opts, precision="f16-storage")), fft.createPlan(dev, opts)
    route, launches = p16.describe()
    assert launches == 1 and route.split()[-1] == "f16", route
    i16, o16 = _bytes_up(fft, dev, x16), dev.createBuffer({"size": x16.nbytes})
    _exec(fft, dev, p16, i16, o16)
    i16.destroy()
    i32 = _bytes_up(fft, dev, x16.astype(np.float32))
    o32 = dev.createBuffer({"size": 2 * x16.nbytes})
    _exec(fft, dev, p32, i32, o32)
    for t in (0, batch // 2, batch - 1):
        g = _read(fft, o16, 4 * n, 4 * n * t).view(np.float16)
        w = _read(fft, o32, 8 * n, 8 * n * t).view(np.float32).astype(np.float16)
        assert _ulps(g, w).max() <= 1, t
        assert _rel(_c(g), np.fft.fft(_c(x16[2 * n * t:2 * n * (t + 1)]))) <= 1e-3
    for b in (o16, i32, o32):
        b.destroy()
    p16.destroy()
    p32.destroy()


def test_exec_offsets_multiple_of_4(fft, dev):
    n = 256
    rng = np.random.default_rng(4)
    x16 = rng.standard_normal(2 * n).astype(np.float16)
    plan = fft.createPlan(dev, {"type": "c2c", "shape": [n], "direction": "forward", "precision": "f16-storage"})
    inp = _bytes_up(fft, dev, np.concatenate([np.zeros(2, np.float16), x16]))      # input at byte offset 4
    out = dev.createBuffer({"size": 4 * n + 12})
    enc = dev.createCommandEncoder()
    plan.exec(enc, {"input": inp, "output": out, "inputOffsetBytes": 4, "outputOffsetBytes": 12})
    dev.queue.submit([enc.finish()])
    dev.queue.onSubmittedWorkDone()
    got = _read(fft, out, 4 * n, 12).view(np.float16)
    assert _rel(_c(got), np.fft.fft(_c(x16))) <= 1e-3
    enc = dev.createCommandEncoder()
    with pytest.raises(fft.Mi355Error):
        plan.exec(enc, {"input": inp, "output": out, "inputOffsetBytes": 2})
    for b in (inp, out):
        b.destroy()
    plan.destroy()
