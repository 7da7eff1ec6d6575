"""CPU tier: fftconv over real data (type "fftconv" with layout.interleavedComplex false -> MI355FFT_FFTCONV_REAL).

Host logic, then the three planner routes under host emulation:
  lines-rconv[N=P]  r2c, product and c2r of a real line in one launch per kernel (kern_lines.hpp fft_lines_rconv_kernel), 1 + K launches
  rconv[K]          composed from the real emitters (also through the switch MI355_EMU_RCONV_FUSED=0 / MI355FFT_RCONV_FUSED=0)
  rconv-widened     circular lines of odd length: the complex plan between a widening and a narrowing pass
Reference values are numpy float64 (FFT on the exact logical length, or a direct sum) computed here; the bars are the project's own for
complex fftconv (test_emu_fftconv_linear.py): elementwise 4e-3 / 4e-3 and rel_l2 < 1e-5 against float64, rel_l2 < 1e-6 between routes
and against the complex plan run on the same data with zero imaginary parts."""
import numpy as np
import pytest

import emu_harness as emu
from mi355fft import _abi
from mi355fft.layout import (createFftConvChannelLanePreset, resolve_plan_options)
from test_emu_fftconv import _close

REAL = {"interleavedComplex": False}
FORBIDDEN = ("gather", "scatter", "zero", "bluestein", "stages", "mixed")


def _desc(opts):
    r = resolve_plan_options(opts)
    return _abi.make_desc(r.get("abi_type", r["type"]), r["shape"], r["batch"], r["direction"], r["normalize"], r["inPlace"], r["input_layout"],
                          r["output_layout"], r["conv"], None, r["zero_pad"]), r


def _opts(shape, kshape, batch, K=1, mode="convolution", boundary="circular", out_layout="kernel-major", zero_pad=None, layout=None, **fc):
    o = {"type": "fftconv", "shape": list(shape), "batch": batch, "layout": dict(REAL, **(layout or {})),
         "fftConv": dict({"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": list(kshape), "outputLayout": out_layout}, **fc)}
    if zero_pad:
        o["zeroPad"] = zero_pad
    return o


def _rand(n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(np.float32)


def _geometry(shape, kshape, boundary):
    """FFT domain, output shape and crop offset per axis (axis 0 first)"""
    if boundary == "circular":
        return list(shape), list(shape), [0] * len(shape)
    fs = [s + k - 1 for s, k in zip(shape, kshape)]
    if boundary == "linear-full":
        return fs, fs, [0] * len(shape)
    if boundary == "linear-same":
        return fs, list(shape), [(k - 1) // 2 for k in kshape]
    return fs, [s - k + 1 for s, k in zip(shape, kshape)], [k - 1 for k in kshape]


def _want(x, h, shape, kshape, batch, K, mode, boundary, zero_pad=None):
    """float64 reference, kernel-major [K][batch][out]: irfft(rfft(x, fs) * rfft(h, fs)) on the exact logical FFT domain (numpy axis order is
    reversed: axis 0 of the plan is the fastest)"""
    fs, os_, off = _geometry(shape, kshape, boundary)
    rs, rk, rf = shape[::-1], kshape[::-1], fs[::-1]
    xs = x.astype(np.float64).reshape([batch] + rs)
    hs = h.astype(np.float64).reshape([K] + rk)
    axes = tuple(range(1, len(shape) + 1))
    xp = np.zeros([batch] + rf)
    xp[(slice(None),) + tuple(slice(0, s) for s in rs)] = xs
    if zero_pad and zero_pad.get("read"):
        m = np.zeros(rf)
        m[tuple(slice(a, b) for a, b in zip(zero_pad["read"]["start"][::-1], zero_pad["read"]["end"][::-1]))] = 1.0
        xp = xp * m
    hp = np.zeros([K] + rf)
    hp[(slice(None),) + tuple(slice(0, s) for s in rk)] = hs
    X, G = np.fft.fftn(xp, axes=axes), np.fft.fftn(hp, axes=axes)
    if mode == "correlation":
        G = np.conj(G)
    out = []
    for k in range(K):
        y = np.fft.ifftn(X * G[k], axes=axes).real
        if zero_pad and zero_pad.get("write"):
            m = np.zeros(rf)
            m[tuple(slice(a, b) for a, b in zip(zero_pad["write"]["start"][::-1], zero_pad["write"]["end"][::-1]))] = 1.0
            y = y * m
        out.append(y[(slice(None),) + tuple(slice(o, o + n) for o, n in zip(off[::-1], os_[::-1]))])
    return np.stack(out)


def _kernel_major(got, batch, K, on, out_layout):
    g = np.asarray(got, dtype=np.float64)
    if out_layout == "kernel-major":
        return g.reshape(K, batch, on)
    return g.reshape(batch, K, on).transpose(1, 0, 2)


def _run(opts, x, h):
    desc, r = _desc(opts)
    on = int(np.prod(r["outputShape"]))
    K = r["conv"]["kernelCount"]
    got, route, launches = emu.run_plan(desc, x, on * r["batch"] * K, kernel=h)
    return got, route, launches, r


def _run_complex(opts, x, h):
    """the complex plan on the same data with zero imaginary parts, real parts of its result"""
    o = dict(opts, layout={"interleavedComplex": True})
    r = resolve_plan_options(o)
    desc = _abi.make_desc(r["type"], r["shape"], r["batch"], r["direction"], r["normalize"], r["inPlace"], r["input_layout"], r["output_layout"],
                          r["conv"], None, r["zero_pad"])
    xc = np.zeros(2 * x.size, np.float32); xc[0::2] = x
    hc = np.zeros(2 * h.size, np.float32); hc[0::2] = h
    on = int(np.prod(r["outputShape"]))
    got, route, _ = emu.run_plan(desc, xc, 2 * on * r["batch"] * r["conv"]["kernelCount"], kernel=hc)
    return got[0::2].copy(), route


def check_against_f64(a, e, what):
    """the bar of the real fftconv routes against float64 (shared with exec_contract_cases.py)"""
    a, e = np.asarray(a, np.float64), np.asarray(e, np.float64)
    l2 = float(np.linalg.norm(a - e) / np.linalg.norm(e))
    print(f"{what}: rel_l2={l2:.3e} max_abs={np.abs(a - e).max():.3e}")
    _close(a.astype(np.float32), e.astype(np.float32), 4e-3, 4e-3, what)
    assert l2 < 1e-5, what


def _check(oracle, got, want, batch, K, out_layout, route):
    on = want.shape[-1] if want.ndim == 3 else int(np.prod(want.shape[2:]))
    g = _kernel_major(got, batch, K, on, out_layout)
    w = want.reshape(K, batch, on)
    for k in range(K):
        check_against_f64(g[k].reshape(-1), w[k].reshape(-1), f"{route.strip()} kernel {k}")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---- host logic ----------------------------------------------------------------------------------------------------------------

def test_host_accepts_the_real_plan():
    desc, r = _desc(_opts([1000], [31], 3, K=2, boundary="linear-full"))
    assert desc.type == 12 == _abi.FFTCONV_REAL
    assert r["type"] == "fftconv" and r["real"] is True
    assert r["outputShape"] == [1030]
    assert (r["inputBytes"], r["kernelBytes"], r["outputBytes"]) == (4 * 3 * 1000, 4 * 2 * 31, 4 * 3 * 2 * 1030)
    assert desc.conv_kernel_count == 2 and desc.conv_boundary == 1 and list(desc.conv_kernel_shape)[:1] == [31]
    # the complex plan is what it was
    dc = resolve_plan_options({"type": "fftconv", "shape": [8], "layout": {"interleavedComplex": True}})
    assert "abi_type" not in dc and "real" not in dc


@pytest.mark.parametrize("extra,msg", [
    ({"inPlace": True}, "fftconv inPlace=true is not supported in current implementation"),
    ({"ioView": {"input": {"shape": [4], "offset": [0]}}}, "ioView is not an fftconv option"),
    ({"precision": "f16-storage"}, 'fftconv supports precision:"f32" only in current implementation'),
])
def test_host_rejections_keep_their_messages(extra, msg):
    with pytest.raises(ValueError) as e:
        resolve_plan_options(dict(_opts([8], [8], 1), **extra))
    assert msg in str(e.value)


def test_presets_keep_requiring_complex_layout():
    base = {"shape": [8], "batch": 2, "kernelCount": 2, "input": {"channels": 2}, "output": {"channels": 2}}
    preset = createFftConvChannelLanePreset(base)
    assert preset["layout"]["interleavedComplex"] is True
    with pytest.raises(ValueError) as e:
        createFftConvChannelLanePreset(dict(base, layout={"interleavedComplex": False}))
    assert "layout.interleavedComplex must be true for fftconv channel-lane presets" in str(e.value)


def test_planner_rejections_keep_their_messages():
    desc, _ = _desc(_opts([256], [256], 2))
    desc.in_place = 1
    with pytest.raises(emu.EmuError) as e:
        emu.plan_only(desc)
    assert "fftconv inPlace=true is not supported in current implementation" in str(e.value)
    desc, _ = _desc(_opts([256], [256], 2))
    desc.precision = 1
    with pytest.raises(emu.EmuError) as e:
        emu.plan_only(desc)
    assert 'fftconv supports precision:"f32" only in current implementation' in str(e.value)
    desc, _ = _desc(_opts([256], [256], 2))
    desc.io_input.enabled = 1
    with pytest.raises(emu.EmuError) as e:
        emu.plan_only(desc)
    assert "ioView is not an fftconv option" in str(e.value)


# ---- route 1 -------------------------------------------------------------------------------------------------------------------

def _route1(route, launches, K, P, fn=None):
    assert f"lines-rconv[N={P}]" in route, route
    assert launches == 1 + K, (route, launches)
    assert not [w for w in FORBIDDEN if w in route], route
    if fn is not None and fn != P:
        assert f"pad[{fn}->{P}]" in route, route
    else:
        assert "pad[" not in route, route


@pytest.mark.parametrize("P,batch", [(128, 70), (1024, 9), (4096, 3), (32768, 2)])
@pytest.mark.parametrize("mode", ["convolution", "correlation"])
def test_route1_circular(oracle, monkeypatch, P, batch, mode):
    """batch 70 at P = 128 (32 lines a tile) and 9 at 1024 (8 a tile): ragged last tiles"""
    if P > 8192:
        monkeypatch.setenv("MI355_EMU_RCONV_FUSED", "2")      # above 8192 the planner's default is rconv[K]: the line route through the switch
    ks = [P] if P <= 1024 else [P // 3]
    x, h = _rand(P * batch, 0x51 + P), _rand(ks[0], 0x52 + P)
    opts = _opts([P], ks, batch, mode=mode)
    got, route, launches, _ = _run(opts, x, h)
    _route1(route, launches, 1, P)
    _check(oracle, got, _want(x, h, [P], ks, batch, 1, mode, "circular"), batch, 1, "kernel-major", route)
    ref, croute = _run_complex(opts, x, h)
    assert _rel(got, ref) < 1e-6, (route, croute)


@pytest.mark.parametrize("n,kn,boundary,mode,batch", [
    (1000, 31, "linear-full", "convolution", 5),       # pad[1030->2048]
    (1000, 31, "linear-same", "correlation", 5),       # the crop straddles split: lags -15..-1 from the top of the padded domain
    (1000, 31, "linear-valid", "convolution", 3),
    (1000, 31, "linear-full", "correlation", 3),
    (20000, 5000, "linear-full", "convolution", 2),    # pad[24999->32768]
    (20000, 5000, "linear-same", "correlation", 1),
    (97, 20, "linear-full", "convolution", 3),         # below the shortest line: pad[116->128]
])
def test_route1_linear_padded(oracle, monkeypatch, n, kn, boundary, mode, batch):
    if n + kn - 1 > 8192:
        monkeypatch.setenv("MI355_EMU_RCONV_FUSED", "2")
    x, h = _rand(n * batch, 0x61 + n), _rand(kn, 0x62 + kn)
    opts = _opts([n], [kn], batch, mode=mode, boundary=boundary)
    got, route, launches, _ = _run(opts, x, h)
    fn = n + kn - 1
    P = max(128, 1 << (fn - 1).bit_length())
    _route1(route, launches, 1, P, fn)
    _check(oracle, got, _want(x, h, [n], [kn], batch, 1, mode, boundary), batch, 1, "kernel-major", route)
    if n <= 1000:
        ref, croute = _run_complex(opts, x, h)
        assert _rel(got, ref) < 1e-6, (route, croute)


def test_route1_linear_same_matches_direct_sum(oracle):
    """an independent reference: the correlation as a direct sum in float64"""
    n, kn, batch = 300, 17, 2
    x, h = _rand(n * batch, 0x71), _rand(kn, 0x72)
    got, route, launches, _ = _run(_opts([n], [kn], batch, mode="correlation", boundary="linear-same"), x, h)
    _route1(route, launches, 1, 512, n + kn - 1)
    xs = x.astype(np.float64).reshape(batch, n)
    full = np.zeros((batch, n + kn - 1))         # logical index m: lag m for m < n, lag m - (n + kn - 1) above
    for b in range(batch):
        for lag in range(-(kn - 1), n):
            m = lag if lag >= 0 else lag + n + kn - 1
            full[b, m] = sum(xs[b, j + lag] * float(h[j]) for j in range(kn) if 0 <= j + lag < n)
    off = (kn - 1) // 2
    _check(oracle, got, full[None, :, off:off + n], batch, 1, "kernel-major", route)


@pytest.mark.parametrize("out_layout", ["kernel-major", "batch-major"])
def test_route1_three_kernels(oracle, out_layout):
    n, kn, batch, K = 500, 13, 11, 3
    x, h = _rand(n * batch, 0x81), _rand(kn * K, 0x82)
    opts = _opts([n], [kn], batch, K=K, boundary="linear-full", out_layout=out_layout)
    got, route, launches, _ = _run(opts, x, h)
    _route1(route, launches, K, 512)
    _check(oracle, got, _want(x, h, [n], [kn], batch, K, "convolution", "linear-full"), batch, K, out_layout, route)
    ref, croute = _run_complex(opts, x, h)
    assert _rel(got, ref) < 1e-6, (route, croute)


@pytest.mark.parametrize("boundary,n,kn", [("circular", 1024, 100), ("linear-full", 1000, 31)])
def test_route1_zero_pad_read_and_write(oracle, boundary, n, kn):
    batch = 4
    fn = n if boundary == "circular" else n + kn - 1
    zp = {"read": {"start": [7], "end": [n - 100]}, "write": {"start": [20], "end": [fn - 33]}}
    x, h = _rand(n * batch, 0x91), _rand(kn, 0x92)
    opts = _opts([n], [kn], batch, mode="correlation", boundary=boundary, zero_pad=zp)
    got, route, launches, _ = _run(opts, x, h)
    _route1(route, launches, 1, 1024 if boundary == "circular" else 2048, fn)
    _check(oracle, got, _want(x, h, [n], [kn], batch, 1, "correlation", boundary, zp), batch, 1, "kernel-major", route)
    ref, croute = _run_complex(opts, x, h)
    assert _rel(got, ref) < 1e-6, (route, croute)


def test_route1_strided_lanes_on_both_sides(oracle):
    """channel lanes: element stride 3 on the input, 2 on the output, explicit batch strides, offsets and a kernel lane step — an element is one f32"""
    n, kn, batch, K = 256, 256, 5, 2
    si, so, ioff, ooff = 3, 2, 5, 3
    ibs, obs, kst = n * si + 11, n * so + 7, 1          # kernel lanes interleave on the output: stride 2, kernel step 1
    layout = {"inputStrides": [si], "outputStrides": [so], "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    opts = _opts([n], [kn], batch, K=K, layout=layout, outputKernelStrideElements=kst)
    desc, r = _desc(opts)
    dense = _rand(n * batch, 0xA1)
    h = _rand(kn * K, 0xA2)
    phys = _rand(ioff + (batch - 1) * ibs + (n - 1) * si + 1, 0xA3)
    for b in range(batch):
        phys[ioff + b * ibs: ioff + b * ibs + n * si: si] = dense[b * n:(b + 1) * n]
    out_floats = ooff + (K - 1) * kst + (batch - 1) * obs + (n - 1) * so + 1
    sentinel = np.full(out_floats, 777.0, np.float32)
    got, route, launches = emu.run_plan(desc, phys, out_floats, kernel=h, out_init=sentinel)
    _route1(route, launches, K, 256)
    want = _want(dense, h, [n], [kn], batch, K, "convolution", "circular")
    touched = np.zeros(out_floats, bool)
    for k in range(K):
        for b in range(batch):
            sl = slice(ooff + k * kst + b * obs, ooff + k * kst + b * obs + n * so, so)
            touched[sl] = True
            _close(got[sl], want[k, b].astype(np.float32), 4e-3, 4e-3, f"{route.strip()} kernel {k} line {b}")
            assert _rel(got[sl], want[k, b]) < 1e-5
    assert np.all(got[~touched] == 777.0), "stores outside the output lanes"


# ---- routes 2 and 3 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kshape,boundary,mode,K,out_layout", [
    ([32, 12], [5, 3], "linear-same", "convolution", 2, "batch-major"),
    ([31, 12], [4, 3], "linear-full", "correlation", 1, "kernel-major"),      # axis 0: 34 (even already); correlation lags on both axes
    ([30, 10], [5, 3], "linear-valid", "correlation", 1, "kernel-major"),     # axis 0: 34
    ([32, 16], [32, 16], "circular", "convolution", 2, "kernel-major"),
    ([16, 6, 5], [3, 2, 2], "linear-full", "convolution", 1, "kernel-major"),
    ([12, 8, 4], [12, 8, 4], "circular", "correlation", 2, "batch-major"),
])
def test_route2_rank2_and_rank3(oracle, shape, kshape, boundary, mode, K, out_layout):
    batch = 2
    x, h = _rand(int(np.prod(shape)) * batch, 0xB1), _rand(int(np.prod(kshape)) * K, 0xB2)
    opts = _opts(shape, kshape, batch, K=K, mode=mode, boundary=boundary, out_layout=out_layout)
    got, route, launches, r = _run(opts, x, h)
    assert f"rconv[K={K}]" in route and "lines-rconv" not in route and "rconv-widened" not in route, route
    want = _want(x, h, shape, kshape, batch, K, mode, boundary)
    _check(oracle, got, want.reshape(K, batch, -1), batch, K, out_layout, route)
    ref, croute = _run_complex(opts, x, h)
    assert _rel(got, ref) < 1e-6, (route, croute)


def test_route2_odd_linear_axis0_is_rounded_up(oracle):
    """rank 2, axis 0 of the FFT domain 33 -> 34, zeroPad on both stages, correlation: the crop straddles split on the padded axis"""
    shape, kshape, batch = [29, 8], [5, 3], 2
    zp = {"read": {"start": [2, 1], "end": [27, 8]}, "write": {"start": [1, 0], "end": [31, 9]}}
    x, h = _rand(29 * 8 * batch, 0xB5), _rand(15, 0xB6)
    opts = _opts(shape, kshape, batch, mode="correlation", boundary="linear-full", zero_pad=zp)
    got, route, launches, _ = _run(opts, x, h)
    assert "pad[33->34]" in route and "rconv[K=1]" in route, route
    want = _want(x, h, shape, kshape, batch, 1, "correlation", "linear-full", zp)
    _check(oracle, got, want.reshape(1, batch, -1), batch, 1, "kernel-major", route)
    ref, croute = _run_complex(opts, x, h)
    assert _rel(got, ref) < 1e-6, (route, croute)


def test_route2_long_linear_line_on_2p16(oracle):
    n, kn, batch, K = 40000, 9000, 2, 2
    x, h = _rand(n * batch, 0xC1), _rand(kn * K, 0xC2)
    got, route, launches, _ = _run(_opts([n], [kn], batch, K=K, mode="correlation", boundary="linear-full"), x, h)
    assert "pad[48999->65536]" in route and "rconv[K=2]" in route and "lines-rconv" not in route, route
    assert not [w for w in ("bluestein", "stages", "mixed") if w in route], route
    _check(oracle, got, _want(x, h, [n], [kn], batch, K, "correlation", "linear-full"), batch, K, "kernel-major", route)


@pytest.mark.parametrize("n,kn,K", [(255, 255, 1), (1001, 77, 2)])
def test_route3_odd_circular_is_widened(oracle, n, kn, K):
    batch = 3
    x, h = _rand(n * batch, 0xD1), _rand(kn * K, 0xD2)
    opts = _opts([n], [kn], batch, K=K, mode="correlation")
    got, route, launches, _ = _run(opts, x, h)
    assert route.startswith("rconv-widened "), route
    _check(oracle, got, _want(x, h, [n], [kn], batch, K, "correlation", "circular"), batch, K, "kernel-major", route)
    ref, croute = _run_complex(opts, x, h)
    assert _rel(got, ref) < 1e-6, (route, croute)


@pytest.mark.parametrize("opts", [
    _opts([1024], [200], 9, K=2, mode="correlation"),
    _opts([1000], [31], 5, K=1, mode="correlation", boundary="linear-same",
          zero_pad={"read": {"start": [3], "end": [990]}, "write": {"start": [10], "end": [1000]}}),
    _opts([4000], [97], 2, K=2, boundary="linear-valid", out_layout="batch-major"),
])
def test_switch_forces_route2_and_routes_agree(oracle, monkeypatch, opts):
    n, kn, batch, K = opts["shape"][0], opts["fftConv"]["kernelShape"][0], opts["batch"], opts["fftConv"]["kernelCount"]
    x, h = _rand(n * batch, 0xE1), _rand(kn * K, 0xE2)
    got1, route1, launches1, _ = _run(opts, x, h)
    assert "lines-rconv[" in route1 and launches1 == 1 + K, route1
    monkeypatch.setenv("MI355_EMU_RCONV_FUSED", "0")
    got2, route2, launches2, _ = _run(opts, x, h)
    assert f"rconv[K={K}]" in route2 and "lines-rconv" not in route2, route2
    assert launches2 > launches1
    assert _rel(got1, got2) < 1e-6, (route1, route2)
    want = _want(x, h, [n], [kn], batch, K, opts["fftConv"]["mode"], opts["fftConv"]["boundary"], opts.get("zeroPad"))
    _check(oracle, got2, want, batch, K, opts["fftConv"]["outputLayout"], route2)


def test_planner_switch_of_the_product(monkeypatch):
    desc, _ = _desc(_opts([4096], [4096], 64, K=2))
    route, launches, _ = emu.plan_only(desc)
    assert "lines-rconv[N=4096]" in route and launches == 3, route
    monkeypatch.setenv("MI355FFT_RCONV_FUSED", "0")
    route0, launches0, _ = emu.plan_only(desc)
    assert "rconv[K=2]" in route0 and "lines-rconv" not in route0 and launches0 > launches, route0
    monkeypatch.delenv("MI355FFT_RCONV_FUSED")
    # P = 16384 and 32768: rconv[K] by default (measured), the line route through the switch's value 2 and for strided sides
    for P in (8192, 16384, 32768):
        dP, _ = _desc(_opts([P], [P], 4, K=2))
        assert ("lines-rconv[N=%d]" % P in emu.plan_only(dP)[0]) == (P <= 8192), P
        dS, _ = _desc(_opts([P], [P], 4, K=1, layout={"inputStrides": [2]}))
        assert "lines-rconv[N=%d]" % P in emu.plan_only(dS)[0], P
        monkeypatch.setenv("MI355FFT_RCONV_FUSED", "2")
        assert "lines-rconv[N=%d]" % P in emu.plan_only(dP)[0], P
        monkeypatch.delenv("MI355FFT_RCONV_FUSED")
    for shape, route_tag in (([65536], "rconv[K=2]"), ([100], "rconv[K=2]"), ([3000], "rconv[K=2]"), ([999], "rconv-widened")):
        d2, _ = _desc(_opts(shape, shape, 4, K=2))
        assert route_tag in emu.plan_only(d2)[0], shape


def test_strided_sides_off_the_line_route_are_unsupported():
    layout = {"inputStrides": [2]}
    for opts in (_opts([1000], [1000], 2, layout=layout),            # circular, not a power of two: rconv[K]
                 _opts([999], [999], 2, layout=layout),              # odd: rconv-widened
                 _opts([40000], [9000], 2, boundary="linear-full", layout=layout)):
        desc, _ = _desc(opts)
        with pytest.raises(emu.EmuError) as e:
            emu.plan_only(desc)
        assert "Unsupported: strided layouts on real fftconv outside the one-launch line route" in str(e.value)
        assert e.value.code == _abi.ERR_UNSUPPORTED
