"""GPU tier (-m gpu): fftconv over real data (type "fftconv" with layout.interleavedComplex false -> MI355FFT_FFTCONV_REAL) through the C ABI.

The families of test_emu_fftconv_real.py on the HIP path: the one-launch line route (lines-rconv[N=P], 1 + K launches), the composed route
(rconv[K], also through MI355FFT_RCONV_FUSED=0) and the widened route of odd circular lines.  References are numpy float64 computed
here (helpers of the CPU tier's module); bars: elementwise 4e-3 / 4e-3 and rel_l2 < 1e-5 against float64, rel_l2 < 1e-6 between routes and
against the complex plan on the same data with zero imaginary parts.  One full-size request is checked route against route on the
device, and one recorded command list is replayed three times with and without a captured graph."""
import numpy as np
import pytest

from test_emu_fftconv_real import FORBIDDEN, _check, _opts, _rand, _rel, _want
from test_gpu_parity import run_plan

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


def _out_floats(opts):
    from mi355fft.layout import resolve_plan_options
    r = resolve_plan_options(opts)
    return int(np.prod(r["outputShape"])) * r["batch"] * r["conv"]["kernelCount"]


def _run(fft, dev, opts, x, h, **kw):
    got, (route, launches) = run_plan(fft, dev, opts, x, _out_floats(opts), kernel=h, **kw)
    return got, route, launches


def _run_complex(fft, dev, opts, x, h):
    xc = np.zeros(2 * x.size, np.float32); xc[0::2] = x
    hc = np.zeros(2 * h.size, np.float32); hc[0::2] = h
    o = dict(opts, layout={"interleavedComplex": True})
    got, (route, _) = run_plan(fft, dev, o, xc, 2 * _out_floats(opts), kernel=hc)
    return got[0::2].copy(), route


def _route1(route, launches, K, P, fn=None):
    assert f"lines-rconv[N={P}]" in route, route
    assert launches == 1 + K, (route, launches)
    assert not [w for w in FORBIDDEN if w in route], route
    assert (f"pad[{fn}->{P}]" in route) if (fn is not None and fn != P) else ("pad[" not in route), route


@pytest.mark.parametrize("P,batch", [(128, 1000), (1024, 777), (4096, 301), (16384, 70), (32768, 33)])
@pytest.mark.parametrize("mode", ["convolution", "correlation"])
def test_route1_circular(fft, dev, oracle, monkeypatch, P, batch, mode):
    """more tiles than workgroups of the resident grid at the short lengths, ragged last tiles"""
    if P > 8192:
        monkeypatch.setenv("MI355FFT_RCONV_FUSED", "2")       # above 8192 the planner's default is rconv[K]: the line route through the switch
    ks = [P] if P <= 1024 else [P // 3]
    x, h = _rand(P * batch, 0x51 + P), _rand(ks[0], 0x52 + P)
    opts = _opts([P], ks, batch, mode=mode)
    got, route, launches = _run(fft, dev, opts, x, h)
    _route1(route, launches, 1, P)
    _check(oracle, got, _want(x, h, [P], ks, batch, 1, mode, "circular"), batch, 1, "kernel-major", route)
    ref, croute = _run_complex(fft, dev, opts, x, h)
    print(f"{route.strip()} vs complex {croute.strip()}: rel_l2={_rel(got, ref):.3e}")
    assert _rel(got, ref) < 1e-6, (route, croute)


@pytest.mark.parametrize("n,kn,boundary,mode,batch", [
    (1000, 31, "linear-full", "convolution", 600),
    (1000, 31, "linear-same", "correlation", 600),     # the crop straddles split
    (1000, 31, "linear-valid", "convolution", 65),
    (20000, 5000, "linear-full", "convolution", 40),   # pad[24999->32768]
    (20000, 5000, "linear-same", "correlation", 7),
    (97, 20, "linear-full", "correlation", 333),       # pad[116->128]
])
def test_route1_linear_padded(fft, dev, oracle, monkeypatch, n, kn, boundary, mode, batch):
    if n + kn - 1 > 8192:
        monkeypatch.setenv("MI355FFT_RCONV_FUSED", "2")
    x, h = _rand(n * batch, 0x61 + n), _rand(kn, 0x62 + kn)
    opts = _opts([n], [kn], batch, mode=mode, boundary=boundary)
    got, route, launches = _run(fft, dev, opts, x, h)
    fn = n + kn - 1
    _route1(route, launches, 1, max(128, 1 << (fn - 1).bit_length()), fn)
    _check(oracle, got, _want(x, h, [n], [kn], batch, 1, mode, boundary), batch, 1, "kernel-major", route)
    ref, croute = _run_complex(fft, dev, opts, x, h)
    print(f"{route.strip()} vs complex {croute.strip()}: rel_l2={_rel(got, ref):.3e}")
    assert _rel(got, ref) < 1e-6, (route, croute)


@pytest.mark.parametrize("out_layout", ["kernel-major", "batch-major"])
def test_route1_three_kernels_with_zero_pad(fft, dev, oracle, out_layout):
    n, kn, batch, K = 1000, 31, 129, 3
    zp = {"read": {"start": [7], "end": [900]}, "write": {"start": [20], "end": [997]}}
    x, h = _rand(n * batch, 0x81), _rand(kn * K, 0x82)
    opts = _opts([n], [kn], batch, K=K, mode="correlation", boundary="linear-full", out_layout=out_layout, zero_pad=zp)
    got, route, launches = _run(fft, dev, opts, x, [h[k * kn:(k + 1) * kn] for k in range(K)])      # kernels as a list
    _route1(route, launches, K, 2048, 1030)
    _check(oracle, got, _want(x, h, [n], [kn], batch, K, "correlation", "linear-full", zp), batch, K, out_layout, route)
    ref, croute = _run_complex(fft, dev, opts, x, h)
    assert _rel(got, ref) < 1e-6, (route, croute)


def test_route1_strided_lanes_on_both_sides(fft, dev, oracle):
    n, kn, batch, K = 256, 256, 75, 2
    si, so, ioff, ooff = 3, 2, 5, 3
    ibs, obs, kst = n * si + 11, n * so + 7, 1
    layout = {"inputStrides": [si], "outputStrides": [so], "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    opts = _opts([n], [kn], batch, K=K, layout=layout, outputKernelStrideElements=kst)
    dense, h = _rand(n * batch, 0xA1), _rand(kn * K, 0xA2)
    phys = _rand(ioff + (batch - 1) * ibs + (n - 1) * si + 2, 0xA3)
    for b in range(batch):
        phys[ioff + b * ibs: ioff + b * ibs + n * si: si] = dense[b * n:(b + 1) * n]
    out_floats = ooff + (K - 1) * kst + (batch - 1) * obs + (n - 1) * so + 1
    got, (route, launches) = run_plan(fft, dev, opts, phys, out_floats, kernel=h, out_init=np.full(out_floats, 777.0, np.float32))
    _route1(route, launches, K, 256)
    want = _want(dense, h, [n], [kn], batch, K, "convolution", "circular")
    touched = np.zeros(out_floats, bool)
    for k in range(K):
        for b in range(batch):
            sl = slice(ooff + k * kst + b * obs, ooff + k * kst + b * obs + n * so, so)
            touched[sl] = True
            oracle.assert_close_elementwise(got[sl], want[k, b].astype(np.float32), 4e-3, 4e-3, f"{route.strip()} kernel {k} line {b}")
            assert _rel(got[sl], want[k, b]) < 1e-5
    assert np.all(got[~touched] == 777.0), "stores outside the output lanes"


@pytest.mark.parametrize("shape,kshape,boundary,mode,K,out_layout,tag", [
    ([64, 48], [5, 3], "linear-same", "convolution", 2, "batch-major", "rconv[K=2]"),
    ([61, 30], [4, 3], "linear-full", "correlation", 1, "kernel-major", "rconv[K=1]"),
    ([32, 16, 8], [3, 2, 2], "linear-full", "convolution", 1, "kernel-major", "rconv[K=1]"),
    ([128, 64], [128, 64], "circular", "correlation", 2, "kernel-major", "rconv[K=2]"),
    ([40000], [9000], "linear-full", "correlation", 2, "kernel-major", "rconv[K=2]"),        # pad[48999->65536]
    ([1001], [77], "circular", "correlation", 2, "kernel-major", "rconv-widened"),
])
def test_routes_2_and_3(fft, dev, oracle, shape, kshape, boundary, mode, K, out_layout, tag):
    batch = 5
    x, h = _rand(int(np.prod(shape)) * batch, 0xB1), _rand(int(np.prod(kshape)) * K, 0xB2)
    opts = _opts(shape, kshape, batch, K=K, mode=mode, boundary=boundary, out_layout=out_layout)
    got, route, launches = _run(fft, dev, opts, x, h)
    assert tag in route and "lines-rconv" not in route, route
    want = _want(x, h, shape, kshape, batch, K, mode, boundary)
    _check(oracle, got, want.reshape(K, batch, -1), batch, K, out_layout, route)
    if shape[0] < 40000:
        ref, croute = _run_complex(fft, dev, opts, x, h)
        assert _rel(got, ref) < 1e-6, (route, croute)


@pytest.mark.parametrize("opts", [
    _opts([1024], [200], 777, K=2, mode="correlation"),
    _opts([1000], [31], 300, K=1, mode="correlation", boundary="linear-same",
          zero_pad={"read": {"start": [3], "end": [990]}, "write": {"start": [10], "end": [1000]}}),
    _opts([16384], [999], 40, K=2, out_layout="batch-major"),
])
def test_switch_forces_route2_and_routes_agree(fft, dev, oracle, monkeypatch, opts):
    n, kn, batch, K = opts["shape"][0], opts["fftConv"]["kernelShape"][0], opts["batch"], opts["fftConv"]["kernelCount"]
    x, h = _rand(n * batch, 0xE1), _rand(kn * K, 0xE2)
    monkeypatch.setenv("MI355FFT_RCONV_FUSED", "2" if n > 8192 else "1")
    got1, route1, launches1 = _run(fft, dev, opts, x, h)
    assert "lines-rconv[" in route1 and launches1 == 1 + K, route1
    monkeypatch.setenv("MI355FFT_RCONV_FUSED", "0")
    got2, route2, launches2 = _run(fft, dev, opts, x, h)
    assert f"rconv[K={K}]" in route2 and "lines-rconv" not in route2 and launches2 > launches1, route2
    print(f"{route1.strip()} vs {route2.strip()}: rel_l2={_rel(got1, got2):.3e}")
    assert _rel(got1, got2) < 1e-6, (route1, route2)


def test_strided_side_off_the_line_route_is_unsupported(fft, dev):
    with pytest.raises(fft.Mi355Error) as e:
        fft.createPlan(dev, _opts([1000], [1000], 2, layout={"inputStrides": [2]}))
    assert "Unsupported: strided layouts on real fftconv outside the one-launch line route" in str(e.value)


def test_exec_checks_the_real_kernel_lengths(fft, dev):
    plan = fft.createPlan(dev, _opts([256], [100], 2, K=2))
    inp, out = dev.createBuffer({"size": 2 * 256 * 4}), dev.createBuffer({"size": 2 * 2 * 256 * 4})
    enc = dev.createCommandEncoder()
    for kernel, msg in ((np.zeros(400, np.float32), "kernel Float32Array length must be 200 for kernelCount=2; got 400"),
                        ([np.zeros(100, np.float32)], "kernel array length must equal fftConv.kernelCount=2; got 1"),
                        ([np.zeros(100, np.float32), np.zeros(200, np.float32)], "kernel[1] Float32Array length must be 100; got 200")):
        with pytest.raises(fft.Mi355Error) as e:
            plan.exec(enc, {"input": inp, "output": out, "kernel": kernel})
        assert msg in str(e.value)
    small = dev.createBuffer({"size": 2 * 100 * 4 - 8})
    with pytest.raises(fft.Mi355Error) as e:
        plan.exec(enc, {"input": inp, "output": out, "kernel": small})
    assert "kernel buffer too small" in str(e.value)
    with pytest.raises(fft.Mi355Error) as e:
        plan.exec(enc, {"input": inp, "output": out})
    assert "fftconv exec requires kernel" in str(e.value)
    for b in (inp, out, small):
        b.destroy()
    plan.destroy()


def test_full_size_route1_against_route2_on_the_device(fft, dev, monkeypatch):
    """4096 points x 65536 lines (1 GiB of input), K = 2: every output of the one-launch route against the composed route"""
    n, batch, K = 4096, 65536, 2
    opts = _opts([n], [n], batch, K=K, mode="correlation")
    h = _rand(n * K, 0xF2)
    inp = dev.createBuffer({"size": 4 * n * batch})
    dev.fillRandom(inp, 0, n, batch, 0xF1F1)
    outs, routes = [], []
    for fused in ("1", "0"):
        monkeypatch.setenv("MI355FFT_RCONV_FUSED", fused)
        plan = fft.createPlan(dev, opts)
        out = dev.createBuffer({"size": 4 * n * batch * K})
        enc = dev.createCommandEncoder()
        plan.exec(enc, {"input": inp, "output": out, "kernel": h})
        dev.queue.submit([enc.finish()])
        dev.queue.onSubmittedWorkDone()
        routes.append(plan.describe())
        plan.destroy()
        outs.append(out)
    assert "lines-rconv[N=4096]" in routes[0][0] and routes[0][1] == 1 + K, routes[0]
    assert "rconv[K=2]" in routes[1][0] and "lines-rconv" not in routes[1][0], routes[1]
    count = n * batch * K
    ref = dev.sumsq(outs[1], 0, count)
    diff = dev.diffSumsq(outs[0], 0, outs[1], 0, 1.0, count)
    rel = float(np.sqrt(diff / ref))
    print(f"{routes[0][0].strip()} vs {routes[1][0].strip()}: {count} outputs, rel_l2={rel:.3e}, rms={np.sqrt(ref / count):.3e}")
    assert ref > 0 and rel < 1e-6
    for b in outs + [inp]:
        b.destroy()


@pytest.mark.parametrize("use_graph", [False, True])
def test_replay_of_a_recorded_list(fft, dev, oracle, use_graph):
    n, kn, batch, K = 1000, 31, 200, 2
    x, h = _rand(n * batch, 0x91), _rand(kn * K, 0x92)
    opts = _opts([n], [kn], batch, K=K, boundary="linear-same")
    want = _want(x, h, [n], [kn], batch, K, "convolution", "linear-same")
    plan = fft.createPlan(dev, opts)
    inp = dev.createBuffer({"size": x.nbytes})
    dev.queue.writeBuffer(inp, 0, x)
    out = dev.createBuffer({"size": 4 * n * batch * K})
    enc = dev.createCommandEncoder()
    plan.exec(enc, {"input": inp, "output": out, "kernel": h})
    cb = enc.finish(use_graph=use_graph)
    route = plan.describe()[0]
    assert "lines-rconv[N=2048]" in route, route
    for rep in range(3):
        dev.queue.writeBuffer(out, 0, np.full(n * batch * K, 777.0, np.float32))
        dev.queue.submit([cb])
        dev.queue.onSubmittedWorkDone()
        got = fft.downloadF32(dev, out, n * batch * K)
        _check(oracle, got, want, batch, K, "kernel-major", f"{route.strip()} replay {rep} graph={use_graph}")
    cb.release()
    plan.destroy()
    inp.destroy()
    out.destroy()
