"""What the tests of the four overlap-save routes of fftconv share (fftconv_{ols,cols,tiles,rtiles}_cases.py hold a Route and its tables,
test_{emu,gpu}_fftconv_{ols,cols,tiles,rtiles}.py run them): the route descriptor with its bars, the case class, the data of a case and its
float64 reference, the checks both tiers run on a case and on the strided request, the exec-contract oracles, float64 direct sums, and the
two tiers' runners.

A case names the request and the block length (rank 2: the tile edge) P that the route's switch forces (names without their prefix: the GPU
tier sets MI355FFT_<switch>, the emulation tier MI355_EMU_<switch>); P = None leaves the planner's own rule, and `rule` is the P that rule
names (None: the tag is checked up to "N=").  Geometry per axis a (axis 0 fastest): M_a = kernelShape[a], L_a = P - (M_a - 1) results a block
and nb_a = ceil((shape[a] + M_a - 1) / L_a) blocks; on real LINES e = (M - 1) & 1 and L = (P - (M - 1) - e) & ~1.

References are numpy float64 on the exact linear domain shape + kernelShape - 1: the conjugated kernel spectrum for a correlation,
zeroPad.read applied to the data and zeroPad.write to the logical result, cropped per boundary (real data: test_emu_fftconv_real._want;
complex data: fftconv_linear_cases.reference on lines, reference2d on images).  Real data are f32 arrays and complex data interleaved f32.

The bars belong to the route, not to this module: `f64` bounds rel_l2 against the float64 reference and `parity` rel_l2 against the same
request planned with the switch at 0 (the routes the planner had before) and, where the route has a `complex_switch`, against the real
parts of the complex plan on the same data with zero imaginary parts.  Elementwise 4e-3 / 4e-3 holds everywhere (real data through
check_against_f64, complex data through exec_contract_cases.TOL_CONV).  Every case asserts the route tag, 1 + K launches and that the route
names none of the `forbidden` launches."""
import operator

import numpy as np

import exec_contract_cases as t
import fftconv_linear_cases as lin
from test_emu_fftconv_real import _check, _desc, _opts, _rand as _rand_real, _rel, _want

MODES = ("convolution", "correlation")
BOUNDARIES = ("linear-full", "linear-same", "linear-valid")


class Bar:
    """rel_l2 < limit or rel_l2 <= limit: which of the two is the route's"""
    def __init__(self, op, limit):
        self.op, self.limit = op, limit

    def holds(self, value):
        return self.op(value, self.limit)


def below(limit):
    return Bar(operator.lt, limit)


def at_most(limit):
    return Bar(operator.le, limit)


def _rand_complex(n, seed):
    """n complex elements, interleaved f32"""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, 2 * n).astype(np.float32)


def options(shape, ks, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None):
    """a complex request"""
    opts = {"type": "fftconv", "shape": list(shape), "batch": batch,
            "fftConv": {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": list(ks), "outputLayout": out_layout}}
    if zero_pad:
        opts["zeroPad"] = zero_pad
    return opts


def _box(zr, dom):
    """a zeroPad range as a boolean mask over the domain (numpy order: axis 1, axis 0)"""
    keep = np.zeros((dom[1], dom[0]), bool)
    keep[max(0, zr["start"][1]):max(0, zr["end"][1]), max(0, zr["start"][0]):max(0, zr["end"][0])] = True
    return keep


def reference2d(shape, ks, batch, K, mode, boundary, zero_pad, x, h):
    """float64 reference [K][batch][os1][os0][2] of dense complex data x [batch][n1][n0] and kernels h [K][m1][m0] (interleaved f32, axis 0 fastest)"""
    (f0, o0, c0), (f1, o1, c1) = (lin.geometry((n, kn, boundary)) for n, kn in zip(shape, ks))
    xc = np.asarray(x, np.float64).reshape(batch, shape[1], shape[0], 2)
    xc = xc[..., 0] + 1j * xc[..., 1]
    if zero_pad and zero_pad.get("read"):
        xc = np.where(_box(zero_pad["read"], shape), xc, 0)
    hc = np.asarray(h, np.float64).reshape(K, ks[1], ks[0], 2)
    hc = hc[..., 0] + 1j * hc[..., 1]
    X = np.fft.fft2(xc, s=(f1, f0))
    want = np.empty((K, batch, o1, o0, 2))
    for k in range(K):
        H = np.fft.fft2(hc[k], s=(f1, f0))
        y = np.fft.ifft2(X * (np.conj(H) if mode == "correlation" else H))
        if zero_pad and zero_pad.get("write"):
            y = np.where(_box(zero_pad["write"], (f0, f1)), y, 0)
        y = y[:, c1:c1 + o1, c0:c0 + o0]
        want[k, ..., 0], want[k, ..., 1] = y.real, y.imag
    return want


class Case:
    def __init__(self, route, name, shape, ks, P, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None,
                 rule=None, kernel_list=False):
        self.route, self.name, self.shape, self.ks, self.P, self.batch, self.K = route, name, tuple(shape), tuple(ks), P, batch, K
        self.mode, self.boundary, self.out_layout, self.zero_pad, self.rule, self.kernel_list = mode, boundary, out_layout, zero_pad, rule, kernel_list

    @property
    def tag(self):
        P = self.P or self.rule
        return self.route.tag + "N=" if P is None else self.route.tag_of(P, self.ks)

    @property
    def opts(self):
        return self.route.options(self.shape, self.ks, self.batch, K=self.K, mode=self.mode, boundary=self.boundary, out_layout=self.out_layout,
                                  zero_pad=self.zero_pad)

    def __repr__(self):
        return self.name


class Route:
    """One overlap-save route: `switch` and `tag` ("...["), the substrings its route string must not hold, rank, real or complex elements, its two
    bars, the seeds of its cases' data (data: seed + elements; kernels: seed + 1 + kernel elements) and of its strided request (seed, + 1, + 2),
    and the strided request itself: dict(shape, ks, batch, K, P, si, so, ioff, ooff, kst), strides per axis in elements.
    route0_has: what the route string of the switch at 0 must hold.  unsupported: the error text of the strided request with the switch at 0 (such
    a request had no plan before the route), in place of the comparison with that plan."""
    def __init__(self, switch, tag, forbidden, rank, real, f64, parity, seed, strided_seed, strided, route0_has=None, complex_switch=None, unsupported=None):
        self.switch, self.tag, self.forbidden, self.rank, self.real, self.f64, self.parity = switch, tag, forbidden, rank, real, f64, parity
        self.seed, self.strided_seed, self.strided = seed, strided_seed, strided
        self.route0_has, self.complex_switch, self.unsupported = route0_has, complex_switch, unsupported
        self.rand = _rand_real if real else _rand_complex
        self._want = {}        # per route: collecting one module computes no other route's references

    def case(self, *a, **kw):
        return Case(self, *a, **kw)

    def tag_of(self, P, ks):
        if self.rank == 2:
            return f"{self.tag}N={P}x{P},L={P - ks[0] + 1}x{P - ks[1] + 1}]"
        pre = ks[0] - 1 + ((ks[0] - 1) & 1 if self.real else 0)
        return f"{self.tag}N={P},L={(P - pre) & ~1 if self.real else P - pre}]"

    def options(self, shape, ks, batch, K=1, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None):
        if self.real:
            return _opts(list(shape), list(ks), batch, K=K, mode=mode, boundary=boundary, out_layout=out_layout, zero_pad=zero_pad)
        return options(shape, ks, batch, K, mode, boundary, out_layout, zero_pad)

    def reference(self, shape, ks, batch, K, mode, boundary, zero_pad, x, h):
        """float64, kernel-major: [K][batch][out] (numpy order; complex data: a last axis of 2)"""
        if self.real:
            return _want(x, h, list(shape), list(ks), batch, K, mode, boundary, zero_pad)
        if self.rank == 1:
            return lin.reference((shape[0], ks[0], boundary, mode, K, None, zero_pad), x, h, batch)
        return reference2d(shape, ks, batch, K, mode, boundary, zero_pad, x, h)

    def in_layout(self, want, K, batch, out_layout):
        """the kernel-major reference flat in the plan's output layout"""
        w = want.reshape(K, batch, -1)
        return np.ascontiguousarray(w if out_layout == "kernel-major" else w.transpose(1, 0, 2)).reshape(-1)

    def data(self, case):
        """(x, h, float64 reference) of a case, computed once per process and read-only.  Real data: the reference kernel-major [K][batch][out];
        complex data: flat, in the plan's output layout"""
        if case.name not in self._want:
            n, kn = int(np.prod(case.shape)), int(np.prod(case.ks))
            x, h = self.rand(n * case.batch, self.seed + n + kn), self.rand(kn * case.K, self.seed + 1 + kn)
            want = self.reference(case.shape, case.ks, case.batch, case.K, case.mode, case.boundary, case.zero_pad, x, h)
            if not self.real:
                want = self.in_layout(want, case.K, case.batch, case.out_layout)
            for a in (x, h, want):
                a.setflags(write=False)
            self._want[case.name] = (x, h, want)
        return self._want[case.name]

    def assert_route(self, case, route, launches):
        assert case.tag in route, (route, case.tag)
        assert launches == 1 + case.K, (route, launches)
        assert not any(f in route for f in self.forbidden), route

    def check_case(self, run, setenv, oracle, case):
        """run(opts, x, out_floats, kernel) -> (got, route, launches) plans and runs under the environment; setenv(name, value) sets the tier's
        form of a planner switch"""
        x, h, want = self.data(case)
        kn = int(np.prod(case.ks))
        kernel = [h[k * kn:(k + 1) * kn] for k in range(case.K)] if case.kernel_list else h
        if case.P is not None:
            setenv(self.switch, str(case.P))
        got, route, launches = run(case.opts, x, want.size, kernel)
        self.assert_route(case, route, launches)
        if self.real:
            _check(oracle, got, want, case.batch, case.K, case.out_layout, route)
            flat = self.in_layout(want, case.K, case.batch, case.out_layout)
        else:
            from test_gpu_parity import check
            print(f"{route.strip()}: rel_l2={_rel(got, want):.3e}")
            check(oracle, got, want.astype(np.float32), f"{case.name} ({route.strip()})", *t.TOL_CONV[1:])
            flat = want
        assert self.f64.holds(_rel(np.asarray(got).reshape(-1), flat))
        if self.complex_switch:
            # the complex plan (its own route where the case forces one) on the same data with zero imaginary parts: what a user could do before
            if case.P is not None:
                setenv(self.complex_switch, str(case.P))
            oc, xc, hc = widened(case.opts, x, h)
            cgot, croute, _ = run(oc, xc, 2 * want.size, hc)
            rel = _rel(got, np.asarray(cgot)[0::2])
            print(f"{route.strip()} vs complex {croute.strip()}: rel_l2={rel:.3e}")
            assert self.parity.holds(rel), (route, croute)
        setenv(self.switch, "0")
        ref, route0, _ = run(case.opts, x, want.size, kernel)
        assert self.tag[:-1] not in route0 and (self.route0_has or "") in route0, route0
        rel = _rel(got, ref)
        print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
        assert self.parity.holds(rel), (route, route0)

    # ---- strided lanes on both sides: strides, offsets and batch strides on every axis, kernel lanes kst apart ----
    def strided_request(self):
        """(opts, physical input, kernels, float64 reference [K][batch][out], output floats, index arrays of the lanes in elements)"""
        s = self.strided
        shape, ks, batch, K, si, so, ioff, ooff, kst = (s[k] for k in ("shape", "ks", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
        ibs, obs = shape[-1] * si[-1] + 11, shape[-1] * so[-1] + 7
        layout = {"inputStrides": list(si), "outputStrides": list(so), "inputOffsetElements": ioff, "outputOffsetElements": ooff,
                  "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
        if self.real:
            opts = _opts(list(shape), list(ks), batch, K=K, boundary="linear-same", layout=layout, outputKernelStrideElements=kst)
        else:
            opts = options(shape, ks, batch, K)
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
            want = self.reference(shape, ks, batch, K, "convolution", "linear-same", None, dense, h)
            phys = phys.reshape(-1)
            for a in (phys, h, want):
                a.setflags(write=False)
            self._want["strided"] = (phys, h, want)
        phys, h, want = self._want["strided"]
        out_elems = ooff + (K - 1) * kst + (batch - 1) * obs + int(opos.max()) + 1
        lanes = {(k, b): ooff + k * kst + b * obs + opos for k in range(K) for b in range(batch)}
        return opts, phys, h, want, out_elems * (1 if self.real else 2), lanes

    def strided_tag(self):
        return self.tag_of(self.strided["P"], self.strided["ks"])

    def _elements(self, a):
        return np.asarray(a) if self.real else np.asarray(a).reshape(-1, 2)

    def check_strided(self, run, setenv, oracle, unsupported=None):
        """run(opts, x, out_floats, kernel, out_init) as above; the output starts as 777.0 everywhere and every element outside the lanes keeps it.
        unsupported(opts), for a route with `unsupported`: asserts that planning the request fails with that text"""
        from test_emu_fftconv import _close
        opts, phys, h, want, out_floats, lanes = self.strided_request()
        K = self.strided["K"]
        setenv(self.switch, str(self.strided["P"]))
        sentinel = np.full(out_floats, 777.0, np.float32)
        got, route, launches = run(opts, phys, out_floats, h, sentinel)
        assert self.strided_tag() in route and launches == 1 + K, (route, launches)
        got = self._elements(got)
        touched = np.zeros(len(got), bool)
        for (k, b), idx in lanes.items():
            assert not touched[idx].any(), "the lanes of the request overlap"
            touched[idx] = True
            _close(got[idx].reshape(-1), want[k, b].astype(np.float32).reshape(-1), 4e-3, 4e-3,
                   f"{route.strip()} kernel {k} {'line' if self.rank == 1 else 'image'} {b}")
            assert self.f64.holds(_rel(got[idx], want[k, b]))
        assert np.all(got[~touched] == 777.0), "stores outside the output lanes"
        setenv(self.switch, "0")
        if self.unsupported:
            unsupported(opts)
            return
        ref, route0, _ = run(opts, phys, out_floats, h, sentinel)
        assert self.tag[:-1] not in route0, route0
        rel = _rel(got[touched], self._elements(ref)[touched])
        print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
        assert self.parity.holds(rel), (route, route0)

    def strided_contract_oracle(self, oracle, o):
        """exec_contract_cases oracle of the strided request: NaN where the plan's contract leaves the output alone"""
        _, phys, h, want, out_floats, lanes = self.strided_request()
        full = self._elements(np.full(out_floats, np.nan))
        for (k, b), idx in lanes.items():
            full[idx] = want[k, b]
        return phys, h, full.reshape(-1)

    def dense_oracle(self, seed):
        """exec_contract_cases oracle of a dense request against the float64 reference, in the plan's output layout"""
        if self.real:
            return t._rconv(seed)

        def f(oracle, o):
            fc, shape, batch = o["fftConv"], o["shape"], o["batch"]
            ks, K = fc["kernelShape"], fc["kernelCount"]
            x, h = self.rand(int(np.prod(shape)) * batch, seed), self.rand(int(np.prod(ks)) * K, seed + 1)
            want = self.reference(shape, ks, batch, K, fc["mode"], fc["boundary"], o.get("zeroPad"), x, h)
            return x, h, self.in_layout(want, K, batch, fc["outputLayout"])
        return f

    # ---- direct sums in float64 (the capability tests: windows of a request whose float64 FFT reference is not worth its time) ----
    def direct_same_conv(self, x, h, shape, ks, lo, hi):
        """outputs [lo_a, hi_a) per axis of the linear-same convolution of one item: float64 or complex128, numpy order ([hi1 - lo1][hi0 - lo0])"""
        rs, rk = tuple(shape)[::-1], tuple(ks)[::-1]

        def values(a, dims):
            a = np.asarray(a, np.float64)
            if self.real:
                return a[:int(np.prod(dims))].reshape(dims)
            a = a.reshape(-1, 2)[:int(np.prod(dims))]
            return (a[:, 0] + 1j * a[:, 1]).reshape(dims)
        xc, hc = values(x, rs), values(h, rk)
        out = np.zeros([b - a for a, b in zip(lo[::-1], hi[::-1])], xc.dtype)
        for r in np.ndindex(*rk):          # y[o] = sum_r h[r] x[o + c - r], c = (M - 1) // 2
            at = [np.arange(a, b) + (m - 1) // 2 - ri for a, b, m, ri in zip(lo[::-1], hi[::-1], rk, r)]
            ok = [(v >= 0) & (v < n) for v, n in zip(at, rs)]
            blk = np.zeros_like(out)
            blk[np.ix_(*ok)] = xc[np.ix_(*(v[m] for v, m in zip(at, ok)))]
            out += hc[r] * blk
        return out


def widened(opts, x, h):
    """the complex request on the same real data with zero imaginary parts: (opts, interleaved data, interleaved kernels)"""
    o = dict(opts, layout={"interleavedComplex": True})
    xc = np.zeros(2 * x.size, np.float32)
    xc[0::2] = x
    hc = np.zeros(2 * h.size, np.float32)
    hc[0::2] = h
    return o, xc, hc


# ---- the two tiers: run(opts, x, out_floats, kernel, out_init=None) -> (got, route, launches) and setenv(name, value) ----
def emu_runner(monkeypatch):
    import emu_harness as emu

    def run(opts, x, out_floats, kernel, out_init=None):
        kernel = np.concatenate(kernel) if isinstance(kernel, list) else kernel
        return emu.run_plan(_desc(opts)[0], x, out_floats, kernel=kernel, out_init=out_init)
    return run, lambda name, value: monkeypatch.setenv("MI355_EMU_" + name, value)


def gpu_runner(fft, dev, monkeypatch):
    from test_gpu_parity import run_plan

    def run(opts, x, out_floats, kernel, out_init=None):
        got, (route, launches) = run_plan(fft, dev, opts, x, out_floats, kernel=kernel, out_init=out_init)
        return got, route, launches
    return run, lambda name, value: monkeypatch.setenv("MI355FFT_" + name, value)


def emu_planned(monkeypatch, case):
    """the emulation tier in front of an exec_contract_cases.Case: its switches set, and no skip by route: the emulator plans every case's route"""
    import emu_harness as emu
    for k, v in case.emu_env.items():
        monkeypatch.setenv("MI355_EMU_" + k, v)
    assert case.route_ok(emu.route_of(t.desc_of(case.opts)[0])[0])
