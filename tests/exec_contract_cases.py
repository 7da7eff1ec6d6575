"""Shared by test_gpu_exec_contract.py and test_emu_exec_contract.py: one table of route cases for the exec contract (guard bands,
exec offsets of 8 (mod 16), caller workspace of any contents, input preserved, replay, aliased c2c).

A case holds plan options, the planner switches that pin its route (names without their prefix: the GPU tier sets MI355FFT_<name>, the
emulation tier MI355_EMU_<name>), the route it must plan to, and its oracle.  data(oracle, case) computes input, kernel and the expected
output once per case and caches them; tolerances are the ones the parity tests of each route already use (TOL below names their source).

The expected output is float64 in the plan's output layout.  Where the plan's contract leaves output elements untouched (ioView.output
without clearOutside) it holds NaN, and the tests expect the poison pattern there."""
import numpy as np

import fftconv_linear_cases as lin
from emu_harness import banded  # noqa: F401  (the guard-banded host array both tiers lay their buffers out with)

GUARD_BYTES = 1 << 20           # at least one 32768-point line on either side of every buffer
POISON = 0x7FC17FC1             # a quiet NaN as f32 and as two binary16 values
REAL = {"interleavedComplex": False}

# how a result is compared with its oracle: the bars of the parity tests, by name
#   check(atol, rtol): test_gpu_parity.check (rel_l2, rel_max <= 1e-5 and elementwise atol + rtol|e|, atol scaled by rms / 64 above 64)
#   l2:                elementwise 4e-3 + 4e-3|e| and rel_l2 < 1e-5 (real fftconv: test_emu_fftconv_real.check_against_f64)
#   maxabs(f):         max|a - e| <= f * max(1, max|e|) (trig: test_dct_dst 1e-4; mapped views: test_c2c_ioview_and_zeropad 2e-5,
#                      test_r2c_c2r_ioview_and_zeropad 3e-5)
#   bluestein:         rel_l2, rel_max <= 1e-5 and elementwise 3e-4 * max(1, max|e| / 30), 3e-4 (test_gpu_parity.check_bluestein)
#   f16:               rel_l2 <= 1e-3 against float64 (test_gpu_f16_storage)
TOL_C2C = ("check", 3e-4, 3e-4)
TOL_MIXED = ("check", 3e-3, 3e-3)
TOL_R2C = ("check", 8e-4, 8e-4)
TOL_C2R = ("check", 2e-3, 2e-3)
TOL_CONV = ("check", 4e-3, 4e-3)
TOL_RCONV = ("l2",)
TOL_VIEW4 = ("check", 2e-3, 2e-3)       # test_c2c_view_of_a_four_step_line


class Case:
    def __init__(self, name, opts, route, oracle, tol, env=None, emu_env=None, replay=False, emu=True, starts=True, note=""):
        self.name, self.opts, self.oracle, self.tol = name, opts, oracle, tol
        self.route = (route,) if isinstance(route, str) else tuple(route)
        self.starts = starts                  # route[0] is a prefix of the route string (else: contained, like the rest)
        self.env = dict(env or {})
        self.emu_env = dict(self.env, **(emu_env or {}))
        self.replay = replay                  # also run the re-execution part: every route with a workspace (the GPU tier checks the flag
                                              # against getWorkspaceSizeBytes()) and one plain line route
        self.emu = emu                        # False: too long under emulation (the 2^20 .. 2^22 cases)
        self.note = note

    @property
    def type(self):
        return self.opts["type"]

    @property
    def f16(self):
        return self.opts.get("precision") == "f16-storage"

    @property
    def in_place(self):
        return bool(self.opts.get("inPlace"))

    def route_ok(self, route):
        first = route.startswith(self.route[0]) if self.starts else self.route[0] in route
        return first and all(r in route for r in self.route[1:])

    def __repr__(self):
        return self.name


def desc_of(opts):
    """(PlanDesc, resolved options) as mi355fft.Plan builds them"""
    from mi355fft import _abi
    from mi355fft.layout import resolve_plan_options
    r = resolve_plan_options(opts)
    return _abi.make_desc(r.get("abi_type", r["type"]), r["shape"], r["batch"], r["direction"], r["normalize"], r["inPlace"], r["input_layout"],
                          r["output_layout"], r.get("conv"), r.get("io_view"), r.get("zero_pad"), r.get("axes"), r.get("precision", "f32")), r


# ---- oracles: (x, kernel, want) ---------------------------------------------------------------------------------------------------
def _c2c(seed):
    def f(oracle, o):
        shape, batch = o["shape"], o["batch"]
        n = int(np.prod(shape))
        x = oracle.random_complex_batch(n, batch, seed).reshape(-1)
        if len(shape) == 1 and n >= 10000 and n & (n - 1):     # the O(N^2) oracle is infeasible: an independent float64 FFT
            c = x.astype(np.float64).view(np.complex128).reshape(batch, n)
            w = np.fft.fft(c, axis=1) if o["direction"] == "forward" else np.fft.ifft(c, axis=1) * n
            inverse = o["direction"] == "inverse"
            w = w * {"none": 1.0, "unitary": 1.0 / np.sqrt(n), "backward": 1.0 / n if inverse else 1.0}[o.get("normalize", "none")]
            return x, None, np.stack([w.real, w.imag], axis=-1).reshape(-1)
        return x, None, oracle.c2c_ref_batch(x, shape, batch, o["direction"], o.get("normalize", "none"))
    return f


def _c2c_view(seed):
    """N-D c2c with ioView / zeroPad against the numpy restatement of test_emu_ioview; NaN where the output keeps its contents"""
    def f(oracle, o):
        from mi355fft.layout import resolve_plan_options
        from test_emu_ioview import reference
        r = resolve_plan_options(o)
        vin, vout = r["io_view"]["input"], r["io_view"]["output"]
        in_n = int(np.prod(vin["shape"] if vin else o["shape"]))
        out_n = int(np.prod(vout["shape"] if vout else o["shape"]))
        x = oracle.random_complex_interleaved(in_n * o["batch"], seed)
        keep = np.full(2 * out_n * o["batch"], np.nan, np.float32)
        want = reference(oracle, x, o["shape"], o["batch"], o["direction"], o.get("normalize", "none"), vin, vout, r["zero_pad"]["read"],
                         r["zero_pad"]["write"], keep)
        return x, None, np.asarray(want, np.float64)
    return f


def _c2c_view_rank1(seed):
    """the case of test_c2c_view_of_a_four_step_line, its reference written out for one line length"""
    def f(oracle, o):
        n, batch = o["shape"][0], o["batch"]
        vin, vout, zr, zw = o["ioView"]["input"], o["ioView"]["output"], o["zeroPad"]["read"], o["zeroPad"]["write"]
        rng = np.random.default_rng(seed)
        x = rng.standard_normal(2 * vin["shape"][0] * batch).astype(np.float32)
        logical = np.zeros((batch, n, 2), np.float32)
        logical[:, vin["offset"][0]:vin["offset"][0] + vin["shape"][0]] = x.reshape(batch, -1, 2)
        logical[:, :zr["start"][0]] = 0
        logical[:, zr["end"][0]:] = 0
        y = oracle.c2c_ref_batch(logical.reshape(-1), [n], batch, o["direction"], o.get("normalize", "none")).reshape(batch, n, 2).astype(np.float64)
        y[:, :zw["start"][0]] = 0
        y[:, zw["end"][0]:] = 0
        want = np.full((batch, vout["shape"][0], 2), 0.0 if vout.get("clearOutside") else np.nan)
        lead = -vout["offset"][0]
        want[:, lead:] = y[:, :vout["shape"][0] - lead]
        return x, None, want.reshape(-1)
    return f


def _r2c(seed):
    def f(oracle, o):
        shape, batch = o["shape"], o["batch"]
        n = int(np.prod(shape))
        x = oracle.random_real_batch(n, batch, seed).reshape(-1)
        if len(shape) == 1:
            pow2 = n & (n - 1) == 0
            want = np.concatenate([oracle.r2c_ref_packed(x[b * n:(b + 1) * n], n, o.get("normalize", "none"), use_pow2=pow2) for b in range(batch)])
        else:       # the full complex oracle, its first shape[0] / 2 + 1 bins along axis 0 (test_r2c_c2r_2d_real_images)
            cplx = np.zeros(2 * n * batch, np.float32)
            cplx[0::2] = x
            full = oracle.c2c_ref_batch(cplx, shape, batch, "forward", o.get("normalize", "none")).reshape(batch, n // shape[0], shape[0], 2)
            want = np.ascontiguousarray(full[:, :, :shape[0] // 2 + 1, :]).reshape(-1)
        return x, None, want
    return f


def _c2r(seed):
    """the oracle's own spectrum of a seeded signal in, the signal out (the round trip the parity tests hold to 2e-3)"""
    def f(oracle, o):
        n, batch = o["shape"][0], o["batch"]
        sig = oracle.random_real_batch(n, batch, seed).reshape(-1)
        pow2 = n & (n - 1) == 0
        spec = np.concatenate([oracle.r2c_ref_packed(sig[b * n:(b + 1) * n], n, "none", use_pow2=pow2) for b in range(batch)])
        return spec, None, sig
    return f


def _c2r_view(seed):
    """c2r of a low-passed spectrum into a window of a larger real array (test_r2c_c2r_ioview_and_zeropad); NaN outside the window"""
    def f(oracle, o):
        n, batch = o["shape"][0], o["batch"]
        bins, on, lead = o["ioView"]["input"]["shape"][0], o["ioView"]["output"]["shape"][0], -o["ioView"]["output"]["offset"][0]
        sig = oracle.random_real_batch(n, batch, seed).reshape(-1)
        spec = np.concatenate([oracle.r2c_ref_packed(sig[b * n:(b + 1) * n], n, "none") for b in range(batch)]).reshape(batch, n // 2 + 1, 2)
        low = np.ascontiguousarray(spec[:, :bins, :]).reshape(-1)
        spec = spec.copy()
        spec[:, bins:, :] = 0
        want = np.full((batch, on), np.nan)
        for b in range(batch):
            want[b, lead:lead + n] = oracle.c2r_ref_from_packed(spec[b].reshape(-1), n, o.get("normalize", "none"))
        return low, None, want.reshape(-1)
    return f


def _trig(seed):
    def f(oracle, o):
        n = int(np.prod(o["shape"]))
        x = oracle.random_real_batch(n, o["batch"], seed).reshape(-1)
        return x, None, oracle.trig_ref_batch(x, o["shape"], o["batch"], o["type"], o["direction"], o.get("normalize", "none"))
    return f


def _conv(seed):
    """complex fftconv, kernel-major, against the oracle's fftConvRef restatement (test_fftconv_product_fused_into_forward_lines)"""
    def f(oracle, o):
        fc, shape, batch = o["fftConv"], o["shape"], o["batch"]
        ks, K = fc.get("kernelShape"), fc["kernelCount"]
        n, kn = int(np.prod(shape)), int(np.prod(ks or shape))
        x = oracle.random_complex_interleaved(n * batch, seed)
        kern = oracle.random_complex_interleaved(kn * K, seed + 1)
        pow2 = len(shape) == 1 and fc.get("boundary", "circular") == "circular" and n & (n - 1) == 0 and n > 4096
        extra = {"use_pow2": True} if pow2 else {}
        want = np.concatenate([oracle.fftconv_ref(x, kern[2 * k * kn:2 * (k + 1) * kn], shape, batch, fc.get("mode", "convolution"),
                                                  fc.get("boundary", "circular"), ks, **extra)[0] for k in range(K)])
        return x, kern, want
    return f


def _conv_linear(case, seed):
    """a long rank-1 request of fftconv_linear_cases.py against that module's reference"""
    def f(oracle, o):
        n, kn, K, batch = case[0], case[1], case[4], o["batch"]
        x = oracle.random_complex_interleaved(n * batch, seed)
        kern = oracle.random_complex_interleaved(kn * K, seed + 1)
        want = lin.want_for(oracle, case, x, kern, batch)                      # [K][batch][on][2]
        if case[5] != "kernel-major":
            want = want.transpose(1, 0, 2, 3)
        return x, kern, np.ascontiguousarray(want).reshape(-1)
    return f


def _rconv(seed):
    """real fftconv against the float64 reference of test_emu_fftconv_real"""
    def f(oracle, o):
        from test_emu_fftconv_real import _rand, _want
        fc, shape, batch = o["fftConv"], o["shape"], o["batch"]
        ks, K = fc["kernelShape"], fc["kernelCount"]
        x, h = _rand(int(np.prod(shape)) * batch, seed), _rand(int(np.prod(ks)) * K, seed + 1)
        want = _want(x, h, shape, ks, batch, K, fc["mode"], fc["boundary"], o.get("zeroPad"))
        want = want.reshape(K, batch, -1)
        if fc.get("outputLayout", "kernel-major") != "kernel-major":
            want = want.transpose(1, 0, 2)
        return x, h, np.ascontiguousarray(want).reshape(-1)
    return f


def _f16(seed):
    """f16-storage: binary16 input, float64 numpy transform of the decoded input (bar: rel_l2 <= 1e-3)"""
    def f(oracle, o):
        n, batch = o["shape"][0], o["batch"]
        rng = np.random.default_rng(seed)
        if o["type"] == "c2r":      # a scaled spectrum of real noise in, its float64 inverse out (test_c2r_fused)
            spec = np.fft.rfft(rng.standard_normal((batch, n)), axis=1) / np.sqrt(n)
            x = np.stack([spec.real, spec.imag], -1).reshape(-1).astype(np.float16)
            c = x.astype(np.float64).reshape(batch, n // 2 + 1, 2)
            return x, None, np.fft.irfft(c[..., 0] + 1j * c[..., 1], n=n, axis=1).reshape(-1)
        if o["type"] == "r2c":
            x = rng.standard_normal(n * batch).astype(np.float16)
            w = np.fft.rfft(x.astype(np.float64).reshape(batch, n), axis=1)
            return x, None, np.stack([w.real, w.imag], axis=-1).reshape(-1)
        view = o.get("ioView")
        in_n = view["input"]["shape"][0] if view else n
        x = rng.standard_normal(2 * in_n * batch).astype(np.float16)
        c = x.astype(np.float64).reshape(batch, in_n, 2)
        logical = np.zeros((batch, n), np.complex128)
        ioff = view["input"]["offset"][0] if view else 0
        logical[:, ioff:ioff + in_n] = c[..., 0] + 1j * c[..., 1]
        w = np.fft.fft(logical, axis=1)
        if not view:
            return x, None, np.stack([w.real, w.imag], axis=-1).reshape(-1)
        on, lead = view["output"]["shape"][0], -view["output"]["offset"][0]
        want = np.full((batch, on, 2), np.nan)
        m = min(on - lead, n)
        want[:, lead:lead + m, 0], want[:, lead:lead + m, 1] = w[:, :m].real, w[:, :m].imag
        return x, None, want.reshape(-1)
    return f


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _o(type_, shape, batch, direction="forward", normalize="none", **kw):
    return dict({"type": type_, "shape": list(shape), "batch": batch, "direction": direction, "normalize": normalize}, **kw)


def _fc(shape, batch, ks, K, boundary="circular", mode="convolution", layout="kernel-major"):
    return {"type": "fftconv", "shape": list(shape), "batch": batch,
            "fftConv": {"mode": mode, "boundary": boundary, "kernelCount": K, "kernelShape": ks, "outputLayout": layout}}


def _rc(shape, ks, batch, K=1, mode="convolution", boundary="circular", layout="kernel-major"):
    return dict(_fc(shape, batch, list(ks), K, boundary, mode, layout), layout=dict(REAL))


FOUR_STEP = {"MAX_LINE": "4096", "LINE32K": "0"}       # as test_c2c_two_pass: keep 2^13 .. 2^15 off the single-workgroup lines
FUSED = {"XCD_FUSED": "1"}                             # (the emulator plans with xcd_fused = 0 unless told)
VIEW17 = {"input": {"shape": [(1 << 17) - 3000], "offset": [1000]}, "output": {"shape": [(1 << 16) + 77], "offset": [-50], "clearOutside": False}}
ZERO17 = {"read": {"start": [5000], "end": [(1 << 17) - 100]}, "write": {"start": [64], "end": [(1 << 16) - 5]}}
VIEW_ND = {"input": {"shape": [40, 8], "placement": "center"}, "output": {"shape": [80, 10], "placement": "center", "clearOutside": True}}
ZERO_ND = {"read": {"start": [4, 0], "end": [60, 8]}, "write": {"start": [0, 1], "end": [64, 7]}}
PIPE_VIEW = lin.PIPELINE_CASES["valid_corr_short_filter"]      # the smallest of that table: 700000 + 1000 points a line, K = 1
PADDED = lin.COMPOSED_CASES["full_corr_32999"]                 # pad[32999->65536]

CASES = [
    # c2c power-of-two lines
    Case("lines64", _o("c2c", [64], 37), "lines[N=64]", _c2c(0xEC01), TOL_C2C, replay=True),
    Case("lines64_in_place", _o("c2c", [64], 37, "inverse", "backward", inPlace=True), "lines[N=64]", _c2c(0xEC02), TOL_C2C),
    Case("lines4096", _o("c2c", [4096], 5, "inverse", "unitary"), "lines[N=4096]", _c2c(0xEC03), TOL_C2C),
    Case("line_reg8192", _o("c2c", [8192], 3), "line-reg[N=8192]", _c2c(0xEC04), TOL_C2C),
    Case("lines16384", _o("c2c", [16384], 3, "inverse", "backward"), "lines[N=16384]", _c2c(0xEC05), TOL_C2C),
    Case("line32k", _o("c2c", [1 << 15], 3), "line32k[N=32768]", _c2c(0xEC06), TOL_C2C),
    # c2c fused and four-step
    Case("xcd_solo_2p16", _o("c2c", [1 << 16], 3, "forward", "backward"), "xcd-solo[", _c2c(0xEC10), TOL_C2C, emu_env=FUSED, replay=True),
    Case("xcd_fused_2p17", _o("c2c", [1 << 17], 3, "inverse", "backward"), "xcd-fused[", _c2c(0xEC11), TOL_C2C, emu_env=FUSED, replay=True),
    Case("xcd_fused_rt32_2p20", _o("c2c", [1 << 20], 2), "xcd-fused-rt32[", _c2c(0xEC12), TOL_C2C, replay=True, emu=False),
    Case("xcd_fused_rt_2p22", _o("c2c", [1 << 22], 1), "xcd-fused-rt[", _c2c(0xEC13), TOL_C2C, replay=True, emu=False),
    Case("two_pass_2p17", _o("c2c", [1 << 17], 3), "two-pass[", _c2c(0xEC14), TOL_C2C, env={"XCD_FUSED": "0"}, replay=True),
    Case("xcd_fused_view_2p17", _o("c2c", [1 << 17], 3, ioView=VIEW17, zeroPad=ZERO17), "xcd-fused-view[N=", _c2c_view_rank1(0xEC15), TOL_VIEW4,
         env={"FUSE_VIEWS": "1"}, emu_env=FUSED, replay=True, starts=False),
    Case("xcd_2d_256x256", _o("c2c", [256, 256], 3, "inverse", "backward"), "xcd-2d-solo[", _c2c(0xEC16), TOL_C2C, env={"XCD_2D": "1"}, emu_env=FUSED, replay=True,
         note="one workgroup per plane, no control block"),
    Case("xcd_2d_512x512", _o("c2c", [512, 512], 3, "forward", "unitary"), "xcd-2d[512x512]", _c2c(0xEC17), TOL_C2C, env={"XCD_2D": "1"}, emu_env=FUSED, replay=True,
         note="the persistent form: control-block reset + launch"),
    # c2c N-D
    Case("columns_64x64x4", _o("c2c", [64, 64, 4], 2, "forward", "unitary"), ("lines[N=64]", "columns[N=64,S=64]"), _c2c(0xEC20), TOL_MIXED,
         note="tolerance of test_c2c_nd"),
    Case("columns_ragged_r2c_64x64x8", _o("r2c", [64, 64, 8], 3), "columns-ragged[", _r2c(0xEC21), TOL_R2C, starts=False, replay=True),
    Case("lines_columns_mapped", _o("c2c", [64, 8], 3, "forward", "unitary", ioView=VIEW_ND, zeroPad=ZERO_ND),
         ("lines-mapped[N=64]", "columns-mapped[N=8,S=64]"), _c2c_view(0xEC22), ("maxabs", 2e-5), env={"FUSE_VIEWS": "1"}, replay=True),
    # c2c mixed radix
    Case("mixed_ct96", _o("c2c", [96], 37, "forward", "unitary"), "mixed-ct[N=96,", _c2c(0xEC30), TOL_MIXED),
    Case("mixed_ct1000", _o("c2c", [1000], 7, "inverse", "backward"), "mixed-ct[N=1000,", _c2c(0xEC31), TOL_MIXED),
    Case("mixed_lines1001", _o("c2c", [1001], 5), "mixed-lines[", _c2c(0xEC32), TOL_MIXED, env={"MIXED_LINES": "2", "MIXED_CT": "0"}),
    Case("stages_3x4096", _o("c2c", [3 * 4096], 3, "inverse", "backward"), "stages[", _c2c(0xEC33), TOL_MIXED, env={"MIXED_CT": "0"}, replay=True),
    # c2c Bluestein
    Case("bluestein_lines17", _o("c2c", [17], 37), "bluestein-lines[", _c2c(0xEC40), ("bluestein",), env={"FUSE_VIEWS": "1"}, replay=True),
    Case("bluestein_lines2039", _o("c2c", [2039], 3, "inverse", "backward"), "bluestein-lines[", _c2c(0xEC41), ("bluestein",), env={"FUSE_VIEWS": "1"}, replay=True),
    Case("bluestein100003", _o("c2c", [100003], 1), "bluestein[", _c2c(0xEC42), ("bluestein",), starts=False, replay=True),
    # real transforms
    Case("lines_r2c256", _o("r2c", [256], 37), "lines-r2c[N=", _r2c(0xEC50), TOL_R2C),
    Case("lines_c2r256", _o("c2r", [256], 37, "inverse", "backward"), "lines-c2r[N=", _c2r(0xEC51), TOL_C2R),
    Case("lines_r2c_2p15", _o("r2c", [1 << 15], 3), "lines-r2c[N=", _r2c(0xEC52), TOL_R2C),
    Case("lines_c2r_2p15", _o("c2r", [1 << 15], 3, "inverse", "backward"), "lines-c2r[N=", _c2r(0xEC53), TOL_C2R),
    Case("xcd_r2c_2p17", _o("r2c", [1 << 17], 3), "xcd-r2c[N=", _r2c(0xEC54), TOL_R2C, emu_env=FUSED, replay=True),
    Case("xcd_c2r_2p17", _o("c2r", [1 << 17], 3, "inverse", "backward"), "xcd-c2r-solo[", _c2r(0xEC55), TOL_C2R, emu_env=FUSED, replay=True,
         note="one workgroup per transform, no control block"),
    Case("xcd_c2r_2p18", _o("c2r", [1 << 18], 3, "inverse", "backward"), "xcd-c2r[N=", _c2r(0xEC5D), TOL_C2R, emu_env=FUSED, replay=True,
         note="the persistent form: control-block reset + launch"),
    Case("xcd_r2c_rt_2p21", _o("r2c", [1 << 21], 1), "xcd-r2c-rt[", _r2c(0xEC56), TOL_R2C, replay=True, emu=False),
    Case("xcd_c2r_rt_2p21", _o("c2r", [1 << 21], 1, "inverse", "backward"), "xcd-c2r-rt[", _c2r(0xEC57), TOL_C2R, replay=True, emu=False),
    Case("lines_c2r_mapped4096", _o("c2r", [4096], 3, "inverse", "backward", ioView={"input": {"shape": [300]}, "output": {"shape": [5000], "offset": [-100]}}),
         "lines-c2r-mapped[N=4096]", _c2r_view(0xEC5C), ("maxabs", 3e-5), env={"FUSE_VIEWS": "1"}),
    Case("r2c_split30", _o("r2c", [30], 37), "r2c-split", _r2c(0xEC58), TOL_R2C, starts=False, replay=True),
    Case("c2r_split30", _o("c2r", [30], 37, "inverse", "backward"), "c2r-split", _c2r(0xEC59), TOL_C2R, starts=False, replay=True),
    Case("r2c_odd21", _o("r2c", [21], 37), ("mixed-lines[N=21,", "r2c-full"), _r2c(0xEC5A), TOL_R2C, replay=True, note="odd length: full complex transform, then the packed half"),
    Case("c2r_odd21", _o("c2r", [21], 37, "inverse", "backward"), ("mixed-lines[N=21,", "c2r-full"), _c2r(0xEC5B), TOL_C2R, replay=True, note="odd length"),
    # trig
    Case("lines_dct2_256", _o("dct2", [256], 5, layout=dict(REAL)), "lines-dct2[N=256]", _trig(0xEC60), ("maxabs", 1e-4)),
    Case("lines_dst3_256", _o("dst3", [256], 5, layout=dict(REAL)), "lines-dst3[N=256]", _trig(0xEC61), ("maxabs", 1e-4)),
    Case("trig_real_dct4_256", _o("dct4", [256], 5, layout=dict(REAL)), "trig-real[", _trig(0xEC62), ("maxabs", 1e-4), replay=True),
    Case("trig_real_dct1_257", _o("dct1", [257], 5, layout=dict(REAL)), "trig-real[", _trig(0xEC63), ("maxabs", 1e-4), replay=True,
         note="dct1: the extension 2(N - 1) = 512 is the power of two"),
    Case("trig_dct2_17", _o("dct2", [17], 5, layout=dict(REAL)), "trig[", _trig(0xEC64), ("maxabs", 1e-4), starts=False, replay=True),
    # fftconv
    Case("fftconv_fused64", _fc([64], 37, None, 2), "fftconv-fused", _conv(0xEC70), TOL_CONV, starts=False),
    Case("lines_mul8192", _fc([8192], 3, None, 2), "lines-mul[", _conv(0xEC71), TOL_CONV, starts=False, replay=True),
    Case("lines_mul_mapped100", _fc([100], 3, [29], 3, boundary="linear-full"), "lines-mul-mapped[", _conv(0xEC79), TOL_CONV, starts=False, replay=True),
    Case("fftconv_pipeline_2p20", _fc([1 << 20], 2, None, 1), "fftconv-pipeline[N=1024x1024,K=1]", _conv(0xEC72), TOL_CONV, starts=False,
         replay=True, emu=False),
    Case("fftconv_pipeline_view", lin.options(PIPE_VIEW, 2), "fftconv-pipeline-view[N=1024x1024,K=1]", _conv_linear(PIPE_VIEW, 0xEC73), TOL_CONV,
         starts=False, replay=True, emu=False),
    Case("fftconv_padded_domain", lin.options(PADDED, 2), "pad[32999->65536]", _conv_linear(PADDED, 0xEC74), TOL_CONV, starts=False, replay=True),
    Case("fftconv_nd_circular", _fc([32, 16], 3, None, 2, mode="correlation"), ("lines[N=32]", "mixed-lines[N=16,S=32,", "fftconv[K=2]"), _conv(0xEC75), TOL_CONV, replay=True,
         note="composed: forward, pointwise, inverse per axis"),
    Case("lines_rconv128", _rc([128], [128], 37), ("lines-rconv[N=128]", "lines-r2c-mapped[N=128]"), _rconv(0xEC76), TOL_RCONV, starts=False, replay=True),
    Case("rconv_rank2", _rc([64, 48], [5, 3], 5, K=2, boundary="linear-same", layout="batch-major"), "rconv[K=2]", _rconv(0xEC77), TOL_RCONV,
         starts=False, replay=True),
    Case("rconv_widened1001", _rc([1001], [77], 5, K=2, mode="correlation"), "rconv-widened", _rconv(0xEC78), TOL_RCONV, starts=False, replay=True),
    # f16-storage
    Case("f16_lines256", _o("c2c", [256], 37, precision="f16-storage"), ("lines[N=256]", " f16"), _f16(0xEC80), ("f16",)),
    Case("f16_lines_r2c256", _o("r2c", [256], 37, precision="f16-storage"), ("lines-r2c[N=", " f16"), _f16(0xEC81), ("f16",)),
    Case("f16_lines_c2r256", _o("c2r", [256], 37, "inverse", "backward", precision="f16-storage"), ("lines-c2r[N=", " f16"), _f16(0xEC84), ("f16",)),
    Case("f16_staged1000", _o("c2c", [1000], 7, precision="f16-storage"), ("f16-in ", "f16-out"), _f16(0xEC82), ("f16",), replay=True),
    Case("f16_keep_outside", _o("c2c", [1024], 5, precision="f16-storage",
                                ioView={"input": {"shape": [700], "offset": [100]}, "output": {"shape": [1100], "offset": [-30], "clearOutside": False}}),
         ("f16-in+out", "f16-out"), _f16(0xEC83), ("f16",), replay=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_DATA = {}


def data(oracle, case):
    """(x, kernel or None, want float64, untouched mask) of a case, computed once per process and read-only"""
    if case.name not in _DATA:
        x, kern, want = case.oracle(oracle, case.opts)
        x = np.ascontiguousarray(x)
        want = np.asarray(want, np.float64).reshape(-1)
        keep = np.isnan(want)
        for a in (x, kern, want, keep):
            if a is not None:
                a.setflags(write=False)
        _DATA[case.name] = (x, None if kern is None else np.ascontiguousarray(kern, np.float32), want, keep)
    return _DATA[case.name]


def out_dtype(case):
    return np.float16 if case.f16 else np.float32


def compare(oracle, case, got, want, keep, what):
    """the oracle bar of the case on the elements the plan writes; NaN anywhere in them fails every form"""
    a = np.asarray(got)[~keep]
    e = want[~keep]
    assert not np.isnan(a.astype(np.float32)).any(), f"{what}: NaN in the output"
    kind = case.tol[0]
    if kind == "f16":
        rel = float(np.linalg.norm(a.astype(np.float64) - e) / np.linalg.norm(e))
        assert rel <= 1e-3, f"{what}: rel_l2={rel:.3e}"
        return
    a = a.astype(np.float32)
    if kind == "maxabs":
        err = float(np.max(np.abs(a.astype(np.float64) - e)))
        assert err <= case.tol[1] * max(1.0, float(np.max(np.abs(e)))), f"{what}: max abs error {err:.3e}"
        return
    if kind == "bluestein":
        from test_gpu_parity import check_bluestein
        check_bluestein(oracle, a, e, what)
    elif kind == "l2":
        from test_emu_fftconv_real import check_against_f64
        check_against_f64(a, e, what)
    else:
        from test_gpu_parity import check
        assert kind == "check"
        check(oracle, a, e, what, case.tol[1], case.tol[2])


def poison_words(nbytes):
    assert nbytes % 4 == 0
    return np.full(nbytes // 4, POISON, np.uint32)


def assert_untouched(got_bytes, keep, case, what):
    """elements the contract leaves alone still hold the poison pattern, compared as bits"""
    if not keep.any():
        return
    width = 2 if case.f16 else 4
    raw = np.asarray(got_bytes).view(np.uint16 if case.f16 else np.uint32)[:keep.size]
    expect = POISON & 0xFFFF if width == 2 else POISON
    assert np.all(raw[keep] == expect), f"{what}: {int(np.count_nonzero(raw[keep] != expect))} elements outside the plan's stores were written"
