"""The tables of test_emu_fftconv_group.py and test_gpu_fftconv_group.py: fftConv.groups = G, grouped and depthwise convolution
    y[b][k] = sum_{c < Cg} x[b][g Cg + c] (*) h[k][c],   g = k // Kg, Cg = C / G, Kg = K / G
on its three kinds of route:
  group     the grouped rank-2 tile kernel, every output kernel in ONE launch (tiles-spectrum[N=64x64] tiles-conv-ols-group[N=64x64,L=L0xL1,C=c,G=g,K=k]
            and its real twin: plan.cpp emit_tiles_ols, kern_tiles.hpp fft_tiles_conv_ols_group_kernel; switch GROUP_OLS2D): 2 launches
  map       depthwise requests (Cg = 1) on the single-channel overlap-save routes through a per-kernel load map (plan.cpp push_per_kernel), the tag's last
            field ",G=g": 1 + K launches, no grouped kernel involved
  composed  fftconv-sum[K=k,C=c,G=g] / rconv-sum[K=k,C=c,G=g], the pointwise pass summing a group's channels (kern_generic.hpp pointwise_group_sum_kernel)

Layout of a request: the input holds batch * C lines, line b * C + c being channel c of item b; the kernel buffer holds K * Cg kernels, kernel (k, c) at
k * Cg + c (the [K][C / G][...] weight order); the output side is that of G = 1.

The float64 reference is fftconv_sum_cases.reference applied per group to the group's channels and kernels, stacked over k.  Bars (the project's own for
fftconv): elementwise 4e-3 / 4e-3, rel_l2 <= 1e-5 against float64, and rel_l2 <= 1e-5 against what a caller could do before the option existed: the float32
outputs of G plans with inputChannels = Cg and kernelCount = Kg on data sliced per group on the host.  Every case asserts its route tag and launch count."""
import numpy as np

import exec_contract_cases as t
import fftconv_ols_scaffold as s
import fftconv_sum_cases as sums
from fftconv_ols_scaffold import BOUNDARIES, MODES
from fftconv_sum_cases import ATOL, F64_BAR, PARITY_BAR, RTOL, ZERO_PAD, _route
from test_emu_fftconv_real import _rel

SWITCH = "GROUP_OLS2D"
SEED = 0x6C00


def group_tag(real, ks, C, G, K, P=64):
    r = "r" if real else ""
    return f"tiles-{r}spectrum[N={P}x{P}] tiles-{r}conv-ols-group[N={P}x{P},L={P - ks[0] + 1}x{P - ks[1] + 1},C={C},G={G},K={K}]"


def composed_tag(real, K, C, G):
    return f"{'rconv' if real else 'fftconv'}-sum[K={K},C={C},G={G}]"


def options(real, shape, ks, batch, C, K, G, mode="convolution", boundary="linear-same", out_layout="kernel-major", zero_pad=None):
    o = sums.options(real, shape, ks, batch, C, K, mode, boundary, out_layout, zero_pad)
    if G is not None:
        o["fftConv"]["groups"] = G
    return o


class Case:
    """kind: "group" (tag: the grouped kernel's, 2 launches), "map" (tag: (prefix, suffix) of the single-channel route's tag, 1 + K launches) or "composed";
    env: the planner switches of the case (the tier's prefix is added by setenv); a "group" case forces the grouped kernel (switch 64) unless `switch` is None"""
    def __init__(self, name, real, shape, ks, batch, C, K, G, kind="group", tag=None, mode="convolution", boundary="linear-same", out_layout="kernel-major",
                 zero_pad=None, env=None, kernel_list=False, switch="64"):
        self.name, self.real, self.shape, self.ks, self.batch, self.C, self.K, self.G = name, real, tuple(shape), tuple(ks), batch, C, K, G
        self.kind, self.mode, self.boundary, self.out_layout, self.zero_pad = kind, mode, boundary, out_layout, zero_pad
        self.env = dict(env or {})
        self.kernel_list = kernel_list
        self.Cg, self.Kg = C // G, K // G
        self.tag = tag if tag is not None else group_tag(real, ks, C, G, K) if kind == "group" else composed_tag(real, K, C, G)
        if kind == "group" and switch is not None:      # (None: the planner's own rule)
            self.env.setdefault(SWITCH, switch)

    @property
    def opts(self):
        return options(self.real, self.shape, self.ks, self.batch, self.C, self.K, self.G, self.mode, self.boundary, self.out_layout, self.zero_pad)

    def __repr__(self):
        return self.name


def group_slices(case, x, h, g):
    """the data and the kernels of group g, contiguous: [batch][Cg][n] and [Kg][Cg][kn]"""
    xg = np.asarray(x).reshape(case.batch, case.C, -1)[:, g * case.Cg:(g + 1) * case.Cg]
    hg = np.asarray(h).reshape(case.K, case.Cg, -1)[g * case.Kg:(g + 1) * case.Kg]
    return np.ascontiguousarray(xg).reshape(-1), np.ascontiguousarray(hg).reshape(-1)


def reference(case, x, h):
    """float64 [K][batch][out]: fftconv_sum_cases.reference per group, stacked over k"""
    parts = []
    for g in range(case.G):
        xg, hg = group_slices(case, x, h, g)
        parts.append(sums.reference(case.real, case.shape, case.ks, case.batch, case.Cg, case.Kg, case.mode, case.boundary, case.zero_pad, xg, hg))
    return np.concatenate(parts, axis=0)


_DATA = {}


def data(case):
    """(x, h, float64 reference flat in the plan's output layout) of a case, computed once per process and read-only"""
    if case.name not in _DATA:
        rand = _route(case.real).rand
        n, kn = int(np.prod(case.shape)), int(np.prod(case.ks))
        x, h = rand(n * case.batch * case.C, SEED + n + kn), rand(kn * case.K * case.Cg, SEED + 1 + kn)
        want = sums.in_layout(reference(case, x, h), case.out_layout)
        for a in (x, h, want):
            a.setflags(write=False)
        _DATA[case.name] = (x, h, want)
    return _DATA[case.name]


def per_group_plans(run, case, x, h, out_floats):
    """what a caller could do before the option: G plans with inputChannels = Cg and kernelCount = Kg on host-sliced data, their float32 outputs put together"""
    o = sums.options(case.real, case.shape, case.ks, case.batch, case.Cg, case.Kg, case.mode, case.boundary, case.out_layout, case.zero_pad)
    parts = []
    for g in range(case.G):
        xg, hg = group_slices(case, x, h, g)
        got = np.asarray(run(o, xg, out_floats // case.G, hg)[0], np.float32)
        parts.append(got.reshape(case.Kg, case.batch, -1) if case.out_layout == "kernel-major" else got.reshape(case.batch, case.Kg, -1).transpose(1, 0, 2))
    return sums.in_layout(np.concatenate(parts, axis=0), case.out_layout)


def assert_route(case, route, launches):
    if case.kind == "map":
        head, tail = case.tag
        assert head in route and route.strip().endswith(tail) and "-group[" not in route and "-sum[" not in route, (route, case.tag)
        assert launches == 1 + case.K, (route, launches)
    else:
        assert case.tag in route, (route, case.tag)
        assert not any(f in route for f in sums.FORBIDDEN_COMPOSED), route
        if case.kind == "group":
            assert launches == 2 and not any(f in route for f in sums.FORBIDDEN_TILES), (route, launches)
        else:
            assert "-ols" not in route, route


def check_case(run, setenv, delenv, oracle, case):
    """run(opts, x, out_floats, kernel, out_init=None) -> (got, route, launches), setenv(name, value) and delenv(name): fftconv_ols_scaffold's runners"""
    x, h, want = data(case)
    kn = int(np.prod(case.ks)) * (1 if case.real else 2)
    kernel = [h[i * kn:(i + 1) * kn] for i in range(case.K * case.Cg)] if case.kernel_list else h
    for name, value in case.env.items():
        setenv(name, value)
    got, route, launches = run(case.opts, x, want.size, kernel)
    assert_route(case, route, launches)
    got = np.asarray(got).reshape(-1)
    rel = _rel(got, want)
    print(f"{case.name} {route.strip()}: rel_l2={rel:.3e} against float64")
    oracle.assert_close_elementwise(got, want.astype(np.float32), ATOL, RTOL, f"{case.name} ({route.strip()})")
    assert rel <= F64_BAR, (route, rel)
    for name in case.env:
        delenv(name)
    before = per_group_plans(run, case, x, h, want.size)
    rel = _rel(got, before)
    print(f"{case.name} {route.strip()}: rel_l2={rel:.3e} against {case.G} plans with inputChannels={case.Cg}, kernelCount={case.Kg}")
    assert rel <= PARITY_BAR, (route, rel)
    return got


def _kind(real):
    return "real" if real else "complex"


GROUP_CASES = [
    # 1: L = 56 x 60 on the domain 158 x 104: 3 x 2 ragged tiles an image, batch 2, C = 4, K = 4, G = 2 (Cg = Kg = 2), both modes x the three linear boundaries
    *[Case(f"{_kind(real)}_150x100_k9x5_C4_K4_G2_{mode[:4]}_{boundary[7:]}", real, (150, 100), (9, 5), 2, 4, 4, 2, mode=mode, boundary=boundary)
      for real in (False, True) for mode in MODES for boundary in BOUNDARIES],
    # 2: real, the domain 158 x 134: nb_1 = 3, the last pair of every row has no partner; depthwise C = K = G = 3
    *[Case(f"real_150x130_k9x5_depthwise3_{mode[:4]}_absent_partner", True, (150, 130), (9, 5), 2, 3, 3, 3, mode=mode) for mode in MODES],
    # 3: channel multiplier 3: C = 2, K = 6, G = 2, so Kg = 3 and Cg = 1
    *[Case(f"{_kind(real)}_150x100_k9x5_C2_K6_G2_multiplier", real, (150, 100), (9, 5), 2, 2, 6, 2) for real in (False, True)],
    # 4: one tile, 17 kernels: the kernel index in the spectrum offset and in the output lane
    *[Case(f"{_kind(real)}_20x30_k9x9_depthwise17_single_tile", real, (20, 30), (9, 9), 3, 17, 17, 17, boundary="linear-full") for real in (False, True)],
    # 5: zeroPad boxes that cut tiles on both axes (read: every channel; write: the sum), correlation, batch-major lanes
    *[Case(f"{_kind(real)}_130x90_k9x9_C4_K4_G2_zero_pad", real, (130, 90), (9, 9), 2, 4, 4, 2, mode="correlation", boundary="linear-full", out_layout="batch-major",
           zero_pad=ZERO_PAD) for real in (False, True)],
]

# 7: no switch.  The rule (plan.cpp group_tiles_block) follows the measurement (profiles/fftconv_group_ab.log): the grouped kernel was ahead of both alternatives on
# every request of all four classes (depthwise / Cg > 1, complex / real), so the rule gives every grouped request inside the tile-sum route's bounds the grouped kernel
def default_case(real):
    return Case(f"{_kind(real)}_default_300x200_k9x9_depthwise4", real, (300, 200), (9, 9), 1, 4, 4, 4, switch=None, kernel_list=not real)


GROUP_CASES += [default_case(False), default_case(True)]

D3 = dict(batch=2, C=3, K=3, G=3)
MAP_CASES = [
    # depthwise C = K = G = 3, batch 2, on the six single-channel overlap-save routes and their circular forms
    *[Case(f"real_9000_k9_depthwise3_{b}", True, (9000,), (9,), kind="map", tag=("lines-rconv-ols[N=1024", ",G=3,wrap]" if b == "circular" else ",G=3]"), boundary=b, **D3)
      for b in ("linear-same", "circular")],
    # an odd line length: channels 1 and 2 start at odd f32 offsets (9001, 18002 + 9001 ...), the real line kernel's 4-byte loads and stores through the per-kernel load map
    *[Case(f"real_9001_k9_depthwise3_{b}", True, (9001,), (9,), kind="map", tag=("lines-rconv-ols[N=1024", ",G=3,wrap]" if b == "circular" else ",G=3]"), boundary=b, **D3)
      for b in ("linear-same", "circular")],
    *[Case(f"complex_17000_k9_depthwise3_{b}", False, (17000,), (9,), kind="map", tag=("lines-conv-ols[N=2048", ",G=3,wrap]" if b == "circular" else ",G=3]"), boundary=b, **D3)
      for b in ("linear-same", "circular")],
    *[Case(f"{_kind(real)}_40x36x34_k3x3x3_depthwise3_{b}", real, (40, 36, 34), (3, 3, 3), kind="map",
           tag=(f"bricks-{'r' if real else ''}conv-ols[N=16x16x16", ",G=3,wrap]" if b == "circular" else ",G=3]"), boundary=b, **D3)
      for real in (False, True) for b in ("linear-same", "circular")],
    *[Case(f"{_kind(real)}_150x130_k9x5_depthwise3_circular", real, (150, 130), (9, 5), kind="map", tag=(f"tiles-{'r' if real else ''}conv-ols[N=64x64", ",G=3,wrap]"),
           boundary="circular", **D3) for real in (False, True)],
    # the switch at 0 on case 2: the single-channel tile route (its own switch forces the 64-point tile, as in the tile tables)
    Case("real_150x130_k9x5_depthwise3_switch_0", True, (150, 130), (9, 5), kind="map", tag=("tiles-rconv-ols[N=64x64,L=56x60", ",G=3]"),
         env={SWITCH: "0", "RCONV_OLS2D": "64"}, **D3),
]

COMPOSED_CASES = [
    # kernels of 18 .. 33 points: no grouped instance; rank 1 with Cg = 2; rank 2 circular; rank 3 with Cg = 2
    *[Case(f"{_kind(real)}_200x140_k33x17_C4_K2_G2_composed", real, (200, 140), (33, 17), 1, 4, 2, 2, kind="composed") for real in (False, True)],
    *[Case(f"{_kind(real)}_1000_k31_C4_K2_G2", real, (1000,), (31,), 2, 4, 2, 2, kind="composed") for real in (False, True)],
    *[Case(f"{_kind(real)}_64x48_k5x5_C4_K4_G2_circular", real, (64, 48), (5, 5), 2, 4, 4, 2, kind="composed", boundary="circular") for real in (False, True)],
    *[Case(f"{_kind(real)}_20x12x10_k3x3x3_C4_K2_G2", real, (20, 12, 10), (3, 3, 3), 2, 4, 2, 2, kind="composed") for real in (False, True)],
]

# groups: 1 is the request without the option: (real, shape, ks, batch, C, K, boundary, switches): one tile-sum request, one composed request, one C = 1 request
G1_CASES = [
    (False, (150, 100), (9, 5), 2, 3, 2, "linear-same", {"SUM_OLS2D": "64"}),
    (True, (1000,), (31,), 2, 3, 2, "linear-same", {}),
    (False, (150, 100), (9, 5), 2, 1, 2, "linear-same", {"CONV_OLS2D": "64"}),
]


# ---- 6: strided lanes on both sides: the scaffold's STRIDED geometry, depthwise C = K = G = 2, with outputKernelStrideElements ----
STRIDED_C = STRIDED_G = 2


def strided_request(real):
    """(opts, physical input, kernels, float64 reference [K][batch][out], output floats, index arrays of the output lanes in elements)"""
    g = _route(real).strided
    shape, ks, batch, K, si, so, ioff, ooff, kst = (g[k] for k in ("shape", "ks", "batch", "K", "si", "so", "ioff", "ooff", "kst"))
    C, G = STRIDED_C, STRIDED_G
    assert K == 2
    ibs, obs = shape[-1] * si[-1] + 11, shape[-1] * so[-1] + 7
    layout = {"inputStrides": list(si), "outputStrides": list(so), "inputOffsetElements": ioff, "outputOffsetElements": ooff,
              "inputBatchStrideElements": ibs, "outputBatchStrideElements": obs}
    if real:
        opts = sums.real_opts(list(shape), list(ks), batch, K=K, boundary="linear-same", layout=layout, outputKernelStrideElements=kst, inputChannels=C, groups=G)
    else:
        opts = s.options(shape, ks, batch, K)
        opts["layout"] = dict(layout, interleavedComplex=True)
        opts["fftConv"].update(outputKernelStrideElements=kst, inputChannels=C, groups=G)
    index = np.meshgrid(*(np.arange(n) for n in shape[::-1]), indexing="ij")[::-1]
    ipos, opos = sum(i * st for i, st in zip(index, si)), sum(i * st for i, st in zip(index, so))
    width = () if real else (2,)
    key = ("strided", real)
    if key not in _DATA:
        rand = _route(real).rand
        n, kn = int(np.prod(shape)), int(np.prod(ks))
        dense, h = rand(n * batch * C, SEED + 0xA1), rand(kn * K * (C // G), SEED + 0xA2)
        phys = rand(ioff + (batch * C - 1) * ibs + int(ipos.max()) + 1, SEED + 0xA3).reshape((-1,) + width)
        for line in range(batch * C):
            phys[ioff + line * ibs + ipos] = dense.reshape((batch * C,) + shape[::-1] + width)[line]
        case = Case("strided", real, shape, ks, batch, C, K, G)
        want = reference(case, dense, h).reshape((K, batch) + shape[::-1] + width)
        phys = phys.reshape(-1)
        for a in (phys, h, want):
            a.setflags(write=False)
        _DATA[key] = (phys, h, want)
    phys, h, want = _DATA[key]
    out_elems = ooff + (K - 1) * kst + (batch - 1) * obs + int(opos.max()) + 1
    lanes = {(k, b): ooff + k * kst + b * obs + opos for k in range(K) for b in range(batch)}
    return opts, phys, h, want, out_elems * (1 if real else 2), lanes


def strided_tag(real):
    g = _route(real).strided
    return group_tag(real, g["ks"], STRIDED_C, STRIDED_G, g["K"], g["P"])


def check_strided(run, setenv, oracle, real):
    """the output starts as 777.0 everywhere and every element outside the lanes keeps it"""
    opts, phys, h, want, out_floats, lanes = strided_request(real)
    setenv(SWITCH, "64")
    sentinel = np.full(out_floats, 777.0, np.float32)
    got, route, launches = run(opts, phys, out_floats, h, sentinel)
    assert strided_tag(real) in route and launches == 2, (route, launches)
    got = np.asarray(got) if real else np.asarray(got).reshape(-1, 2)
    touched = np.zeros(len(got), bool)
    for (k, b), idx in lanes.items():
        assert not touched[idx].any(), "the lanes of the request overlap"
        touched[idx] = True
        oracle.assert_close_elementwise(got[idx].reshape(-1), want[k, b].astype(np.float32).reshape(-1), ATOL, RTOL, f"{route.strip()} kernel {k} image {b}")
        assert _rel(got[idx], want[k, b]) <= F64_BAR
    assert np.all(got[~touched] == 777.0), "stores outside the output lanes"


def strided_contract_oracle(real):
    """exec_contract_cases oracle of the strided request: NaN where the plan's contract leaves the output alone"""
    def f(oracle, o):
        _, phys, h, want, out_floats, lanes = strided_request(real)
        full = np.full(out_floats, np.nan)
        full = full if real else full.reshape(-1, 2)
        for (k, b), idx in lanes.items():
            full[idx] = want[k, b]
        return phys, h, full.reshape(-1)
    return f


def dense_oracle(real, seed):
    """exec_contract_cases oracle of a dense request against the float64 reference, in the plan's output layout"""
    def f(oracle, o):
        fc, shape, batch = o["fftConv"], o["shape"], o["batch"]
        case = Case("oracle", real, shape, fc["kernelShape"], batch, fc["inputChannels"], fc["kernelCount"], fc["groups"], mode=fc["mode"], boundary=fc["boundary"],
                    zero_pad=o.get("zeroPad"), kind="composed")
        rand = _route(real).rand
        x, h = rand(int(np.prod(shape)) * batch * case.C, seed), rand(int(np.prod(case.ks)) * case.K * case.Cg, seed + 1)
        return x, h, sums.in_layout(reference(case, x, h), fc["outputLayout"])
    return f


# ---- exec contract: guards, offsets, poisoned temp, untouched input / kernel, replay: grouped dense, grouped strided and depthwise-by-map ----
CONTRACT_CASES = [
    t.Case("group_tiles_dense_150x100_k9x5_C4_K4_G2", options(False, (150, 100), (9, 5), 2, 4, 4, 2), group_tag(False, (9, 5), 4, 2, 4), dense_oracle(False, SEED + 0xC0),
           t.TOL_CONV, env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("group_rtiles_dense_150x130_k9x5_depthwise3", options(True, (150, 130), (9, 5), 2, 3, 3, 3), group_tag(True, (9, 5), 3, 3, 3), dense_oracle(True, SEED + 0xC2),
           t.TOL_RCONV, env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("group_tiles_strided_150x100_k9x5_depthwise2", strided_request(False)[0], strided_tag(False), strided_contract_oracle(False), t.TOL_CONV,
           env={SWITCH: "64"}, starts=False, replay=True),
    t.Case("depthwise_by_map_9000_k9", options(True, (9000,), (9,), 2, 3, 3, 3), "lines-rconv-ols[N=1024", dense_oracle(True, SEED + 0xC4), t.TOL_RCONV,
           starts=False, replay=True),
]
