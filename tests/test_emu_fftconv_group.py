"""CPU tier: fftConv.groups, grouped and depthwise convolution, under host emulation.

The tables and their bars are fftconv_group_cases.py's, shared with the GPU tier: the grouped rank-2 tile kernel (every output kernel in one launch, complex
and real), depthwise requests on the single-channel overlap-save routes through the per-kernel load map, and the composed routes, against float64 references
per group and against the float32 outputs of the G per-group plans a caller had to run before; strided lanes on both sides; the grouped kernel against the
switch at 0; groups = 1 as the request without the option (same route, same launches, the same bits); the planner alone on the switch, its neighbours and its
bad values; validation; the descriptor word; the kernel lists (which entry each class of request plans, its slots and work items; their lengths, threads and LDS
bytes: test_emu_fftconv_group_asan.py); the length errors of Plan.exec's kernel argument; and the exec contract (test_emu_exec_contract.py's harness)."""
import re

import numpy as np
import pytest

import emu_harness as emu
import fftconv_group_cases as groups
import fftconv_ols_scaffold as scaffold
import fftconv_sum_cases as sums
import test_emu_exec_contract as contract
from mi355fft.layout import resolve_plan_options
from test_emu_fftconv_real import _desc, _rel


def _runner(monkeypatch):
    run, setenv = scaffold.emu_runner(monkeypatch)
    return run, setenv, lambda name: monkeypatch.delenv("MI355_EMU_" + name, raising=False)


@pytest.mark.parametrize("case", groups.GROUP_CASES + groups.MAP_CASES + groups.COMPOSED_CASES, ids=repr)
def test_grouped_and_depthwise(oracle, monkeypatch, case):
    groups.check_case(*_runner(monkeypatch), oracle, case)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_strided_lanes_on_both_sides(oracle, monkeypatch, real):
    groups.check_strided(*scaffold.emu_runner(monkeypatch), oracle, real)


@pytest.mark.parametrize("name", ["complex_150x100_k9x5_C4_K4_G2_conv_same", "real_150x130_k9x5_depthwise3_conv_absent_partner"])
def test_the_grouped_kernel_agrees_with_the_switch_at_0(monkeypatch, name):
    """GROUP_OLS2D = 0 (Cg > 1: the composed route; depthwise: the single-channel tile route through the load map) against the grouped kernel, rel_l2 <= 1e-5"""
    run, setenv = scaffold.emu_runner(monkeypatch)
    case = next(c for c in groups.GROUP_CASES if c.name == name)
    x, h, want = groups.data(case)
    setenv(groups.SWITCH, "64")
    one, route, launches = run(case.opts, x, want.size, h)
    setenv(groups.SWITCH, "0")
    if case.Cg == 1:
        setenv("RCONV_OLS2D" if case.real else "CONV_OLS2D", "64")
    other, route0, launches0 = run(case.opts, x, want.size, h)
    assert case.tag in route and launches == 2 and "-group[" not in route0, (route, route0)
    assert (f",G={case.G}]" in route0 and launches0 == 1 + case.K) if case.Cg == 1 else groups.composed_tag(case.real, case.K, case.C, case.G) in route0, (route0, launches0)
    rel = _rel(one, other)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= groups.PARITY_BAR


@pytest.mark.parametrize("real,shape,ks,batch,C,K,boundary,env", groups.G1_CASES, ids=lambda v: None)
def test_one_group_is_the_request_without_the_option(monkeypatch, real, shape, ks, batch, C, K, boundary, env):
    run, setenv = scaffold.emu_runner(monkeypatch)
    for name, value in env.items():
        setenv(name, value)
    rand = sums._route(real).rand
    x, h = rand(int(np.prod(shape)) * batch * C, 0x6C11), rand(int(np.prod(ks)) * K * C, 0x6C12)
    out_floats = int(np.prod(shape)) * batch * K * (1 if real else 2)
    plain = run(groups.options(real, shape, ks, batch, C, K, None, boundary=boundary), x, out_floats, h)
    one = run(groups.options(real, shape, ks, batch, C, K, 1, boundary=boundary), x, out_floats, h)
    assert plain[1:] == one[1:], (plain[1:], one[1:])
    assert "G=" not in one[1] and "-group" not in one[1], one[1]
    assert np.array_equal(np.asarray(plain[0]).view(np.uint32), np.asarray(one[0]).view(np.uint32))


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(real, shape, ks, batch, C, K, G, boundary="linear-same", **kw):
    return emu.plan_only(_desc(groups.options(real, shape, ks, batch, C, K, G, boundary=boundary, **kw))[0])


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_the_switch_and_the_neighbours(monkeypatch, real):
    tag, r = "conv-ols-group[", "r" if real else ""
    sw = "MI355FFT_GROUP_OLS2D"
    monkeypatch.setenv(sw, "64")
    route, launches, work = _plan(real, (300, 200), (9, 9), 2, 8, 8, 4)
    assert groups.group_tag(real, (9, 9), 8, 4, 8) in route and launches == 2, (route, launches)
    assert 8 * 2 * 64 * 64 * 8 <= work < 1 << 20, work                   # the K Cg kernel spectra alone
    assert groups.group_tag(real, (9, 9), 17, 17, 17) in _plan(real, (20, 30), (9, 9), 3, 17, 17, 17, boundary="linear-full")[0]
    assert groups.group_tag(real, (63, 3), 2, 2, 4) in _plan(real, (70, 200), (63, 3), 1, 2, 4, 2)[0]      # every request the tile fits, L >= 2
    assert tag not in _plan(real, (70, 200), (64, 3), 1, 2, 4, 2)[0]
    assert tag not in _plan(real, (256, 256), (9, 9), 2, 2, 2, 2, boundary="circular")[0]                  # circular grouped instances do not exist
    assert tag not in _plan(real, (300, 200), (9, 9), 2, 8, 8, 1)[0]                                       # G = 1 is not a grouped request
    # 0 and every value that is neither 1 nor 64: no grouped kernel; Cg > 1 composed, depthwise on the single-channel route through the load map
    for bad in ("0", "32", "128", "2", "-1"):
        monkeypatch.setenv(sw, bad)
        route, launches, _ = _plan(real, (300, 200), (9, 9), 2, 8, 8, 4)
        assert tag not in route and groups.composed_tag(real, 8, 8, 4) in route, (bad, route)
        route, launches, _ = _plan(real, (300, 200), (9, 9), 2, 4, 8, 4)
        assert tag not in route and f"tiles-{r}conv-ols[N=64x64,L=56x56,G=4]" in route and launches == 9, (bad, route, launches)
    # the switches in front of the single-channel tile route come first
    monkeypatch.setenv(sw, "64")
    for name, value in ((("MI355FFT_RCONV_OLS2D", "0"), ("MI355FFT_RCONV_FUSED", "0")) if real else (("MI355FFT_CONV_OLS2D", "0"), ("MI355FFT_CONV_LINES", "0"))) + \
            (("MI355FFT_FORCE_GENERIC", "1"),):
        monkeypatch.setenv(name, value)
        route = _plan(real, (300, 200), (9, 9), 2, 8, 8, 4)[0]
        assert tag not in route and groups.composed_tag(real, 8, 8, 4) in route, (name, route)
        monkeypatch.delenv(name)
    monkeypatch.delenv(sw)
    # Cg > 1 outside rank 2: composed; the other single-channel routes stay out with C > 1, depthwise or not
    for shape, ks in (((100000,), (9,)), ((100, 80, 70), (5, 5, 5))):
        route = _plan(real, shape, ks, 2, 4, 2, 2)[0]
        assert groups.composed_tag(real, 2, 4, 2) in route and "-ols[" not in route, route
    route = _plan(real, (1000,), (31,), 2, 3, 3, 3)[0]
    assert groups.composed_tag(real, 3, 3, 3) in route and not any(f in route for f in ("lines-mul", "lines-rconv[", "fftconv-fused", "pipeline")), route
    # and G = 1 plans what the request without the option plans
    for shape, ks, C in (((300, 200), (9, 9), 4), ((100000,), (9,), 1), ((1000,), (31,), 3), ((100, 80, 70), (5, 5, 5), 1)):
        assert _plan(real, shape, ks, 2, C, 2, 1) == _plan(real, shape, ks, 2, C, 2, None), (shape, ks)


def _steps(desc):
    """the steps of the product planner's PlanIR (emu_plan_dump): [(variant, grid, i[0..19])]"""
    rc, text = emu.plan_dump(desc)
    assert rc == 0, text
    out = []
    for line in text.splitlines():
        m = re.match(r"step \d+ kind=\d+ variant=(-?\d+) grid=(\d+) .* i=([-\d,]+) f=", line)
        if m:
            out.append((int(m.group(1)), int(m.group(2)), [int(v) for v in m.group(3).split(",")]))
    return out


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_the_kernel_lists(monkeypatch, real):
    """MI355_TILE_GROUP_KERNEL_LIST has two entries per data type: id 0 the sum form (Cg > 1), id 1 the depthwise form (Cg = 1), both P = 64; the spectrum launch
    stays on id 0 of the single-channel list.  The grouped step carries Cg | C << 32, K | Kg << 32 and lane_k in slots 8, 7 and 6, and B K per_image work items.
    There is no 128-point grouped instance and no circular one.  (The threads and LDS bytes of every list entry against what the dispatch launches with, and the
    list's length: tests/emu/fftconv_group_asan_main.cpp check_registry, run by test_emu_fftconv_group_asan.py)"""
    monkeypatch.setenv("MI355FFT_GROUP_OLS2D", "64")
    batch, shape, ks = 2, (150, 130), (9, 5)
    per_image = 3 * (2 if real else 3)                                   # L = 56 x 60 on 158 x 134: 3 x 3 tiles, real: 3 x 2 pairs
    for (C, K, G), variant in (((4, 4, 2), 0), ((6, 2, 2), 0), ((3, 3, 3), 1), ((2, 6, 2), 1)):
        steps = _steps(_desc(groups.options(real, shape, ks, batch, C, K, G))[0])
        assert len(steps) == 2, steps
        (sv, _, si), (gv, grid, gi) = steps
        Cg, Kg = C // G, K // G
        assert sv == 0 and si[0] == K * Cg and si[7] == 0 and si[8] == 0, (C, K, G, sv, si)          # the spectrum launch: K Cg single-channel work items
        assert gv == variant, (C, K, G, gv)
        assert gi[8] == Cg | C << 32 and gi[7] == K | Kg << 32 and gi[6] == batch * shape[0] * shape[1], (C, K, G, gi)
        assert gi[0] == batch * K * per_image and 1 <= grid <= gi[0], (C, K, G, gi[0], grid)
    # kernels of 18 .. 33 points would need a 128-point tile: no grouped instance, whatever the switch says; nor a circular one
    for sw in ("64", "128", "1"):
        monkeypatch.setenv("MI355FFT_GROUP_OLS2D", sw)
        route = _plan(real, (300, 200), (33, 17), 2, 4, 4, 2)[0]
        assert ("conv-ols-group[N=64x64,L=32x48" in route) == (sw == "64") and "N=128x128" not in route, (sw, route)
        assert "-group[" not in _plan(real, (300, 200), (9, 9), 2, 4, 4, 4, boundary="circular")[0], sw


def test_kernel_array_length_errors():
    """Plan.exec's kernel argument, host side: the packed array of K Cg kernels or a list of K Cg arrays.  With G > 1 the two length errors name the count as
    kernelCount=K x inputChannels/groups=Cg; with G = 1 the messages are the ones the sum tests pin"""
    import mi355fft

    def plan(opts):
        p = mi355fft.Plan.__new__(mi355fft.Plan)
        p._resolved, p._kernel_upload = resolve_plan_options(opts), None
        return p
    h = np.zeros(2 * 25 * 12, np.float32)
    p = plan(groups.options(False, (64, 48), (5, 5), 2, 4, 6, 2))          # K Cg = 12 kernels of 50 floats
    with pytest.raises(mi355fft.Mi355Error, match=r"kernel array length must equal fftConv.kernelCount=6 x inputChannels/groups=2; got 6"):
        p._kernel_buffer([h[:50]] * 6)
    with pytest.raises(mi355fft.Mi355Error, match=r"kernel Float32Array length must be 600 for kernelCount=6 x inputChannels/groups=2; got 300"):
        p._kernel_buffer(h[:300])
    with pytest.raises(mi355fft.Mi355Error, match=r"kernel\[3\] Float32Array length must be 50; got 49"):
        p._kernel_buffer([h[:50]] * 3 + [h[:49]] + [h[:50]] * 8)
    p = plan(groups.options(True, (64, 48), (5, 5), 2, 3, 3, 3))           # depthwise, real: K Cg = 3 kernels of 25 floats
    with pytest.raises(mi355fft.Mi355Error, match=r"kernel Float32Array length must be 75 for kernelCount=3 x inputChannels/groups=1; got 225"):
        p._kernel_buffer(h[:225])
    p = plan(groups.options(False, (64, 48), (5, 5), 2, 4, 6, 1))          # G = 1: today's messages
    with pytest.raises(mi355fft.Mi355Error, match=r"kernel array length must equal fftConv.kernelCount=6 x inputChannels=4; got 6"):
        p._kernel_buffer([h[:50]] * 6)
    p = plan(groups.options(False, (64, 48), (5, 5), 2, None, 6, None))
    with pytest.raises(mi355fft.Mi355Error, match=r"kernel Float32Array length must be 300 for kernelCount=6; got 600"):
        p._kernel_buffer(h)


# ---- validation --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [0, -1, 1.5, "2", True])
def test_groups_must_be_a_positive_integer(bad):
    with pytest.raises(ValueError, match="fftConv.groups must be a positive integer; got"):
        resolve_plan_options(groups.options(False, (64, 48), (5, 5), 2, 4, 4, bad))


def test_groups_must_divide_both_counts():
    with pytest.raises(ValueError, match=r"fftConv.groups=3 must divide fftConv.inputChannels=4"):
        resolve_plan_options(groups.options(False, (64, 48), (5, 5), 2, 4, 6, 3))
    with pytest.raises(ValueError, match=r"fftConv.groups=2 must divide fftConv.kernelCount=3"):
        resolve_plan_options(groups.options(False, (64, 48), (5, 5), 2, 4, 3, 2))
    with pytest.raises(ValueError, match=r"fftConv.groups=2 must divide fftConv.inputChannels=1"):
        resolve_plan_options(groups.options(False, (64, 48), (5, 5), 2, None, 2, 2))
    # everything inputChannels > 1 rejects stays rejected with its present message
    o = groups.options(False, (64, 48), (5, 5), 2, 2, 2, 2)
    o["fftConv"]["channelPolicy"] = {"input": {"preset": "nchw"}}
    with pytest.raises(ValueError, match="fftConv.inputChannels > 1 cannot be combined with fftConv.channelPolicy.input"):
        resolve_plan_options(o)
    with pytest.raises(ValueError, match="fftconv inPlace=true is not supported"):
        resolve_plan_options(dict(groups.options(False, (64, 48), (5, 5), 2, 2, 2, 2), inPlace=True))
    with pytest.raises(emu.EmuError, match="Unsupported: fftConv.inputChannels > 1 on real circular fftconv with odd shape") as e:
        _plan(True, (63, 48), (5, 5), 2, 2, 2, 2, boundary="circular")
    assert e.value.code == 2


def test_the_descriptor_word():
    """the group count rides mi355fft_zero_range.reserved of zero_read, and the planner rejects it anywhere else"""
    desc, r = _desc(groups.options(False, (64, 48), (5, 5), 2, 4, 6, 2))
    assert desc.zero_read.reserved == 2 and desc.zero_write.reserved == 0 and desc.input.reserved == 4 and r["conv"]["groups"] == 2
    assert _desc(groups.options(False, (64, 48), (5, 5), 2, 4, 6, 1))[0].zero_read.reserved == 0
    import ctypes
    assert ctypes.sizeof(desc) == 912
    desc, r = _desc(groups.options(True, (64, 48), (5, 5), 2, 4, 6, 2))
    assert (r["inputBytes"], r["kernelBytes"], r["outputBytes"]) == (4 * 2 * 4 * 64 * 48, 4 * 6 * 2 * 25, 4 * 2 * 6 * 64 * 48)
    desc.zero_write.reserved = 2
    with pytest.raises(emu.EmuError, match="mi355fft_zero_range.reserved must be 0") as e:
        emu.plan_only(desc)
    assert e.value.code == 1
    from exec_contract_cases import desc_of
    c2c = desc_of({"type": "c2c", "shape": [64], "batch": 2, "direction": "forward", "normalize": "none"})[0]
    c2c.zero_read.reserved = 2
    with pytest.raises(emu.EmuError, match="mi355fft_zero_range.reserved must be 0") as e:
        emu.plan_only(c2c)
    assert e.value.code == 1
    for word, text in ((-1, "fftConv.groups must be a positive integer"), (3, "fftConv.groups=3 must divide fftConv.inputChannels=4")):
        bad = _desc(groups.options(False, (64, 48), (5, 5), 2, 4, 6, 1))[0]
        bad.zero_read.reserved = word
        with pytest.raises(emu.EmuError, match=text) as e:
            emu.plan_only(bad)
        assert e.value.code == 1
    bad = _desc(groups.options(False, (64, 48), (5, 5), 2, 4, 6, 1))[0]
    bad.zero_read.reserved = 4
    with pytest.raises(emu.EmuError, match="fftConv.groups=4 must divide fftConv.kernelCount=6"):
        emu.plan_only(bad)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", groups.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans every case"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
