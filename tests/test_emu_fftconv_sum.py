"""CPU tier: fftConv.inputChannels, the sum over input channels, under host emulation.

The tables and their bars are fftconv_sum_cases.py's, shared with the GPU tier: the sum form of the rank-2 tile kernel (complex and real) and the
composed routes fftconv-sum / rconv-sum against float64 references summed over the channels and against the float32 sum of the C single-channel
plans a caller had to run before; strided lanes on both sides; C = 1 as the request without the option (same route, same launches, the same bits);
the planner alone on the switch and its neighbours; validation; and the exec contract (test_emu_exec_contract.py's harness)."""
import re

import numpy as np
import pytest

import emu_harness as emu
import fftconv_ols_scaffold as scaffold
import fftconv_sum_cases as sums
import test_emu_exec_contract as contract
from mi355fft.layout import resolve_plan_options
from test_emu_fftconv_real import _desc, _rel


@pytest.mark.parametrize("case", sums.TILE_CASES + sums.COMPOSED_CASES, ids=repr)
def test_sum_over_input_channels(oracle, monkeypatch, case):
    sums.check_case(*scaffold.emu_runner(monkeypatch), oracle, case)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_strided_lanes_on_both_sides(oracle, monkeypatch, real):
    sums.check_strided(*scaffold.emu_runner(monkeypatch), oracle, real)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_the_composed_route_agrees_with_the_tile_route(monkeypatch, real):
    """SUM_OLS2D = 0 on the first request of the table against the tile route, rel_l2 <= 1e-5"""
    run, setenv = scaffold.emu_runner(monkeypatch)
    case = next(c for c in sums.TILE_CASES if c.real == real)
    x, h, want = sums.data(case)
    setenv(sums.SWITCH, "64")
    tile, route, _ = run(case.opts, x, want.size, h)
    setenv(sums.SWITCH, "0")
    composed, route0, _ = run(case.opts, x, want.size, h)
    assert case.tag in route and sums.composed_tag(real, case.K, case.C) in route0 and "ols-sum" not in route0, (route, route0)
    rel = _rel(tile, composed)
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={rel:.3e}")
    assert rel <= sums.PARITY_BAR


@pytest.mark.parametrize("real,shape,ks,batch,K,boundary,env", sums.C1_CASES, ids=lambda v: None)
def test_one_channel_is_the_request_without_the_option(monkeypatch, real, shape, ks, batch, K, boundary, env):
    run, setenv = scaffold.emu_runner(monkeypatch)
    for name, value in env.items():
        setenv(name, value)
    rand = sums._route(real).rand
    x, h = rand(int(np.prod(shape)) * batch, 0x5C11), rand(int(np.prod(ks)) * K, 0x5C12)
    out_floats = int(np.prod(resolve_plan_options(sums.options(real, shape, ks, batch, None, K, boundary=boundary))["outputShape"])) * batch * K * (1 if real else 2)
    plain = run(sums.options(real, shape, ks, batch, None, K, boundary=boundary), x, out_floats, h)
    one = run(sums.options(real, shape, ks, batch, 1, K, boundary=boundary), x, out_floats, h)
    assert plain[1:] == one[1:], (plain[1:], one[1:])
    assert "-sum" not in one[1], one[1]
    assert np.array_equal(np.asarray(plain[0]).view(np.uint32), np.asarray(one[0]).view(np.uint32))


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(real, shape, ks, batch, C, K=1, boundary="linear-same", **kw):
    return emu.plan_only(_desc(sums.options(real, shape, ks, batch, C, K, boundary=boundary, **kw))[0])


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
def test_the_switch_and_the_neighbours(monkeypatch, real):
    tag = "conv-ols-sum["
    route, launches, work = _plan(real, (300, 200), (9, 9), 2, 4, K=2)
    assert sums.tile_tag(real, 64, (9, 9), 4) in route and launches == 3, (route, launches)
    assert 2 * 4 * 64 * 64 * 8 <= work < 1 << 20, work                  # the K C kernel spectra alone
    for ks in ((1, 1), (17, 3), (3, 17)):                                # the rule: the 64-point tile up to 17 points an axis
        assert sums.tile_tag(real, 64, ks, 3) in _plan(real, (300, 200), ks, 2, 3)[0], ks
    for ks in ((18, 3), (3, 33)):                                        # beyond: no sum instance, the composed route, whatever the switch says
        for sw in (None, "128", "64"):
            if sw:
                monkeypatch.setenv("MI355FFT_SUM_OLS2D", sw)
            route = _plan(real, (300, 200), ks, 2, 3)[0]
            assert (tag in route) == (sw == "64") and (sums.composed_tag(real, 1, 3) in route) == (sw != "64"), (ks, sw, route)
        monkeypatch.delenv("MI355FFT_SUM_OLS2D")
    # 0: composed; 64: every linear rank-2 request the tile fits, L >= 2; not a tile edge: composed
    monkeypatch.setenv("MI355FFT_SUM_OLS2D", "0")
    assert sums.composed_tag(real, 1, 4) in _plan(real, (300, 200), (9, 9), 2, 4)[0]
    monkeypatch.setenv("MI355FFT_SUM_OLS2D", "64")
    assert sums.tile_tag(real, 64, (9, 9), 17) in _plan(real, (20, 30), (9, 9), 3, 17, boundary="linear-full")[0]
    assert sums.tile_tag(real, 64, (63, 3), 2) in _plan(real, (70, 200), (63, 3), 1, 2)[0]
    assert tag not in _plan(real, (70, 200), (64, 3), 1, 2)[0]
    assert tag not in _plan(real, (256, 256), (9, 9), 2, 2, boundary="circular")[0]      # circular sum instances do not exist
    for bad in ("32", "100", "256"):
        monkeypatch.setenv("MI355FFT_SUM_OLS2D", bad)
        assert tag not in _plan(real, (300, 200), (9, 9), 2, 4)[0], bad
    monkeypatch.delenv("MI355FFT_SUM_OLS2D")
    # the switches in front of the single-channel tile route come first
    for name, value in ((("MI355FFT_RCONV_OLS2D", "0"), ("MI355FFT_RCONV_FUSED", "0")) if real else (("MI355FFT_CONV_OLS2D", "0"), ("MI355FFT_CONV_LINES", "0"))) + \
            (("MI355FFT_FORCE_GENERIC", "1"),):
        monkeypatch.setenv(name, value)
        route = _plan(real, (300, 200), (9, 9), 2, 4)[0]
        assert tag not in route and sums.composed_tag(real, 1, 4) in route, (name, route)
        monkeypatch.delenv(name)
    # the single-channel routes are not considered with C > 1: rank 1 and rank 3 requests that take overlap-save, lines-mul, lines-rconv without the option
    for shape, ks in (((100000,), (9,)), ((1000,), (31,)), ((100, 80, 70), (5, 5, 5))):
        route = _plan(real, shape, ks, 2, 3)[0]
        assert sums.composed_tag(real, 1, 3) in route and not any(f in route for f in ("-ols[", "lines-mul", "lines-rconv[", "fftconv-fused", "pipeline")), route
    # and C = 1 plans what the request without the option plans
    for shape, ks in (((300, 200), (9, 9)), ((100000,), (9,)), ((1000,), (31,)), ((100, 80, 70), (5, 5, 5))):
        assert _plan(real, shape, ks, 2, 1) == _plan(real, shape, ks, 2, None), (shape, ks)


# ---- validation --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [0, -1, 1.5, "2", True])
def test_input_channels_must_be_a_positive_integer(bad):
    with pytest.raises(ValueError, match="fftConv.inputChannels must be a positive integer"):
        resolve_plan_options(sums.options(False, (64, 48), (5, 5), 2, bad))


def test_rejected_combinations():
    policy = {"input": {"preset": "nchw"}, "output": {"preset": "nchw"}}
    o = sums.options(False, (64, 48), (5, 5), 2, 2)
    o["fftConv"]["channelPolicy"] = {"input": policy["input"]}
    with pytest.raises(ValueError, match="fftConv.inputChannels > 1 cannot be combined with fftConv.channelPolicy.input"):
        resolve_plan_options(o)
    o = sums.options(False, (64, 48), (5, 5), 2, 2)
    o["layout"] = {"interleavedComplex": True, "whdcn": {"input": {"channels": 2, "channel": 0}}}
    with pytest.raises(ValueError, match="fftConv.inputChannels > 1 cannot be combined with layout.whdcn"):
        resolve_plan_options(o)
    # inPlace and f16-storage keep their messages
    with pytest.raises(ValueError, match="fftconv inPlace=true is not supported"):
        resolve_plan_options(dict(sums.options(False, (64, 48), (5, 5), 2, 2), inPlace=True))
    with pytest.raises(ValueError, match='fftconv supports precision:"f32" only'):
        resolve_plan_options(dict(sums.options(False, (64, 48), (5, 5), 2, 2), precision="f16-storage"))
    with pytest.raises(ValueError, match="ioView is not an fftconv option"):
        resolve_plan_options(dict(sums.options(False, (64, 48), (5, 5), 2, 2), ioView={"input": {"shape": [8, 8], "offset": [0, 0]}}))


def test_the_descriptor_word():
    """the channel count rides mi355fft_side_layout.reserved of the input side, and the planner rejects it anywhere else"""
    desc, r = _desc(sums.options(False, (64, 48), (5, 5), 2, 3, K=2))
    assert desc.input.reserved == 3 and desc.output.reserved == 0 and r["conv"]["inputChannels"] == 3
    assert _desc(sums.options(False, (64, 48), (5, 5), 2, 1))[0].input.reserved == 0
    desc, r = _desc(sums.options(True, (64, 48), (5, 5), 2, 3, K=2))
    assert (r["inputBytes"], r["kernelBytes"], r["outputBytes"]) == (4 * 2 * 3 * 64 * 48, 4 * 2 * 3 * 25, 4 * 2 * 2 * 64 * 48)
    desc.output.reserved = 3
    with pytest.raises(emu.EmuError, match="reserved must be 0") as e:
        emu.plan_only(desc)
    assert e.value.code == 1
    from exec_contract_cases import desc_of
    c2c = desc_of({"type": "c2c", "shape": [64], "batch": 2, "direction": "forward", "normalize": "none"})[0]
    c2c.input.reserved = 2
    with pytest.raises(emu.EmuError, match="reserved must be 0") as e:
        emu.plan_only(c2c)
    assert e.value.code == 1
    neg = _desc(sums.options(False, (64, 48), (5, 5), 2, 1))[0]
    neg.input.reserved = -1
    with pytest.raises(emu.EmuError, match="fftConv.inputChannels must be a positive integer"):
        emu.plan_only(neg)


def test_odd_circular_real_lines_have_no_sum_plan():
    """real circular with odd shape[0] (rconv-widened without the option): Unsupported with C > 1; with C = 1 it plans as before"""
    with pytest.raises(emu.EmuError, match=re.escape(sums.UNSUPPORTED_ODD)) as e:
        _plan(True, (63, 48), (5, 5), 2, 2, boundary="circular")
    assert e.value.code == 2
    assert "rconv-widened" in _plan(True, (63, 48), (5, 5), 2, 1, boundary="circular")[0]
    assert sums.composed_tag(False, 1, 2) in _plan(False, (63, 48), (5, 5), 2, 2, boundary="circular")[0]     # complex data: a plan
    with pytest.raises(emu.EmuError, match="Unsupported: strided layouts on real fftconv"):                  # strided real sides outside the tile route: as before
        emu.plan_only(_desc(dict(sums.options(True, (1000,), (31,), 2, 2), layout={"interleavedComplex": False, "inputStrides": [2]}))[0])


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sums.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans every case"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
