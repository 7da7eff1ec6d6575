"""CPU tier: the overlap-save brick route of rank-3 real fftconv (bricks-rconv-ols[N=16x16x16,L=L0xL1xL2]) under host emulation.

The case table and its bars are fftconv_rbricks_cases.py's, shared with the GPU tier: float64 references, the same request with the switch at 0,
the complex plan on the widened data, the exact route tag and 1 + K launches.  Then the strided request (no plan at all with the switch at 0:
the capability the route adds), the planner alone on the rule, the switch and the neighbours whose routes must not move, the accuracy ladder,
and the exec contract (exec_contract_cases.py's harness: guard bands catch a load or store outside a brick's predicates) on a dense and a
strided request."""
import pytest

import emu_harness as emu
import fftconv_bricks_cases as bricks
import fftconv_ols_scaffold as scaffold
import fftconv_rbricks_cases as rbricks
import test_emu_accuracy as accuracy
import test_emu_exec_contract as contract
from mi355fft import _abi
from test_emu_fftconv_real import _desc, _opts


@pytest.mark.parametrize("case", rbricks.CASES, ids=repr)
def test_overlap_save_real_bricks(oracle, monkeypatch, case):
    rbricks.ROUTE.check_case(*scaffold.emu_runner(monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(oracle, monkeypatch):
    def unsupported(opts):
        with pytest.raises(emu.EmuError) as e:
            emu.plan_only(_desc(opts)[0])
        assert rbricks.UNSUPPORTED in str(e.value) and e.value.code == _abi.ERR_UNSUPPORTED
    rbricks.ROUTE.check_strided(*scaffold.emu_runner(monkeypatch), oracle, unsupported)


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(shape, ks, batch, K=1, boundary="linear-same", mode="convolution", layout=None, **fc):
    return emu.plan_only(_desc(_opts(list(shape), list(ks), batch, K=K, mode=mode, boundary=boundary, layout=layout, **fc))[0])


_tag = rbricks.ROUTE.tag_of
SWITCH = "MI355FFT_RCONV_OLS3D"


@pytest.mark.parametrize("shape,ks,K,before", [((256, 256, 256), (3, 3, 3), 1, 57), ((256, 256, 256), (3, 3, 3), 4, None), ((512, 512, 512), (5, 5, 5), 1, 57)])
def test_capability_volumes_plan_to_the_route(monkeypatch, shape, ks, K, before):
    """1 + K launches and the K kernel spectra alone as workspace for any volume; with the switch at 0 rconv[K] on the exact-length domain: 57 launches
    and a workspace of several whole-volume spectra (0.90 GB at 256^3, 7.14 GB at 512^3)"""
    route, launches, work = _plan(shape, ks, 1, K)
    assert route.startswith("bricks-rspectrum[N=16x16x16] ") and _tag(16, ks) in route, route
    assert not any(f in route for f in rbricks.ROUTE.forbidden), route
    assert "tiles-rconv-ols[" not in route
    assert launches == 1 + K, (route, launches)
    assert work < 1 << 20 and work >= K * 32768, (route, work)
    monkeypatch.setenv(SWITCH, "0")
    route0, launches0, work0 = _plan(shape, ks, 1, K)
    assert rbricks.ROUTE.tag not in route0 and f"rconv[K={K}]" in route0, route0
    assert before is None or launches0 == before, (route0, launches0)
    assert work0 > 256 << 20, (route0, launches0, work0)


def test_the_default_rule(monkeypatch):
    """as measured (plan.cpp rconv_bricks_block): kernels up to RULE_MAX_KERNEL points on their longest axis, on domains above 32768 points with
    every axis of at least 32; beyond that the switch alone"""
    for ks in ((1, 1, 1), (3, 3, 3), (2, 3, 1)) + tuple(k for k in ((5, 5, 5), (5, 5, 3), (7, 7, 7), (9, 9, 9)) if max(k) <= bricks.RULE_MAX_KERNEL):
        assert _tag(16, ks) in _plan((100, 80, 70), ks, 2)[0], ks
    m = bricks.RULE_MAX_KERNEL + 1
    for ks in ((m, 3, 3), (3, m, 3), (3, 3, m), (15, 15, 15)):
        default = _plan((100, 80, 70), ks, 2)
        assert rbricks.ROUTE.tag not in default[0] and "rconv[K=1]" in default[0], ks
        monkeypatch.setenv(SWITCH, "0")
        assert _plan((100, 80, 70), ks, 2) == default, ks
        monkeypatch.delenv(SWITCH)


def test_the_switch_and_the_neighbours(monkeypatch):
    tag = rbricks.ROUTE.tag
    # the switch: 0 gives what the planner gave before the route, 16 forces the brick where the default rule does not go
    assert tag in _plan((100, 80, 70), (3, 3, 3), 1)[0]
    monkeypatch.setenv(SWITCH, "0")
    route = _plan((100, 80, 70), (3, 3, 3), 1)[0]
    assert "rconv[K=1]" in route and tag not in route, route
    monkeypatch.setenv(SWITCH, "16")
    assert _tag(16, (9, 9, 9)) in _plan((20, 12, 10), (9, 9, 9), 2, boundary="linear-full")[0]
    for ks in ((15, 3, 3), (3, 15, 3), (3, 3, 15)):                       # the longest kernel a brick takes on an axis: L >= 2
        assert _tag(16, ks) in _plan((40, 40, 40), ks, 1)[0], ks
    for ks in ((16, 3, 3), (3, 16, 3), (3, 3, 16)):                       # L = 1 on one axis: the routes below
        assert tag not in _plan((40, 40, 40), ks, 1)[0], ks
    assert tag not in _plan((32, 32, 32), (3, 3, 3), 2, boundary="circular")[0]     # a forced brick leaves circular requests alone
    for bad in ("8", "32", "64"):                                         # not a brick edge of the route: the other routes
        monkeypatch.setenv(SWITCH, bad)
        assert tag not in _plan((100, 80, 70), (3, 3, 3), 1)[0], bad
    monkeypatch.delenv(SWITCH)
    # RCONV_FUSED = 0 and FORCE_GENERIC = 1 come first, also in front of a forced brick
    for name, value in (("MI355FFT_RCONV_FUSED", "0"), ("MI355FFT_FORCE_GENERIC", "1")):
        for forced in (None, "16"):
            if forced:
                monkeypatch.setenv(SWITCH, forced)
            monkeypatch.setenv(name, value)
            route = _plan((100, 80, 70), (3, 3, 3), 1)[0]
            assert tag not in route and "rconv[K=1]" in route, (name, route)
            monkeypatch.delenv(name)
        monkeypatch.delenv(SWITCH)
    # the complex route's switch does not reach real data
    monkeypatch.setenv("MI355FFT_CONV_OLS3D", "0")
    assert tag in _plan((100, 80, 70), (3, 3, 3), 1)[0]
    monkeypatch.delenv("MI355FFT_CONV_OLS3D")
    # neighbours that must not move: circular rank 3, ranks 1, 2 and 4, 32 x 16 x 8 (*) 3 x 2 x 2 (pinned to rconv[K=1] by the GPU tier), domains of at most
    # 32768 points (30^3 (*) 3^3: 32^3), an axis of 31 points
    for shape, ks, boundary in (((64, 64, 64), (3, 3, 3), "circular"), ((100000,), (9,), "linear-same"), ((300, 200), (9, 9), "linear-same"),
                                ((20, 18, 16, 12), (3, 3, 3, 3), "linear-same"), ((32, 16, 8), (3, 2, 2), "linear-same"), ((16, 6, 5), (3, 2, 2), "linear-same"),
                                ((30, 30, 30), (3, 3, 3), "linear-same"), ((100, 80, 29), (3, 3, 3), "linear-same"), ((29, 80, 100), (3, 3, 3), "linear-same")):
        default = _plan(shape, ks, 2, boundary=boundary)
        assert tag not in default[0], (shape, ks, default[0])
        monkeypatch.setenv(SWITCH, "0")
        assert _plan(shape, ks, 2, boundary=boundary) == default, (shape, ks)
        monkeypatch.delenv(SWITCH)
    assert "rconv[K=1]" in _plan((32, 16, 8), (3, 2, 2), 2)[0]
    assert tag in _plan((31, 30, 30), (3, 3, 3), 2)[0]           # the bound is on the domain: 33 x 32 x 32 > 32768 >= 32^3 (30^3 above)


def test_real_strided_rank3_has_a_plan_with_the_route_alone(monkeypatch):
    """strided lanes ride the route's address maps; with the switch at 0 such a request has no plan"""
    lay = {"inputStrides": [3, 301, 24101], "outputStrides": [1, 101, 8101]}
    route, launches, _ = _plan((100, 80, 70), (3, 3, 3), 2, K=2, layout=lay, outputKernelStrideElements=2000001)
    assert rbricks.ROUTE.tag in route and launches == 3, route
    monkeypatch.setenv(SWITCH, "0")
    with pytest.raises(emu.EmuError) as e:
        _plan((100, 80, 70), (3, 3, 3), 2, K=2, layout=lay, outputKernelStrideElements=2000001)
    assert rbricks.UNSUPPORTED in str(e.value) and e.value.code == _abi.ERR_UNSUPPORTED


# ---- accuracy ladder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", rbricks.ACCURACY_CASES, ids=repr)
def test_accuracy(oracle, monkeypatch, case):
    scaffold.emu_planned(monkeypatch, case)
    accuracy.test_accuracy(oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", rbricks.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans both"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
