"""CPU tier: the overlap-save tile route of rank-2 real fftconv (tiles-rconv-ols[N=PxP,L=L0xL1]) under host emulation.

The case table and its bars are fftconv_rtiles_cases.py's, shared with the GPU tier: float64 references, the same request with the switch at 0,
the complex plan on the widened data, the exact route tag and 1 + K launches.  Then the strided request (no plan at all with the switch at 0:
the capability the route adds), the planner alone on the rule, the switch and the neighbours whose routes must not move, the accuracy ladder,
and the exec contract (exec_contract_cases.py's harness: guard bands catch a load or store outside a tile's predicates) on a dense and a
strided request."""
import pytest

import emu_harness as emu
import fftconv_ols_scaffold as scaffold
import fftconv_rtiles_cases as rtiles
import test_emu_accuracy as accuracy
import test_emu_exec_contract as contract
from mi355fft import _abi
from test_emu_fftconv_real import _desc, _opts


@pytest.mark.parametrize("case", rtiles.CASES, ids=repr)
def test_overlap_save_real_tiles(oracle, monkeypatch, case):
    rtiles.ROUTE.check_case(*scaffold.emu_runner(monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(oracle, monkeypatch):
    def unsupported(opts):
        with pytest.raises(emu.EmuError) as e:
            emu.plan_only(_desc(opts)[0])
        assert rtiles.UNSUPPORTED in str(e.value) and e.value.code == _abi.ERR_UNSUPPORTED
    rtiles.ROUTE.check_strided(*scaffold.emu_runner(monkeypatch), oracle, unsupported)


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(shape, ks, batch, K=1, boundary="linear-same", mode="convolution", layout=None, **fc):
    return emu.plan_only(_desc(_opts(list(shape), list(ks), batch, K=K, mode=mode, boundary=boundary, layout=layout, **fc))[0])


@pytest.mark.parametrize("shape,ks,batch,K,boundary,P", [
    ((1024, 1024), (9, 9), 8, 1, "linear-same", 64),
    ((1024, 1024), (9, 9), 8, 4, "linear-same", 64),
    ((4096, 4096), (33, 33), 1, 1, "linear-valid", 128),
])
def test_capability_images_plan_to_the_route(monkeypatch, shape, ks, batch, K, boundary, P):
    """1 + K launches and the K kernel spectra alone as workspace for any image; with the switch at 0 rconv[K] on the exact-length domain with a
    workspace of several whole-image spectra"""
    route, launches, work = _plan(shape, ks, batch, K, boundary)
    assert route.startswith(f"tiles-rspectrum[N={P}x{P}] ") and rtiles.ROUTE.tag_of(P, ks) in route, route
    assert not any(f in route for f in rtiles.ROUTE.forbidden), route
    assert launches == 1 + K, (route, launches)
    assert work < 1 << 20 and work >= K * P * P * 8, (route, work)
    monkeypatch.setenv("MI355FFT_RCONV_OLS2D", "0")
    route0, launches0, work0 = _plan(shape, ks, batch, K, boundary)
    assert rtiles.ROUTE.tag not in route0 and f"rconv[K={K}]" in route0, route0
    assert launches0 > 1 + K and work0 > 64 << 20, (route0, launches0, work0)


def test_the_default_rule():
    """the tile edge: 64 up to kernels of 17 points on their longer axis, 128 up to 33"""
    for ks, P in (((1, 1), 64), ((9, 9), 64), ((17, 3), 64), ((3, 17), 64), ((18, 3), 128), ((3, 18), 128), ((33, 33), 128)):
        assert rtiles.ROUTE.tag_of(P, ks) in _plan((300, 200), ks, 2)[0], (ks, P)


def test_the_switch_and_the_neighbours(monkeypatch):
    tag = rtiles.ROUTE.tag
    # the switch: 0 gives what the planner gave before the route, a tile edge forces it where the default rule does not go
    assert tag in _plan((300, 200), (9, 9), 2)[0]
    monkeypatch.setenv("MI355FFT_RCONV_OLS2D", "0")
    route = _plan((300, 200), (9, 9), 2)[0]
    assert "rconv[K=1]" in route and tag not in route, route
    monkeypatch.setenv("MI355FFT_RCONV_OLS2D", "64")
    assert rtiles.ROUTE.tag_of(64, (9, 9)) in _plan((20, 30), (9, 9), 3, boundary="linear-full")[0]
    assert rtiles.ROUTE.tag_of(64, (63, 3)) in _plan((70, 200), (63, 3), 1)[0]         # the longest kernel a tile takes on an axis: L >= 2
    assert tag not in _plan((70, 200), (64, 3), 1)[0]                           # L0 = 1: the routes below
    assert tag not in _plan((200, 70), (3, 64), 1)[0]
    assert tag not in _plan((64, 64), (9, 9), 2, boundary="circular")[0]        # a forced tile leaves circular requests alone
    monkeypatch.setenv("MI355FFT_RCONV_OLS2D", "128")
    assert rtiles.ROUTE.tag_of(128, (9, 9)) in _plan((300, 200), (9, 9), 2)[0]
    for bad in ("32", "100", "256"):                                            # not a tile edge of the route: the other routes
        monkeypatch.setenv("MI355FFT_RCONV_OLS2D", bad)
        assert tag not in _plan((300, 200), (9, 9), 2)[0], bad
    monkeypatch.delenv("MI355FFT_RCONV_OLS2D")
    # RCONV_FUSED = 0 and FORCE_GENERIC = 1 come first, also in front of a forced tile
    for name, value in (("MI355FFT_RCONV_FUSED", "0"), ("MI355FFT_FORCE_GENERIC", "1")):
        for forced in (None, "64"):
            if forced:
                monkeypatch.setenv("MI355FFT_RCONV_OLS2D", forced)
            monkeypatch.setenv(name, value)
            route = _plan((300, 200), (9, 9), 2)[0]
            assert tag not in route and "rconv[K=1]" in route, (name, route)
            monkeypatch.delenv(name)
        monkeypatch.delenv("MI355FFT_RCONV_OLS2D")
    # the complex route's switch does not reach real data, nor this one complex data
    monkeypatch.setenv("MI355FFT_CONV_OLS2D", "0")
    assert tag in _plan((300, 200), (9, 9), 2)[0]
    monkeypatch.delenv("MI355FFT_CONV_OLS2D")
    # neighbours that must not move: the small rank-2 requests (64 x 48 (*) 5 x 3 among them), circular rank 2, rank 1, rank 3, axes below 64 points,
    # kernels beyond 33 points
    for shape, ks, boundary in (((64, 48), (5, 3), "linear-same"), ((64, 64), (9, 9), "circular"), ((256, 256), (9, 9), "circular"), ((32, 12), (5, 3), "linear-same"),
                                ((29, 8), (5, 3), "linear-full"), ((300, 200), (34, 3), "linear-same"), ((300, 200), (3, 34), "linear-same"),
                                ((120, 120), (9, 9), "linear-same"), ((2000, 60), (3, 3), "linear-same")):
        default = _plan(shape, ks, 2, boundary=boundary)
        assert tag not in default[0] and "rconv[K=1]" in default[0], (shape, ks, default[0])
        monkeypatch.setenv("MI355FFT_RCONV_OLS2D", "0")
        assert _plan(shape, ks, 2, boundary=boundary) == default, (shape, ks)
        monkeypatch.delenv("MI355FFT_RCONV_OLS2D")
    assert tag in _plan((121, 120), (9, 9), 2)[0]           # the bound is on the domain: 129 x 128 > 16384 >= 128 x 128 (120 x 120 above)
    route = emu.plan_only(_desc(_opts([100000], [9], 4, boundary="linear-same"))[0])[0]
    assert tag not in route and "lines-rconv-ols[" in route, route
    assert tag not in emu.plan_only(_desc(_opts([100, 80, 70], [5, 5, 5], 1, boundary="linear-same"))[0])[0]
    # strided lanes ride the route's address maps; with the switch at 0 such a request has no plan
    lay = {"inputStrides": [3, 1001], "outputStrides": [1, 301]}
    route, launches, _ = _plan((300, 200), (9, 9), 2, K=2, layout=lay, outputKernelStrideElements=1000001)
    assert tag in route and launches == 3, route
    monkeypatch.setenv("MI355FFT_RCONV_OLS2D", "0")
    with pytest.raises(emu.EmuError) as e:
        _plan((300, 200), (9, 9), 2, K=2, layout=lay, outputKernelStrideElements=1000001)
    assert rtiles.UNSUPPORTED in str(e.value) and e.value.code == _abi.ERR_UNSUPPORTED


# ---- accuracy ladder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", rtiles.ACCURACY_CASES, ids=repr)
def test_accuracy(oracle, monkeypatch, case):
    scaffold.emu_planned(monkeypatch, case)
    accuracy.test_accuracy(oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", rtiles.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans both"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
