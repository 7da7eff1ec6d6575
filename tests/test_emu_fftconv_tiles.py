"""CPU tier: the overlap-save tile route of rank-2 complex fftconv (tiles-conv-ols[N=PxP,L=L0xL1]) under host emulation.

The case table and its bars are fftconv_tiles_cases.py's, shared with the GPU tier: float64 references, the same request with the switch at 0,
the exact route tag and 1 + K launches.  Then the planner alone on image sizes whose earlier plans took 33 launches and hundreds of MiB of
workspace (route, launches, workspace: the capability the route adds) and on the neighbours whose routes the switch must not move, the
accuracy ladder, and the exec contract (exec_contract_cases.py's harness: guard bands catch a load or store outside a tile's predicates) on a
dense and a strided request."""
import pytest

import emu_harness as emu
import fftconv_ols_scaffold as scaffold
import fftconv_tiles_cases as tiles
import test_emu_accuracy as accuracy
import test_emu_exec_contract as contract
from test_emu_fftconv import _desc


@pytest.mark.parametrize("case", tiles.CASES, ids=repr)
def test_overlap_save_tiles(oracle, monkeypatch, case):
    tiles.ROUTE.check_case(*scaffold.emu_runner(monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(oracle, monkeypatch):
    tiles.ROUTE.check_strided(*scaffold.emu_runner(monkeypatch), oracle)


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(shape, ks, batch, K=1, boundary="linear-same", mode="convolution", layout=None, **fc):
    opts = scaffold.options(shape, ks, batch, K, mode, boundary)
    opts["fftConv"].update(fc)
    if layout:
        opts["layout"] = layout
    return emu.plan_only(_desc(opts)[0])


_tag = tiles.ROUTE.tag_of


@pytest.mark.parametrize("shape,ks,batch,K,boundary,P,before", [
    ((1024, 1024), (9, 9), 8, 1, "linear-same", 64, ("bluestein-lines[N=1032,M=4096]", 33)),
    ((1024, 1024), (9, 9), 8, 4, "linear-same", 64, ("bluestein-lines[N=1032,M=4096]", None)),
    ((4096, 4096), (33, 33), 1, 1, "linear-valid", 128, ("bluestein-lines[N=4128,M=16384]", 33)),
])
def test_capability_images_plan_to_the_route(monkeypatch, shape, ks, batch, K, boundary, P, before):
    """8 x 1024 x 1024 (*) 9 x 9 (33 launches and 461 MiB of workspace before the route) and 4096 x 4096 (*) 33 x 33 (33 launches, 1036 MiB):
    1 + K launches and the K kernel spectra alone as workspace; with the switch at 0 the planner's earlier route and launch count"""
    route, launches, work = _plan(shape, ks, batch, K, boundary)
    assert route.startswith(f"tiles-spectrum[N={P}x{P}] ") and _tag(P, ks) in route, route
    assert not any(f in route for f in tiles.ROUTE.forbidden), route
    assert launches == 1 + K, (route, launches)
    assert work < 1 << 20 and work >= K * P * P * 8, (route, work)
    monkeypatch.setenv("MI355FFT_CONV_OLS2D", "0")
    route0, launches0, work0 = _plan(shape, ks, batch, K, boundary)
    assert tiles.ROUTE.tag not in route0 and before[0] in route0 and f"fftconv[K={K}]" in route0, route0
    assert before[1] is None or launches0 == before[1], (route0, launches0)
    assert work0 > 256 << 20, (route0, work0)


def test_the_default_rule():
    """the tile edge: 64 up to kernels of 17 points on their longer axis, 128 up to 33"""
    for ks, P in (((1, 1), 64), ((9, 9), 64), ((17, 3), 64), ((3, 17), 64), ((18, 3), 128), ((3, 18), 128), ((33, 33), 128)):
        assert _tag(P, ks) in _plan((300, 200), ks, 2)[0], (ks, P)


def test_the_switch_and_the_neighbours(monkeypatch):
    tag = tiles.ROUTE.tag
    # the switch: 0 gives what the planner gave before the route, a tile edge forces it where the default rule does not go
    assert tag in _plan((300, 200), (9, 9), 2)[0]
    monkeypatch.setenv("MI355FFT_CONV_OLS2D", "0")
    route = _plan((300, 200), (9, 9), 2)[0]
    assert "fftconv[K=1]" in route and tag not in route, route
    monkeypatch.setenv("MI355FFT_CONV_OLS2D", "64")
    assert _tag(64, (9, 9)) in _plan((20, 30), (9, 9), 3, boundary="linear-full")[0]
    assert _tag(64, (63, 3)) in _plan((70, 200), (63, 3), 1)[0]          # the longest kernel a tile takes on an axis: L >= 2
    assert tag not in _plan((70, 200), (64, 3), 1)[0]                   # L0 = 1: the routes below
    assert tag not in _plan((200, 70), (3, 64), 1)[0]
    assert _tag(64, (9, 5)) in _plan((150, 100), (9, 5), 3, boundary="linear-full", mode="correlation")[0]
    monkeypatch.setenv("MI355FFT_CONV_OLS2D", "128")
    assert _tag(128, (9, 9)) in _plan((300, 200), (9, 9), 2)[0]
    for bad in ("32", "100", "256"):                                    # not a tile edge of the route: the other routes
        monkeypatch.setenv("MI355FFT_CONV_OLS2D", bad)
        assert tag not in _plan((300, 200), (9, 9), 2)[0], bad
    monkeypatch.delenv("MI355FFT_CONV_OLS2D")
    # CONV_LINES = 0 and FORCE_GENERIC = 1 switch the route off, as they do for the line routes
    for name in ("MI355FFT_CONV_LINES", "MI355FFT_FORCE_GENERIC"):
        monkeypatch.setenv(name, "0" if name.endswith("LINES") else "1")
        assert tag not in _plan((300, 200), (9, 9), 2)[0], name
        monkeypatch.delenv(name)
    # neighbours that must not move: circular rank 2, rank 1, rank 3, domains of at most 16384 points, axes below 64 points, kernels beyond 33 points
    assert tag not in _plan((256, 256), (9, 9), 2, boundary="circular")[0]
    opts = {"type": "fftconv", "shape": [100000], "batch": 4, "fftConv": {"boundary": "linear-same", "kernelCount": 1, "kernelShape": [9]}}
    route = emu.plan_only(_desc(opts)[0])[0]
    assert tag not in route and "lines-conv-ols[" in route, route
    opts = {"type": "fftconv", "shape": [100, 80, 70], "batch": 1, "fftConv": {"boundary": "linear-same", "kernelCount": 1, "kernelShape": [5, 5, 5]}}
    assert tag not in emu.plan_only(_desc(opts)[0])[0]
    for shape, ks in (((12, 5), (3, 2)), ((30, 6), (3, 3)), ((32768, 4), (65, 3)), ((300, 200), (34, 3)), ((300, 200), (3, 34)), ((120, 120), (9, 9)), ((2000, 60), (3, 3))):
        for env in (None, "0"):
            if env is not None:
                monkeypatch.setenv("MI355FFT_CONV_OLS2D", env)
            got = _plan(shape, ks, 2)
            assert tag not in got[0], (shape, ks)
            if env is None:
                default = got
        assert got == default, (shape, ks)
        monkeypatch.delenv("MI355FFT_CONV_OLS2D")
    assert tag in _plan((121, 120), (9, 9), 2)[0]           # the bound is on the domain: 129 x 128 > 16384 >= 128 x 128 (120 x 120 above)
    # strided lanes ride the route's address maps
    route, launches, _ = _plan((300, 200), (9, 9), 2, K=2, layout={"interleavedComplex": True, "inputStrides": [2, 700], "outputStrides": [3, 1000]}, outputKernelStrideElements=1000000)
    assert tag in route and launches == 3, route


# ---- accuracy ladder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tiles.ACCURACY_CASES, ids=repr)
def test_accuracy(oracle, monkeypatch, case):
    scaffold.emu_planned(monkeypatch, case)
    accuracy.test_accuracy(oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tiles.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans both"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
