"""CPU tier: the overlap-save route of complex fftconv (lines-conv-ols[N=P,L=L]) under host emulation.

The case table and its bars are fftconv_cols_cases.py's, shared with the GPU tier: float64 references, the same request with the switch at 0,
the route tag and 1 + K launches.  Then the planner alone on requests far beyond host memory (route, launches, workspace: the capability
the route adds) and on the neighbours whose routes the switch must not move, the accuracy ladder, and the exec contract
(exec_contract_cases.py's harness: guard bands catch a load or store outside a block's predicates) on a dense and a strided request."""
import pytest

import emu_harness as emu
import fftconv_cols_cases as cols
import fftconv_linear_cases as lin
import fftconv_ols_scaffold as scaffold
import test_emu_accuracy as accuracy
import test_emu_exec_contract as contract
from test_emu_fftconv import _desc


@pytest.mark.parametrize("case", cols.CASES, ids=repr)
def test_overlap_save(oracle, monkeypatch, case):
    cols.ROUTE.check_case(*scaffold.emu_runner(monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(oracle, monkeypatch):
    cols.ROUTE.check_strided(*scaffold.emu_runner(monkeypatch), oracle)


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(n, kn, batch, K=1, boundary="linear-same", mode="convolution", layout=None, **fc):
    opts = lin.options((n, kn, boundary, mode, K, "kernel-major", None), batch)
    opts["fftConv"].update(fc)
    if layout:
        opts["layout"] = layout
    return emu.plan_only(_desc(opts)[0])


@pytest.mark.parametrize("n,kn,batch,K", [(5000000, 255, 1, 1), (1 << 20, 255, 256, 1)])
def test_capability_long_lines_plan_to_the_route(n, kn, batch, K):
    """a complex line of 5000000 points (an error before the route: Bluestein axis above 2^22) and 256 lines of 2^20 points (12 launches and 9 GB of
    workspace before it): 1 + K launches and the K kernel spectra alone as workspace"""
    route, launches, work = _plan(n, kn, batch, K)
    assert route.startswith("lines-mapped[N=") and cols.ROUTE.tag in route, route
    assert not any(f in route for f in cols.ROUTE.forbidden), route
    assert launches == 1 + K, (route, launches)
    P = int(route.split(cols.ROUTE.tag + "N=")[1].split(",")[0])
    L = int(route.split(",L=")[1].split("]")[0])
    assert L == P - (kn - 1) and L >= 2, route
    assert work < 1 << 20 and work >= K * P * 8, (route, work)


def test_requests_that_were_an_error(monkeypatch):
    """exact-length domains above 2^22 that are not 13-smooth: a route where the planner raised Unsupported"""
    for n, kn, batch in ((5000000, 255, 16), (4194304, 255, 4), (6000000, 33, 2)):
        route, launches, work = _plan(n, kn, batch)
        assert cols.ROUTE.tag in route and launches == 2 and work < 1 << 20, (route, launches, work)
    monkeypatch.setenv("MI355FFT_CONV_OLS", "0")
    with pytest.raises(emu.EmuError) as e:
        _plan(5000000, 255, 16)
    assert "Unsupported: Bluestein axis length 5000254 exceeds 2^22" in str(e.value)


def test_the_default_rule():
    """the block length: the smallest power of two >= 8 (M - 1), from 2048 up to 4096"""
    for kn, P in ((1, 2048), (31, 2048), (129, 2048), (255, 2048), (257, 2048), (258, 4096), (513, 4096)):
        assert f"{cols.ROUTE.tag}N={P},L={P - kn + 1}]" in _plan(100000, kn, 4)[0], (kn, P)


def test_the_switch_and_the_neighbours(monkeypatch):
    tag = cols.ROUTE.tag
    # the switch: 0 gives what the planner gave before the route, a block length forces it below the default rule's threshold
    assert tag in _plan(100000, 129, 4)[0]
    monkeypatch.setenv("MI355FFT_CONV_OLS", "0")
    route = _plan(100000, 129, 4)[0]
    assert "pad[100128->131072]" in route and "fftconv[K=1]" in route and tag not in route, route
    monkeypatch.setenv("MI355FFT_CONV_OLS", "512")
    assert f"{tag}N=512,L=482]" in _plan(1000, 31, 4)[0]
    assert f"{tag}N=512,L=2]" in _plan(1000, 511, 4)[0]        # the longest kernel a block takes: L >= 2
    assert tag not in _plan(1000, 512, 4)[0]                   # L = 1: the routes below
    assert f"{tag}N=512,L=" in _plan(100000, 129, 4, boundary="linear-full", mode="correlation")[0]
    for bad in ("300", "64", "8192"):                          # not a block length of the route: the other routes
        monkeypatch.setenv("MI355FFT_CONV_OLS", bad)
        assert tag not in _plan(1000, 31, 4)[0], bad
    monkeypatch.delenv("MI355FFT_CONV_OLS")
    # requests of at most 16384 points, kernels beyond 513 points, circular boundaries and rank 2 keep their routes
    assert tag not in _plan(16354, 31, 4)[0] and tag in _plan(16355, 31, 4)[0]
    route = _plan(700000, 1000, 2, boundary="linear-valid", mode="correlation")[0]
    assert tag not in route and "pad[700999->1048576]" in route, route
    assert tag not in _plan(100000, 514, 4)[0] and tag in _plan(100000, 513, 4)[0]
    assert tag not in _plan(1 << 17, 129, 4, boundary="circular")[0]
    opts = {"type": "fftconv", "shape": [32768, 4], "batch": 2, "fftConv": {"boundary": "linear-same", "kernelCount": 1, "kernelShape": [65, 3]}}
    assert tag not in emu.plan_only(_desc(opts)[0])[0]
    # CONV_LINES = 0 and FORCE_GENERIC = 1 switch the route off, as they do for the other line routes
    for name in ("MI355FFT_CONV_LINES", "MI355FFT_FORCE_GENERIC"):
        monkeypatch.setenv(name, "0" if name.endswith("LINES") else "1")
        assert tag not in _plan(100000, 129, 4)[0], name
        monkeypatch.delenv(name)
    # strided lanes ride the route's address maps
    route, launches, _ = _plan(100000, 129, 4, K=2, layout={"interleavedComplex": True, "inputStrides": [2], "outputStrides": [3]}, outputKernelStrideElements=1000000)
    assert tag in route and launches == 3, route


# ---- accuracy ladder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cols.ACCURACY_CASES, ids=repr)
def test_accuracy(oracle, monkeypatch, case):
    scaffold.emu_planned(monkeypatch, case)
    accuracy.test_accuracy(oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cols.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans both"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
