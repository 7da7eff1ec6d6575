"""CPU tier: the overlap-save route of real fftconv (lines-rconv-ols[N=P,L=L]) under host emulation.

The case table and its bars are fftconv_ols_cases.py's, shared with the GPU tier: float64 references, the same request with the switch at 0,
the route tag and 1 + K launches.  Then the planner alone on requests far beyond host memory (route, launches, workspace) and on the
neighbours whose routes the switch must not move, and the exec contract (exec_contract_cases.py's harness) on a dense and a strided request."""
import pytest

import emu_harness as emu
import fftconv_ols_cases as ols
import fftconv_ols_scaffold as scaffold
import test_emu_exec_contract as contract
from test_emu_fftconv_real import _desc, _opts


@pytest.mark.parametrize("case", ols.CASES, ids=repr)
def test_overlap_save(oracle, monkeypatch, case):
    ols.ROUTE.check_case(*scaffold.emu_runner(monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(oracle, monkeypatch):
    ols.ROUTE.check_strided(*scaffold.emu_runner(monkeypatch), oracle)


# ---- planner only ------------------------------------------------------------------------------------------------------------------

def _plan(n, kn, batch, K=1, **kw):
    desc, _ = _desc(_opts([n], [kn], batch, K=K, boundary=kw.pop("boundary", "linear-same"), **kw))
    return emu.plan_only(desc)


@pytest.mark.parametrize("n,kn,batch,K", [(5000000, 255, 16, 1), (1 << 20, 1024, 8, 1), (1 << 20, 1024, 8, 4), (100000, 129, 2048, 2)])
def test_long_lines_plan_to_the_route(n, kn, batch, K):
    """1 + K launches and a workspace of the K packed kernel spectra alone, whatever the line's length"""
    route, launches, work = _plan(n, kn, batch, K)
    assert route.startswith("lines-r2c-mapped[N=") and "lines-rconv-ols[N=" in route, route
    assert "pad[" not in route and "bluestein" not in route and "xcd" not in route, route
    assert launches == 1 + K, (route, launches)
    P = int(route.split("lines-rconv-ols[N=")[1].split(",")[0])
    L = int(route.split(",L=")[1].split("]")[0])
    assert L == (P - (kn - 1) - ((kn - 1) & 1)) & ~1 and L >= 2, route
    assert work == (K * (P // 2 + 1) * 8 + 255) // 256 * 256, (route, work)


def test_the_switch_and_the_neighbours(monkeypatch):
    ols_tag = "lines-rconv-ols["
    # the switch: 0 gives what the planner gave before the route, a block length forces it below the default rule's threshold
    assert ols_tag in _plan(9000, 33, 4)[0]
    monkeypatch.setenv("MI355FFT_RCONV_OLS", "0")
    route, launches, _ = _plan(9000, 33, 4)
    assert "pad[9032->16384]" in route and "rconv[K=1]" in route and ols_tag not in route, route
    route, launches, _ = _plan(5000000, 255, 16)
    assert "bluestein[" in route and "rconv[K=1]" in route, route
    monkeypatch.setenv("MI355FFT_RCONV_OLS", "512")
    assert "lines-rconv-ols[N=512,L=482]" in _plan(1000, 31, 4)[0]
    assert "lines-rconv-ols[N=512,L=2]" in _plan(1000, 511, 4)[0]      # the longest kernel a block takes: L >= 2
    assert ols_tag not in _plan(1000, 512, 4)[0]                        # L = 0: the routes below
    monkeypatch.setenv("MI355FFT_RCONV_OLS", "300")        # not a block length: as the default
    assert "lines-rconv[N=2048]" in _plan(1000, 31, 4)[0]
    monkeypatch.delenv("MI355FFT_RCONV_OLS")
    # requests of at most 8192 points stay on the full-line route
    assert "lines-rconv[N=8192]" in _plan(8000, 193, 4)[0]
    # RCONV_FUSED comes first
    monkeypatch.setenv("MI355FFT_RCONV_FUSED", "0")
    route = _plan(9000, 33, 4)[0]
    assert "pad[9032->16384]" in route and "rconv[K=1]" in route and "lines-rconv" not in route, route
    monkeypatch.setenv("MI355FFT_RCONV_FUSED", "2")
    assert "lines-rconv[N=32768]" in _plan(20000, 5000, 1, boundary="linear-full")[0]
    assert "lines-rconv[N=16384]" in _plan(9000, 33, 4)[0]
    monkeypatch.delenv("MI355FFT_RCONV_FUSED")
    # kernels beyond the measured limit, circular boundaries and rank 2 are not the route's
    route = _plan(40000, 9000, 2, K=2, boundary="linear-full", mode="correlation")[0]
    assert "pad[48999->65536]" in route and "rconv[K=2]" in route and "lines-rconv" not in route, route
    with pytest.raises(emu.EmuError) as e:
        _plan(40000, 9000, 2, boundary="linear-full", layout={"inputStrides": [2]})
    assert "Unsupported: strided layouts on real fftconv outside the one-launch line route" in str(e.value)
    assert "lines-rconv[N=4096]" in _plan(4096, 4096, 64, K=2, boundary="circular")[0]
    desc, _ = _desc(_opts([16384, 4], [65, 3], 2, boundary="linear-same"))
    assert ols_tag not in emu.plan_only(desc)[0]
    # strided lanes ride the route's address maps: a long strided request is planned now
    route, launches, _ = _plan(100000, 129, 4, K=2, layout={"inputStrides": [2], "outputStrides": [3]}, outputKernelStrideElements=1000000)
    assert ols_tag in route and launches == 3, route


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ols.CONTRACT_CASES, ids=repr)
def test_exec_contract(oracle, monkeypatch, case):
    """guard bands, exec offsets of 8 (mod 16), a workspace of 0xFF bytes, input and kernel untouched; no skip by route: the emulator plans both"""
    scaffold.emu_planned(monkeypatch, case)
    contract.test_exec_contract(oracle, monkeypatch, case)
