"""GPU tier (-m gpu): boundary "circular" on the six overlap-save routes of fftconv (route tags ending in ",wrap]") through the C ABI.

The case table and its bars are fftconv_circular_cases.py's, shared with the CPU tier.  On the device as well: the capabilities the routes add
(a complex circular line of 5000000 points against float64 direct circular sums on three windows, its neighbour of 5000001 points that had no
plan, real requests on strided sides that had no plan), and the exec contract and replay (test_gpu_exec_contract.py's harness) on a dense and
a strided request per route."""
import numpy as np
import pytest

import fftconv_circular_cases as circ
import fftconv_ols_scaffold as scaffold
import test_gpu_exec_contract as contract
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)
from test_gpu_parity import run_plan

pytestmark = pytest.mark.gpu

ENV = "MI355FFT_" + circ.SWITCH


@pytest.mark.parametrize("rc", circ.CASES, ids=circ.case_id)
def test_circular_overlap_save(fft, dev, oracle, monkeypatch, rc):
    route, case = rc
    route.check_case(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, case)


@pytest.mark.parametrize("route", circ.ROUTES, ids=lambda r: r.tag[:-1])
def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch, route):
    """with the switch at 0 the real requests have no plan (the capability the real routes add), the complex ones their earlier plan"""
    def unsupported(opts):
        with pytest.raises(Exception) as e:
            fft.createPlan(dev, opts)
        assert circ.UNSUPPORTED in str(e.value), e.value
    route.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, unsupported)


def _direct_circular(x, h, n, lo, hi, corr=False):
    """outputs [lo, hi) of the circular convolution (correlation) of one complex line of n points, float64 direct sums"""
    xc = np.asarray(x, np.float64).reshape(-1, 2)[:n]
    xc = xc[:, 0] + 1j * xc[:, 1]
    hc = np.asarray(h, np.float64).reshape(-1, 2)
    hc = hc[:, 0] + 1j * hc[:, 1]
    m = np.arange(lo, hi)
    out = np.zeros(hi - lo, np.complex128)
    for t, ht in enumerate(hc):
        out += (np.conj(ht) * xc[(m + t) % n]) if corr else (ht * xc[(m - t) % n])
    return out


@pytest.mark.parametrize("n", [5000000, 5000001])
def test_capability_a_circular_line_of_5000000_points(fft, dev, monkeypatch, n):
    """1 x n (*) 255 circular (40 MB each way): the windows [0, 300), [n / 2, n / 2 + 300) and [n - 300, n) against float64 direct circular sums.
    With the switch at 0, 5000000 (13-smooth) takes 30 per-radix stage launches, and 5000001 has no plan (a Bluestein axis beyond 2^22)"""
    kn = 255
    x, h = circ.LINES.rand(n, 0xC1F1), circ.LINES.rand(kn, 0xC1F2)
    opts = circ.LINES.options((n,), (kn,), 1, boundary="circular")
    got, (route, launches) = run_plan(fft, dev, opts, x, 2 * n, kernel=h)
    assert circ.LINES.tag_of(2048, (kn,)) in route and launches == 2 and not any(f in route for f in circ.LINES.forbidden), (route, launches)
    got = np.asarray(got).reshape(n, 2)
    for lo in (0, n // 2, n - 300):
        want = _direct_circular(x, h, n, lo, lo + 300)
        g = got[lo:lo + 300, 0].astype(np.float64) + 1j * got[lo:lo + 300, 1]
        err = np.abs(g - want)
        rel = float(np.linalg.norm(g - want) / np.linalg.norm(want))
        print(f"{route.strip()} outputs [{lo}, {lo + 300}): rel_l2={rel:.3e} max_abs={err.max():.3e}")
        assert np.all(err <= 4e-3 + 4e-3 * np.abs(want)) and rel < 1e-5, (lo, rel)
    if n == 5000001:
        monkeypatch.setenv(ENV, "0")
        with pytest.raises(Exception) as e:
            fft.createPlan(dev, opts)
        assert "Unsupported: Bluestein axis length" in str(e.value), e.value


def test_capability_an_odd_real_line_is_not_widened(fft, dev):
    plan = fft.createPlan(dev, circ.RLINES.options((8193,), (31,), 3, boundary="circular"))
    route, launches = plan.describe()
    plan.destroy()
    assert circ.RLINES.tag_of(1024, (31,)) in route and "rconv-widened" not in route and "pad[" not in route and launches == 2, (route, launches)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", circ.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", circ.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
