"""GPU tier (-m gpu): the overlap-save route of complex fftconv (lines-conv-ols[N=P,L=L]) through the C ABI.

The case table and its bars are fftconv_cols_cases.py's, shared with the CPU tier.  On the device as well: the capability the route adds (a
line of 5000000 complex points, an error before it) against float64 direct sums on three windows, one full-size request of the planner's
own rule checked against the planner's earlier route with device reductions, the accuracy ladder, and the exec contract and replay
(test_gpu_exec_contract.py's harness) on a dense and a strided request."""
import numpy as np
import pytest

import fftconv_cols_cases as cols
import fftconv_linear_cases as lin
import fftconv_ols_scaffold as scaffold
import test_gpu_accuracy as accuracy
import test_gpu_exec_contract as contract
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)
from test_gpu_parity import run_plan

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", cols.CASES, ids=repr)
def test_overlap_save(fft, dev, oracle, monkeypatch, case):
    cols.ROUTE.check_case(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch):
    cols.ROUTE.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle)


def test_capability_a_line_of_5000000_points(fft, dev):
    """1 x 5000000 (*) 255 linear-same (40 MB each way; the planner raised Unsupported before the route): three windows of 4096 outputs, the
    head, one straddling a block boundary and the tail, against float64 direct sums"""
    n, kn = 5000000, 255
    x, h = cols.ROUTE.rand(n, 0x0CF1), cols.ROUTE.rand(kn, 0x0CF2)
    opts = lin.options((n, kn, "linear-same", "convolution", 1, "kernel-major", None), 1)
    got, (route, launches) = run_plan(fft, dev, opts, x, 2 * n, kernel=h)
    assert cols.ROUTE.tag in route and launches == 2 and not any(f in route for f in cols.ROUTE.forbidden), (route, launches)
    L = int(route.split(",L=")[1].split("]")[0])
    mid = (n // 2) // L * L - (kn - 1) // 2          # output index of the first result of a block
    got = got.reshape(n, 2)
    for lo in (0, mid - 2048, n - 4096):
        want = cols.ROUTE.direct_same_conv(x, h, (n,), (kn,), (lo,), (lo + 4096,))
        g = got[lo:lo + 4096, 0].astype(np.float64) + 1j * got[lo:lo + 4096, 1]
        err = np.abs(g - want)
        rel = float(np.linalg.norm(g - want) / np.linalg.norm(want))
        print(f"{route.strip()} outputs [{lo}, {lo + 4096}): rel_l2={rel:.3e} max_abs={err.max():.3e}")
        assert np.all(err <= 4e-3 + 4e-3 * np.abs(want)) and rel < 1e-5, (lo, rel)


def test_full_size_against_the_earlier_route_on_the_device(fft, dev, monkeypatch):
    """32 lines of 2^20 complex points (256 MiB of input), 255 taps, linear-same: every output of the planner's own rule against the route the
    switch's 0 restores"""
    n, kn, batch = 1 << 20, 255, 32
    opts = lin.options((n, kn, "linear-same", "convolution", 1, "kernel-major", None), batch)
    h = cols.ROUTE.rand(kn, 0x0CF3)
    inp = dev.createBuffer({"size": 8 * n * batch})
    dev.fillRandom(inp, 0, 2 * n, batch, 0xC1F2)
    outs, routes = [], []
    for switch in (None, "0"):
        if switch is not None:
            monkeypatch.setenv("MI355FFT_CONV_OLS", switch)
        plan = fft.createPlan(dev, opts)
        out = dev.createBuffer({"size": 8 * n * batch})
        enc = dev.createCommandEncoder()
        plan.exec(enc, {"input": inp, "output": out, "kernel": h})
        dev.queue.submit([enc.finish()])
        dev.queue.onSubmittedWorkDone()
        routes.append(plan.describe())
        plan.destroy()
        outs.append(out)
    assert cols.ROUTE.tag in routes[0][0] and routes[0][1] == 2, routes[0]
    assert "fftconv[K=1]" in routes[1][0] and cols.ROUTE.tag not in routes[1][0], routes[1]
    count = 2 * n * batch
    ref = dev.sumsq(outs[1], 0, count)
    diff = dev.diffSumsq(outs[0], 0, outs[1], 0, 1.0, count)
    rel = float(np.sqrt(diff / ref))
    print(f"{routes[0][0].strip()} vs {routes[1][0].strip()}: {count} outputs, rel_l2={rel:.3e}, rms={np.sqrt(ref / count):.3e}")
    assert ref > 0 and rel <= 1e-5
    for b in outs + [inp]:
        b.destroy()


# ---- accuracy ladder ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cols.ACCURACY_CASES, ids=repr)
def test_accuracy(fft, dev, oracle, monkeypatch, case):
    accuracy.test_accuracy(fft, dev, oracle, monkeypatch, case)


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", cols.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", cols.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
