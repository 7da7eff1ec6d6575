"""GPU tier (-m gpu): the overlap-save route of real fftconv (lines-rconv-ols[N=P,L=L]) through the C ABI.

The case table and its bars are fftconv_ols_cases.py's, shared with the CPU tier.  On the device as well: one recorded list replayed three
times as an op list and as a captured graph, one full-size request checked against the planner's earlier route with device reductions,
and the exec contract (test_gpu_exec_contract.py's harness) on a dense and a strided request."""
import numpy as np
import pytest

import fftconv_ols_cases as ols
import fftconv_ols_scaffold as scaffold
import test_gpu_exec_contract as contract
from test_emu_fftconv_real import _check, _opts, _rand, _want
from test_gpu_exec_contract import dev, fft, harness  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ols.CASES, ids=repr)
def test_overlap_save(fft, dev, oracle, monkeypatch, case):
    ols.ROUTE.check_case(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle, case)


def test_strided_lanes_on_both_sides(fft, dev, oracle, monkeypatch):
    ols.ROUTE.check_strided(*scaffold.gpu_runner(fft, dev, monkeypatch), oracle)


@pytest.mark.parametrize("use_graph", [False, True])
def test_replay_of_a_recorded_list(fft, dev, oracle, monkeypatch, use_graph):
    n, kn, batch, K = 5000, 31, 37, 2
    monkeypatch.setenv("MI355FFT_RCONV_OLS", "256")
    x, h = _rand(n * batch, 0x0191), _rand(kn * K, 0x0192)
    want = _want(x, h, [n], [kn], batch, K, "convolution", "linear-same")
    plan = fft.createPlan(dev, _opts([n], [kn], batch, K=K, boundary="linear-same"))
    inp = dev.createBuffer({"size": x.nbytes})
    dev.queue.writeBuffer(inp, 0, x)
    out = dev.createBuffer({"size": 4 * n * batch * K})
    enc = dev.createCommandEncoder()
    plan.exec(enc, {"input": inp, "output": out, "kernel": h})
    cb = enc.finish(use_graph=use_graph)
    route, launches = plan.describe()
    assert "lines-rconv-ols[N=256,L=226]" in route and launches == 1 + K, (route, launches)
    for rep in range(3):
        dev.queue.writeBuffer(out, 0, np.full(n * batch * K, 777.0, np.float32))
        dev.queue.submit([cb])
        dev.queue.onSubmittedWorkDone()
        got = fft.downloadF32(dev, out, n * batch * K)
        _check(oracle, got, want, batch, K, "kernel-major", f"{route.strip()} replay {rep} graph={use_graph}")
    cb.release()
    plan.destroy()
    inp.destroy()
    out.destroy()


def test_full_size_against_the_earlier_route_on_the_device(fft, dev, monkeypatch):
    """64 lines of 2^20 points (256 MiB of input), 255 taps, linear-same: every output of the planner's own rule against the route the
    switch's 0 restores"""
    n, kn, batch = 1 << 20, 255, 64
    opts = _opts([n], [kn], batch, boundary="linear-same")
    h = _rand(kn, 0x01F2)
    inp = dev.createBuffer({"size": 4 * n * batch})
    dev.fillRandom(inp, 0, n, batch, 0xF1F2)
    outs, routes = [], []
    for switch in (None, "0"):
        if switch is not None:
            monkeypatch.setenv("MI355FFT_RCONV_OLS", switch)
        plan = fft.createPlan(dev, opts)
        out = dev.createBuffer({"size": 4 * n * batch})
        enc = dev.createCommandEncoder()
        plan.exec(enc, {"input": inp, "output": out, "kernel": h})
        dev.queue.submit([enc.finish()])
        dev.queue.onSubmittedWorkDone()
        routes.append(plan.describe())
        plan.destroy()
        outs.append(out)
    assert "lines-rconv-ols[N=" in routes[0][0] and routes[0][1] == 2, routes[0]
    assert "rconv[K=1]" in routes[1][0] and "lines-rconv" not in routes[1][0], routes[1]
    count = n * batch
    ref = dev.sumsq(outs[1], 0, count)
    diff = dev.diffSumsq(outs[0], 0, outs[1], 0, 1.0, count)
    rel = float(np.sqrt(diff / ref))
    print(f"{routes[0][0].strip()} vs {routes[1][0].strip()}: {count} outputs, rel_l2={rel:.3e}, rms={np.sqrt(ref / count):.3e}")
    assert ref > 0 and rel < 1e-6
    for b in outs + [inp]:
        b.destroy()


# ---- exec contract -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("harness", ols.CONTRACT_CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):  # noqa: F811
    contract.test_exec_contract(harness, oracle)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", ols.CONTRACT_CASES, ids=repr, indirect=True)
def test_replay(harness, use_graph):  # noqa: F811
    contract.test_replay(harness, use_graph)
