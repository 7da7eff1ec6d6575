"""CPU tier: long rank-1 linear fftconv requests (planner + kernels under host emulation).

A linear result is cropped out of the FFT domain, so the planner transforms on the next power of two above
shape + kernelShape - 1 (route tag pad[fN->P]) instead of the exact length; on a 2^20-point domain with dense sides the whole
request is the one-launch pipeline in its VIEW form (kern_regtile.hpp fft_xcd_conv1m_kernel<N1, true>: the embed of the data is a
predicate of the first loads, crop and zeroPad.write are predicates of the last stores).  Values against the float64 reference at
the exact logical length (fftconv_linear_cases.py) and against the composed route; planner-only checks of the switches."""
import numpy as np
import pytest

import emu_harness as emu
import fftconv_linear_cases as cases
from test_emu_fftconv import _close, _desc


def _run(oracle, case, batch, seed):
    n, kn, K = case[0], case[1], case[4]
    x = oracle.random_complex_interleaved(n * batch, seed)
    kern = oracle.random_complex_interleaved(kn * K, seed + 1)
    desc, _ = _desc(cases.options(case, batch))
    on = cases.geometry(case)[1]
    got, route, launches = emu.run_plan(desc, x, 2 * on * batch * K, kernel=kern)
    return x, kern, desc, got, route


@pytest.mark.parametrize("name,cus", [("full_conv_exact_2p20", 2), ("full_corr_wrapped_lags", 3), ("circular_zero_pad", 2)])
def test_fftconv_pipeline_view_2p20(oracle, monkeypatch, name, cus):
    """rows 1, 4 and 5 of the table: an exact 2^20 linear domain, a padded correlation whose wrapped negative lags are part of the
    output, and circular lines with zeroPad.read / zeroPad.write"""
    monkeypatch.setenv("MI355_EMU_XCD_FUSED", "1")
    monkeypatch.setenv("MI355_EMU_CUS", str(cus))
    monkeypatch.setenv("MI355_EMU_XCDS", "1")
    case, batch = cases.PIPELINE_CASES[name], 2
    K = case[4]
    x, kern, desc, got, route = _run(oracle, case, batch, 0xD4DE)
    assert "fftconv-pipeline-view[N=1024x1024,K=%d]" % K in route, route
    assert not [w for w in cases.FORBIDDEN_IN_PIPELINE_ROUTE if w in route], route
    want = cases.want_for(oracle, case, x, kern, batch)
    g = cases.kernel_major(got, case, batch)
    for k in range(K):
        _close(g[k].reshape(-1), want[k].reshape(-1), 4e-3, 4e-3, f"{route.strip()} kernel {k}")
        assert oracle.rel_l2(g[k].reshape(-1), want[k].reshape(-1)) < 1e-5, route
    monkeypatch.setenv("MI355_EMU_CONV_PIPELINE", "0")       # the composed route on the same domain
    on = cases.geometry(case)[1]
    old, route0, _ = emu.run_plan(desc, x, 2 * on * batch * K, kernel=kern)
    assert "fftconv-pipeline" not in route0 and not [w for w in ("bluestein", "stages", "mixed") if w in route0], route0
    assert oracle.rel_l2(got, old) < 1e-6, (route, route0)


def test_fftconv_padded_domain_composed_route(oracle):
    """[20000] (*) [13000] linear-full correlation, K = 2: logical FFT length 32999 -> 65536; zero + embed, forward, products, inverse
    and the crop in two pieces (positive lags from the bottom of the padded domain, negative lags from its top)"""
    case, batch = cases.COMPOSED_CASES["full_corr_32999"], 2
    K = case[4]
    x, kern, desc, got, route = _run(oracle, case, batch, 0xD6DE)
    assert "pad[32999->65536]" in route and "fftconv[K=2]" in route, route
    assert not [w for w in ("bluestein", "stages", "mixed") if w in route], route
    want = cases.want_for(oracle, case, x, kern, batch)
    g = cases.kernel_major(got, case, batch)
    for k in range(K):
        _close(g[k].reshape(-1), want[k].reshape(-1), 4e-3, 4e-3, f"{route.strip()} kernel {k}")
        assert oracle.rel_l2(g[k].reshape(-1), want[k].reshape(-1)) < 1e-5, route


@pytest.mark.parametrize("name", sorted(cases.PIPELINE_CASES))
def test_planner_routes_of_the_2p20_domain(monkeypatch, name):
    """planner only, every row of the table at the product's defaults and under its two switches"""
    case = cases.PIPELINE_CASES[name]
    desc, _ = _desc(cases.options(case, 37))
    fn = cases.geometry(case)[0]
    route, launches, _ = emu.plan_only(desc)
    assert "fftconv-pipeline-view[N=1024x1024,K=%d]" % case[4] in route, route
    assert not [w for w in cases.FORBIDDEN_IN_PIPELINE_ROUTE if w in route], route
    assert ("pad[%d->1048576]" % fn in route) == (fn != 1 << 20), route
    monkeypatch.setenv("MI355FFT_CONV_PIPELINE", "0")
    route0, launches0, _ = emu.plan_only(desc)
    assert "fftconv-pipeline" not in route0 and not [w for w in ("bluestein", "stages", "mixed") if w in route0], route0
    assert launches0 > launches
    monkeypatch.setenv("MI355FFT_CONV_PAD", "0")              # the exact-length domain
    route1, _, _ = emu.plan_only(desc)
    assert "pad[" not in route1 and "fftconv-pipeline" not in route1, route1
    if fn & (fn - 1):
        assert [w for w in ("bluestein", "stages", "mixed") if w in route1], route1


@pytest.mark.parametrize("name", sorted(cases.COMPOSED_CASES))
def test_planner_pads_long_linear_domains(monkeypatch, name):
    case = cases.COMPOSED_CASES[name]
    desc, _ = _desc(cases.options(case, 3))
    fn = cases.geometry(case)[0]
    p = 1 << (fn - 1).bit_length()
    route, _, work = emu.plan_only(desc)
    assert "pad[%d->%d]" % (fn, p) in route and not [w for w in ("bluestein", "stages", "mixed") if w in route], route
    monkeypatch.setenv("MI355FFT_CONV_PAD", "0")
    route0, _, _ = emu.plan_only(desc)
    assert "pad[" not in route0, route0


def test_planner_leaves_other_requests_alone(monkeypatch):
    """short linear lines, rank 2, circular lines and domains above 2^22 keep the exact-length domain (same route, launches and workspace
    as with the switch off)"""
    reqs = [
        {"type": "fftconv", "shape": [100], "batch": 2, "fftConv": {"boundary": "linear-full", "kernelCount": 1, "kernelShape": [29]}},
        {"type": "fftconv", "shape": [16000], "batch": 2, "fftConv": {"boundary": "linear-full", "kernelCount": 1, "kernelShape": [385]}},   # 16384
        {"type": "fftconv", "shape": [300, 200], "batch": 2, "fftConv": {"boundary": "linear-same", "kernelCount": 1, "kernelShape": [31, 17]}},
        {"type": "fftconv", "shape": [40000], "batch": 2, "fftConv": {"boundary": "circular", "kernelCount": 1, "kernelShape": [30000]}},
        {"type": "fftconv", "shape": [6291000], "batch": 1, "fftConv": {"boundary": "linear-full", "kernelCount": 1, "kernelShape": [457]}},   # 3 * 2^21 > 2^22
    ]
    for opts in reqs:
        desc, _ = _desc(opts)
        monkeypatch.delenv("MI355FFT_CONV_PAD", raising=False)
        on = emu.plan_only(desc)
        monkeypatch.setenv("MI355FFT_CONV_PAD", "0")
        off = emu.plan_only(desc)
        assert "pad[" not in on[0] and on == off, (opts, on, off)
