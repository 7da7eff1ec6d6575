"""GPU tier (-m gpu): long rank-1 linear fftconv requests on the HIP path.

The planner transforms them on the next power of two above shape + kernelShape - 1 (route tag pad[fN->P]); on a 2^20-point domain
with dense sides the whole request is ONE persistent launch, the VIEW form of the fftconv pipeline (kern_regtile.hpp
fft_xcd_conv1m_kernel<N1, true>).  Values: the first data lines against the reference at the EXACT logical length
(fftconv_linear_cases.py: the oracle where that length is a power of two, float64 numpy otherwise), all lines against the composed
route on the same domain (MI355FFT_CONV_PIPELINE=0) and, for one request, against the exact-length plan (MI355FFT_CONV_PAD=0)."""
import numpy as np
import pytest

import fftconv_linear_cases as cases
from test_gpu_parity import check, run_plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fft():
    import mi355fft
    return mi355fft


@pytest.fixture(scope="module")
def dev(fft):
    d = fft.Device(0)
    yield d
    d.close()


def _inputs(oracle, case, batch, seed):
    n, kn, K = case[0], case[1], case[4]
    x = oracle.random_complex_interleaved(n * batch, seed)
    kern = oracle.random_complex_interleaved(kn * K, seed + 1)
    return x, kern, [kern[2 * k * kn:2 * (k + 1) * kn] for k in range(K)]


def _check_first_lines(oracle, case, got, batch, x, kern, route):
    nb = min(batch, 3)
    want = cases.want_for(oracle, case, x, kern, nb)
    g = cases.kernel_major(got, case, batch)
    for k in range(case[4]):
        a, e = g[k, :nb].reshape(-1), want[k].reshape(-1)
        print(f"{route.strip()} kernel {k}: rel_l2={oracle.rel_l2(a, e):.3e} rel_max={oracle.rel_max(a, e):.3e}")
        check(oracle, a, e, f"{route.strip()} kernel {k}", 4e-3, 4e-3)
        assert oracle.rel_l2(a, e) < 1e-5, route


# more data lines than groups (16 on this part) in the two K = 1 cases; one case replayed through a captured graph
@pytest.mark.parametrize("name,batch,use_graph", [("full_conv_exact_2p20", 37, False), ("same_conv_batch_major", 5, False),
                                                  ("valid_corr_short_filter", 37, False), ("full_corr_wrapped_lags", 5, True),
                                                  ("circular_zero_pad", 5, False), ("same_corr_zero_write", 5, False)])
def test_fftconv_pipeline_view(fft, dev, oracle, monkeypatch, name, batch, use_graph):
    case = cases.PIPELINE_CASES[name]
    K, on = case[4], cases.geometry(case)[1]
    opts = cases.options(case, batch)
    x, kern, kernels = _inputs(oracle, case, batch, 0xD4DE)
    got, (route, _) = run_plan(fft, dev, opts, x, 2 * on * batch * K, kernel=kernels, use_graph=use_graph)
    assert "fftconv-pipeline-view[N=1024x1024,K=%d]" % K in route, route
    assert not [w for w in cases.FORBIDDEN_IN_PIPELINE_ROUTE if w in route], route
    _check_first_lines(oracle, case, got, batch, x, kern, route)
    monkeypatch.setenv("MI355FFT_CONV_PIPELINE", "0")       # every line against the composed route on the same domain
    old, (route0, _) = run_plan(fft, dev, opts, x, 2 * on * batch * K, kernel=kernels)
    assert "fftconv-pipeline" not in route0 and not [w for w in ("bluestein", "stages", "mixed") if w in route0], route0
    print(f"{route.strip()} vs {route0.strip()}: rel_l2={oracle.rel_l2(got, old):.3e}")
    assert oracle.rel_l2(got, old) < 1e-6


@pytest.mark.parametrize("name,batch", [("full_corr_32999", 3), ("same_conv_69999", 2), ("valid_conv_1999999", 2)])
def test_fftconv_padded_domain_composed_route(fft, dev, oracle, monkeypatch, name, batch):
    case = cases.COMPOSED_CASES[name]
    K, (fn, on, _) = case[4], cases.geometry(case)
    opts = cases.options(case, batch)
    x, kern, kernels = _inputs(oracle, case, batch, 0xD6DE)
    got, (route, _) = run_plan(fft, dev, opts, x, 2 * on * batch * K, kernel=kernels)
    assert "pad[%d->%d]" % (fn, 1 << (fn - 1).bit_length()) in route, route
    assert not [w for w in ("bluestein", "stages", "mixed") if w in route], route
    _check_first_lines(oracle, case, got, batch, x, kern, route)
    if name == "full_corr_32999":                            # the same request on the exact-length domain
        monkeypatch.setenv("MI355FFT_CONV_PAD", "0")
        old, (route0, _) = run_plan(fft, dev, opts, x, 2 * on * batch * K, kernel=kernels)
        assert "pad[" not in route0, route0
        print(f"{route.strip()} vs {route0.strip()}: rel_l2={oracle.rel_l2(got, old):.3e}")
        assert oracle.rel_l2(got, old) < 1e-5


def test_short_and_rank2_linear_requests_are_not_padded(fft, dev, oracle):
    for opts in ({"type": "fftconv", "shape": [100], "batch": 2, "fftConv": {"boundary": "linear-full", "kernelCount": 1, "kernelShape": [29]}},
                 {"type": "fftconv", "shape": [300, 200], "batch": 2, "fftConv": {"boundary": "linear-same", "kernelCount": 1, "kernelShape": [31, 17]}}):
        plan = fft.createPlan(dev, opts)
        route = plan.describe()[0]
        plan.destroy()
        assert "pad[" not in route and "fftconv-pipeline" not in route, route
