"""GPU tier (-m gpu): the float64 bar of accuracy_cases.py on the strided axes and on the request space around the kernels
(nd_sweep_cases.py), on the device, through the C ABI: the instance table (every column instance of line_kernels.def, the other forms of a
strided axis, N-D r2c, c2r, DCT / DST) and the seeded sweep over views, strides and plain N-D requests.  No seed is skipped here.  Every
case prints the ladder's log line (profiles/nd_sweep_gpu.log)."""
import numpy as np
import pytest

import nd_sweep_cases as nd

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


GUARD = 1 << 16         # f32 words of quiet NaN on either side of both buffers: a store outside the plan's extent lands there and fails the test


def _banded(dev, payload, words):
    """(buffer, host image) of GUARD words, `words` words that start with `payload` (NaN behind it), GUARD words"""
    host = np.full(2 * GUARD + words, np.nan, np.float32)
    if payload is not None:
        host[GUARD:GUARD + payload.size] = payload
    buf = dev.createBuffer({"size": host.nbytes})
    dev.queue.writeBuffer(buf, 0, host)
    return buf, host


def _run(fft, dev, monkeypatch, case, x, want_size, init):
    """(route, output as f32[want_size]) of one execution of the case's plan, both buffers between guard bands"""
    for k, v in case.env.items():
        monkeypatch.setenv("MI355FFT_" + k, v)
    plan = fft.createPlan(dev, case.opts)
    bufs = []
    try:
        route = plan.describe()[0]
        inp, in_host = _banded(dev, x, max(x.size, want_size) if case.in_place else x.size)
        bufs.append(inp)
        args = {"input": inp, "inputOffsetBytes": 4 * GUARD}
        if not case.in_place:
            out, out_host = _banded(dev, init, want_size)
            bufs.append(out)
            args.update(output=out, outputOffsetBytes=4 * GUARD)
        enc = dev.createCommandEncoder()
        plan.exec(enc, args)
        cb = enc.finish(use_graph=False)
        dev.queue.submit([cb])
        dev.queue.onSubmittedWorkDone()
        cb.release()
        for buf, host in ((inp, in_host),) if case.in_place else ((inp, in_host), (out, out_host)):
            after = fft.downloadF32(dev, buf, host.size)
            for band in (slice(0, GUARD), slice(host.size - GUARD, host.size)):
                assert np.array_equal(after[band].view(np.uint32), host[band].view(np.uint32)), f"{case.name} ({route.strip()}) wrote outside its buffers"
            if not case.in_place and buf is inp:
                assert np.array_equal(after.view(np.uint32), host.view(np.uint32)), f"{case.name} ({route.strip()}) changed its input"
        return route, after[GUARD:GUARD + want_size]
    finally:
        plan.destroy()
        for b in bufs:
            b.destroy()


@pytest.mark.parametrize("case", nd.TABLE, ids=repr)
def test_table(fft, dev, oracle, monkeypatch, case):
    x, _, want, keep = nd.acc.data(oracle, case)
    try:
        route, got = _run(fft, dev, monkeypatch, case, x, want.size, None)
        assert case.route_ok(route), f"{case.name} is planned as {route.strip()}, not {case.route}"
        nd.acc.measure(oracle, case, route, got, want, keep)
    finally:
        nd.acc.forget(case)


def _sweep(fft, dev, oracle, monkeypatch, family, seed):
    d = nd.draw(family, seed)
    dat = nd.data(oracle, d)
    route, got = _run(fft, dev, monkeypatch, d.case, dat.x, dat.want.size, dat.init)
    nd.check(oracle, d, route, got, dat)


@pytest.mark.parametrize("seed", range(nd.SEEDS["V"]))
def test_sweep_views(fft, dev, oracle, monkeypatch, seed):
    _sweep(fft, dev, oracle, monkeypatch, "V", seed)


@pytest.mark.parametrize("seed", range(nd.SEEDS["S"]))
def test_sweep_strides(fft, dev, oracle, monkeypatch, seed):
    _sweep(fft, dev, oracle, monkeypatch, "S", seed)


@pytest.mark.parametrize("seed", range(nd.SEEDS["P"]))
def test_sweep_plain(fft, dev, oracle, monkeypatch, seed):
    _sweep(fft, dev, oracle, monkeypatch, "P", seed)
