"""GPU tier (-m gpu): the rounding error of every route of accuracy_cases.py on the device, through the C ABI, against a float64 transform
of the same f32 input.

One case per test: the plan must take the route the table names, its output must be finite, and its error is held to 4 Y in rel_l2 and to
8 Y over the worst class of outputs (every batch line; for long rank-1 lines the residues and blocks of the four-step split; for rank > 1
every index of every axis), Y being the
f32 oracle's own error against float64 measured in this process (accuracy_cases.py).  Output elements the plan's contract leaves alone
start as NaN and are left out.  Every case prints one line: route, both values, Y, both ratios (profiles/accuracy_ladder.log)."""
import numpy as np
import pytest

import accuracy_cases as acc

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


def _upload(dev, host, nbytes=None):
    buf = dev.createBuffer({"size": max(nbytes or host.nbytes, 8)})
    dev.queue.writeBuffer(buf, 0, host)
    return buf


@pytest.mark.parametrize("case", acc.CASES, ids=repr)
def test_accuracy(fft, dev, oracle, monkeypatch, case):
    for k, v in case.env.items():
        monkeypatch.setenv("MI355FFT_" + k, v)
    plan = fft.createPlan(dev, case.opts)
    bufs = []
    try:
        route = plan.describe()[0]
        assert case.route_ok(route), f"{case.name} is planned as {route.strip()}, not {case.route}"
        x, kern, want, keep = acc.data(oracle, case)
        nbytes = 4 * want.size
        inp = _upload(dev, x, max(x.nbytes, nbytes) if case.in_place else None)
        bufs.append(inp)
        args = {"input": inp}
        if not case.in_place:
            out = _upload(dev, np.full(want.size, np.nan, np.float32)) if keep.any() else dev.createBuffer({"size": max(nbytes, 8)})
            bufs.append(out)
            args["output"] = out
        if kern is not None:
            kb = _upload(dev, kern)
            bufs.append(kb)
            args["kernel"] = kb
        enc = dev.createCommandEncoder()
        plan.exec(enc, args)
        cb = enc.finish(use_graph=False)
        dev.queue.submit([cb])
        dev.queue.onSubmittedWorkDone()
        cb.release()
        got = fft.downloadF32(dev, inp if case.in_place else out, want.size)
        acc.measure(oracle, case, route, got, want, keep)
    finally:
        plan.destroy()
        for b in bufs:
            b.destroy()
        if want_size_of(case) > 1 << 20:
            acc.forget(case)


def want_size_of(case):
    return int(np.prod(case.opts["shape"])) * case.opts["batch"]
