"""GPU tier (-m gpu): the exec contract of plan.exec on every route family of exec_contract_cases.py.

A plain run (buffers of the plan's own size at offset 0, the plan's arena) is held to the route's oracle bar.  Then the same plan runs with
every side inside a larger buffer, 1 MiB of poison (one quiet-NaN bit pattern, written and compared as uint32) before and after it: input,
output and kernel at byte offsets of 8 (mod 16) (f16 plans: 4), and once more with the input aligned and the output not; the workspace is
a caller's `temp` of exactly getWorkspaceSizeBytes() bytes, wrapped over an allocation with 1 MiB more behind it, all poison.  Each such run must give the plain run's output bit for bit
(pointer shifts and the workspace's origin change no arithmetic, and no kernel accumulates floats atomically), leave every guard word, the
input and the kernel buffers as they were, and leave output elements that the plan's contract does not write holding the poison.  A read
outside the input range that feeds the result shows as NaN.  Routes with a control block or a workspace, and one plain line route, are
also recorded twice in one encoder and submitted twice, as an op list and as a captured graph.  Out-of-place c2c plans run once with the
output on the input."""
import numpy as np
import pytest

import exec_contract_cases as t

pytestmark = pytest.mark.gpu
G = t.GUARD_BYTES


@pytest.fixture(scope="module")
def fft():
    import mi355fft
    return mi355fft


@pytest.fixture(scope="module")
def dev(fft):
    d = fft.Device(0)
    yield d
    d.close()


def _read(fft, buf, nbytes, offset=0):
    out = np.empty(nbytes, np.uint8)
    fft._chk(fft.lib().mi355fft_buffer_read(buf._h, offset, out.ctypes.data, nbytes))
    return out


def _upload(dev, host):
    buf = dev.createBuffer({"size": host.nbytes})
    dev.queue.writeBuffer(buf, 0, host)
    return buf


def _poison(dev, buf):
    """fills a buffer (a multiple of 16 bytes) with the poison pattern: 1 MiB from the host, doubled on the device"""
    nbytes = buf.size
    done = min(nbytes, 1 << 20)
    dev.queue.writeBuffer(buf, 0, t.poison_words(done))
    enc = dev.createCommandEncoder()
    while done < nbytes:
        step = min(done, nbytes - done)
        enc.copyBufferToBuffer(buf, 0, buf, done, step)
        done += step
    dev.queue.submit([enc.finish()])
    dev.queue.onSubmittedWorkDone()


def _assert_poison(raw, what):
    bad = np.flatnonzero(raw.view(np.uint32) != t.POISON)
    assert bad.size == 0, f"{what}: {bad.size} guard words were written, the first at word {int(bad[0])}"


def _assert_guards(raw, off, nbytes, what):
    _assert_poison(raw[:off], what + " (before the range)")
    _assert_poison(raw[off + (nbytes + 3) // 4 * 4:], what + " (after the range)")


class Harness:
    """one case's plan, data and device buffers; every run leaves its buffers destroyed"""

    def __init__(self, fft, dev, oracle, case):
        self.fft, self.dev, self.case = fft, dev, case
        self.plan = fft.createPlan(dev, case.opts)
        self.route = self.plan.describe()[0]
        assert case.route_ok(self.route), f"{case.name} is planned as {self.route.strip()}, not {case.route}"
        self.x, self.kern, self.want, self.keep = t.data(oracle, case)
        self.nbytes = (self.want.size * (2 if case.f16 else 4) + 3) // 4 * 4
        self.pad = 4 if case.f16 else 8
        self.work = self.plan.getWorkspaceSizeBytes()
        assert case.replay or not self.work, f"{case.name} has a workspace of {self.work} bytes: set replay=True in the table"
        self.temp_guard_at = (self.work + 15) // 16 * 16
        # the caller's temp is a buffer of exactly the workspace size, wrapped over the head of an allocation whose last 1 MiB is the guard
        self.temp_alloc = dev.createBuffer({"size": self.temp_guard_at + G}) if self.work else None
        self.temp = dev.wrapBuffer(self.temp_alloc.device_ptr, self.temp_guard_at) if self.work else None

    def close(self):
        self.plan.destroy()
        if self.temp is not None:
            self.temp.destroy()
            self.temp_alloc.destroy()

    def run(self, guard, in_pad, out_pad, kernel_pad, temp, alias=False, what=""):
        """one exec, one submit; returns the output range's bytes after checking everything around it"""
        case, fft, dev = self.case, self.fft, self.dev
        alias = alias or case.in_place
        in_host = t.banded(self.x, guard, in_pad, max(self.x.nbytes, self.nbytes) if alias else self.x.nbytes)
        ib = _upload(dev, in_host)
        ob = None if alias else _upload(dev, t.banded(np.empty(0, np.uint8), guard, out_pad, self.nbytes))
        k_host = None if self.kern is None else t.banded(self.kern, guard, kernel_pad, self.kern.nbytes)
        kb = None if k_host is None else _upload(dev, k_host)
        args = {"input": ib, "inputOffsetBytes": guard + in_pad}
        if not case.in_place:
            args.update(output=ib if alias else ob, outputOffsetBytes=guard + (in_pad if alias else out_pad))
        if kb is not None:
            args.update(kernel=kb, kernelOffsetBytes=guard + kernel_pad)
        temp = temp and self.temp is not None
        if temp:
            _poison(dev, self.temp_alloc)
            args["temp"] = self.temp
        try:
            enc = dev.createCommandEncoder()
            self.plan.exec(enc, args)
            cb = enc.finish(use_graph=False)
            dev.queue.submit([cb])
            dev.queue.onSubmittedWorkDone()
            cb.release()
            in_after = _read(fft, ib, in_host.nbytes)
            if alias:
                _assert_guards(in_after, guard + in_pad, max(self.x.nbytes, self.nbytes), f"{what}: input")
                out = in_after[guard + in_pad:guard + in_pad + self.nbytes]
            else:
                assert np.array_equal(in_after, in_host), f"{what}: the input buffer was written"
                out_after = _read(fft, ob, ob.size)
                _assert_guards(out_after, guard + out_pad, self.nbytes, f"{what}: output")
                out = out_after[guard + out_pad:guard + out_pad + self.nbytes]
            if kb is not None:
                assert np.array_equal(_read(fft, kb, k_host.nbytes), k_host), f"{what}: the kernel buffer was written"
            if temp:
                self.check_temp(what, used=not alias or case.in_place)
            return out.copy(), in_host
        finally:
            for b in (ib, ob, kb):
                if b is not None:
                    b.destroy()

    def check_temp(self, what, used=True):
        """nothing behind the workspace was written; used: and the run did work in the caller's temp (exec falls back to the plan's arena
        without a word, which would make every temp assertion empty).  Not asked of a run on one buffer: an ioView plan's staged twin
        needs more workspace than the plan reports and runs on its own arena."""
        _assert_poison(_read(self.fft, self.temp_alloc, G, self.temp_guard_at), f"{what}: behind the workspace")
        at, written = 0, False
        while used and not written and at < self.work:
            n = min(4 << 20, (self.work - at) // 4 * 4)
            if not n:
                break
            written = bool(np.any(_read(self.fft, self.temp, n, at).view(np.uint32) != t.POISON))
            at += n
        assert written or not used, f"{what}: no word of the caller's temp was written: the plan ran on its arena"

    def same_bits(self, out, base, what):
        differ = np.flatnonzero(out != base)
        assert differ.size == 0, f"{what}: {differ.size} bytes differ from the plain run, the first at byte {int(differ[0])}"


@pytest.fixture
def harness(fft, dev, oracle, monkeypatch, request):
    case = request.param
    for k, v in case.env.items():
        monkeypatch.setenv("MI355FFT_" + k, v)
    h = Harness(fft, dev, oracle, case)
    yield h
    h.close()


@pytest.mark.parametrize("harness", t.CASES, ids=repr, indirect=True)
def test_exec_contract(harness, oracle):
    h, case = harness, harness.case
    base, _ = h.run(0, 0, 0, 0, temp=False, what=f"{case.name} plain")
    got = base.view(t.out_dtype(case))[:h.want.size]
    t.compare(oracle, case, got, h.want, h.keep, f"{case.name} ({h.route.strip()})")
    t.assert_untouched(base, h.keep, case, case.name)
    for in_pad, out_pad in ((h.pad, h.pad), (0, h.pad)):
        if case.in_place and in_pad != out_pad:
            continue
        what = f"{case.name} input +{in_pad} output +{out_pad} ({h.route.strip()})"
        out, _ = h.run(G, in_pad, out_pad, 8, temp=True, what=what)
        h.same_bits(out, base, what)


@pytest.mark.parametrize("use_graph", [False, True], ids=["ops", "graph"])
@pytest.mark.parametrize("harness", [c for c in t.CASES if c.replay], ids=repr, indirect=True)
def test_replay(harness, use_graph):
    """exec recorded twice in one encoder to two output ranges of one buffer, the list submitted twice: four results, each the plain run's.
    The op list runs on the caller's temp, the graph on the plan's arena (dirty from the plain run)."""
    h, case, fft, dev = harness, harness.case, harness.fft, harness.dev
    base, _ = h.run(0, 0, 0, 0, temp=False, what=f"{case.name} plain")
    room = (h.nbytes + 15) // 16 * 16
    offs = (G + h.pad, G + h.pad + room + G)
    out_host = t.poison_words(3 * G + 2 * room + 16).view(np.uint8)
    in_host = t.banded(h.x, G, h.pad, h.x.nbytes)
    ib, ob = _upload(dev, in_host), _upload(dev, out_host)
    k_host = None if h.kern is None else t.banded(h.kern, G, 8, h.kern.nbytes)
    kb = None if k_host is None else _upload(dev, k_host)
    try:
        enc = dev.createCommandEncoder()
        for off in offs:
            args = {"input": ib, "inputOffsetBytes": G + h.pad, "output": ob, "outputOffsetBytes": off}
            if kb is not None:
                args.update(kernel=kb, kernelOffsetBytes=G + 8)
            if not use_graph and h.temp is not None:
                args["temp"] = h.temp
            h.plan.exec(enc, args)
        if not use_graph and h.temp is not None:
            _poison(dev, h.temp_alloc)
        cb = enc.finish(use_graph=use_graph)
        for submit in (1, 2):
            what = f"{case.name} {'graph' if use_graph else 'op list'}, submit {submit} ({h.route.strip()})"
            dev.queue.submit([cb])
            dev.queue.onSubmittedWorkDone()
            after = _read(fft, ob, out_host.nbytes)
            for n, off in enumerate(offs):
                h.same_bits(after[off:off + h.nbytes], base, f"{what}, exec {n + 1}")
            _assert_poison(after[:offs[0]], what + ": before the first range")
            _assert_poison(after[offs[0] + room:offs[1]], what + ": between the ranges")
            _assert_poison(after[offs[1] + room:], what + ": after the second range")
            assert np.array_equal(_read(fft, ib, in_host.nbytes), in_host), f"{what}: the input buffer was written"
            if kb is not None:
                assert np.array_equal(_read(fft, kb, k_host.nbytes), k_host), f"{what}: the kernel buffer was written"
            if not use_graph and h.temp is not None:
                h.check_temp(what)
            dev.queue.writeBuffer(ob, 0, out_host)      # poison the outputs again
        cb.release()
    finally:
        for b in (ib, ob, kb):
            if b is not None:
                b.destroy()


@pytest.mark.parametrize("harness", [c for c in t.CASES if c.type == "c2c" and not c.in_place], ids=repr, indirect=True)
def test_out_of_place_c2c_on_one_buffer(harness, oracle):
    """output = the input buffer at the same offset: the oracle's result with the guards intact.  No case of the table is refused."""
    h, case = harness, harness.case
    what = f"{case.name} on one buffer ({h.route.strip()})"
    out, in_host = h.run(G, h.pad, h.pad, 8, temp=True, alias=True, what=what)
    t.compare(oracle, case, out.view(t.out_dtype(case))[:h.want.size], h.want, h.keep, what)
    if h.keep.any():      # elements the plan leaves alone hold what the input had there
        bits = np.uint16 if case.f16 else np.uint32
        was = in_host[G + h.pad:G + h.pad + h.nbytes].view(bits)[:h.want.size]
        assert np.array_equal(out.view(bits)[:h.want.size][h.keep], was[h.keep]), f"{what}: elements outside the plan's stores were written"


def test_refusals(fft, dev):
    """kernelOffsetBytes needs a kernel buffer; dense c2c ranges of one buffer that overlap at different offsets have no one-range variant"""
    conv = fft.createPlan(dev, t.BY_NAME["fftconv_fused64"].opts)
    buf = dev.createBuffer({"size": 1 << 20})
    with pytest.raises(fft.Mi355Error, match="kernelOffsetBytes requires kernel to be a buffer"):
        conv.exec(dev.createCommandEncoder(), {"input": buf, "output": buf, "kernel": np.zeros(2 * 64 * 2, np.float32), "kernelOffsetBytes": 8})
    conv.destroy()
    c2c = fft.createPlan(dev, t.BY_NAME["lines64"].opts)
    with pytest.raises(fft.Mi355Error, match="output range overlaps the input range at another offset"):
        c2c.exec(dev.createCommandEncoder(), {"input": buf, "output": buf, "inputOffsetBytes": 0, "outputOffsetBytes": 64})
    c2c.exec(dev.createCommandEncoder(), {"input": buf, "output": buf, "inputOffsetBytes": 0, "outputOffsetBytes": 64 * 37 * 8})   # disjoint ranges: as ever
    c2c.destroy()
    buf.destroy()
