"""GPU tier: precision "f16-storage" through the JavaScript host (js/test/f16_storage.test.mjs over the N-API addon) produces the
same bytes as the Python host for one fused case and one ioView case."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "webgpu-fft_amd", "lib", "mi355fft.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed on this machine")]


def _python_bytes(fft, dev, opts, x16, out_bytes, out_init=None):
    plan = fft.createPlan(dev, dict(opts, precision="f16-storage"))
    inp = dev.createBuffer({"size": x16.nbytes})
    dev.queue.writeBuffer(inp, 0, x16)
    out = dev.createBuffer({"size": out_bytes})
    if out_init is not None:
        dev.queue.writeBuffer(out, 0, out_init)
    enc = dev.createCommandEncoder()
    plan.exec(enc, {"input": inp, "output": out})
    dev.queue.submit([enc.finish()])
    dev.queue.onSubmittedWorkDone()
    got = np.empty(out_bytes, np.uint8)
    fft._chk(fft.lib().mi355fft_buffer_read(out._h, 0, got.ctypes.data, out_bytes))
    plan.destroy()
    inp.destroy()
    out.destroy()
    return got


def test_js_f16_storage_matches_python(tmp_path):
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (run __graft_entry__.build())")
    rng = np.random.default_rng(16)
    fused_in = rng.standard_normal(2 * 1024 * 8).astype(np.float16)
    view_in = rng.standard_normal(2 * 8).astype(np.float16)
    fused_in.tofile(tmp_path / "fused.in.bin")
    view_in.tofile(tmp_path / "ioview.in.bin")
    p = subprocess.run([NODE, os.path.join(ROOT, "webgpu-fft_amd", "js", "test", "f16_storage.test.mjs"), str(tmp_path)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]

    import mi355fft as fft
    dev = fft.Device(0)
    try:
        want = _python_bytes(fft, dev, {"type": "c2c", "shape": [1024], "batch": 8, "direction": "forward", "normalize": "none"}, fused_in, 1024 * 8 * 4)
        assert np.array_equal(np.fromfile(tmp_path / "fused.out.bin", np.uint8), want)
        sentinel = np.tile(np.array([1.5, -2.0], np.float16), 32)
        opts = {"type": "c2c", "shape": [16], "batch": 1, "direction": "forward", "normalize": "none",
                "ioView": {"input": {"shape": [8], "placement": "center"}, "output": {"shape": [32], "placement": "center", "clearOutside": False}}}
        want = _python_bytes(fft, dev, opts, view_in, 32 * 4, sentinel)
        assert np.array_equal(np.fromfile(tmp_path / "ioview.out.bin", np.uint8), want)
    finally:
        dev.close()
