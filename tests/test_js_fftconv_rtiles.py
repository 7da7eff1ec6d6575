"""GPU tier: the overlap-save tile route of rank-2 real fftconv through the JavaScript host (js/test/fftconv_rtiles.test.mjs over the N-API
addon): the first case of fftconv_rtiles_cases.py's table (150 x 130 (*) 9 x 5, the switch forcing the 64-point tile) and a request on the
planner's own rule (300 x 200 (*) 9 x 9), each against a float64 direct sum computed in the script, with its route and launch count."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "webgpu-fft_amd", "lib", "mi355fft.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed on this machine")]


def test_js_fftconv_rtiles():
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (run __graft_entry__.build())")
    p = subprocess.run([NODE, os.path.join(ROOT, "webgpu-fft_amd", "js", "test", "fftconv_rtiles.test.mjs")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
