"""GPU tier: boundary "circular" on the overlap-save routes of fftconv through the JavaScript host (js/test/fftconv_circular.test.mjs over the
N-API addon): one complex request (150 x 130 (*) 9 x 5, tiles) and one real request (an odd line of 8193 points (*) 31, K = 2) on the planner's
default rule, each against a float64 direct circular sum computed in the script, with its route, launch count and workspace, and without the
route's tag under MI355FFT_OLS_CIRCULAR=0."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "webgpu-fft_amd", "lib", "mi355fft.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed on this machine")]


def test_js_fftconv_circular():
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (run __graft_entry__.build())")
    p = subprocess.run([NODE, os.path.join(ROOT, "webgpu-fft_amd", "js", "test", "fftconv_circular.test.mjs")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
