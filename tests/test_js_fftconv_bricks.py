"""GPU tier: the overlap-save brick routes of rank-3 fftconv through the JavaScript host (js/test/fftconv_bricks.test.mjs over the N-API
addon): 30 x 20 x 18 (*) 5 x 3 x 4 with the switch forcing the brick (the shape of the first cases of fftconv_bricks_cases.py's table, as
linear-same convolution), complex and real, and 40 x 36 x 34 (*) 3 x 3 x 3 on the planner's own rule, each against a float64 direct sum
computed in the script, with its route and launch count."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "webgpu-fft_amd", "lib", "mi355fft.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed on this machine")]


def test_js_fftconv_bricks():
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (run __graft_entry__.build())")
    p = subprocess.run([NODE, os.path.join(ROOT, "webgpu-fft_amd", "js", "test", "fftconv_bricks.test.mjs")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
