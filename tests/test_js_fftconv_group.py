"""GPU tier: fftConv.groups through the JavaScript host (js/test/fftconv_group.test.mjs over the N-API addon): the first request of
fftconv_group_cases.py's grouped tile table (150 x 100 (*) 9 x 5, C = 4, K = 4, G = 2, the switch forcing the grouped kernel) and its rank-1 composed
request (1000 (*) 31, C = 4, K = 2, G = 2, the kernels as a list of K Cg arrays), each against a float64 direct sum computed in the script, with route
and launch count; the length errors that name the count as kernelCount=K x inputChannels/groups=Cg; the host's validation of the option."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "webgpu-fft_amd", "lib", "mi355fft.node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node is not installed on this machine")]


def test_js_fftconv_group():
    if not os.path.exists(ADDON):
        pytest.skip("N-API addon not built (run __graft_entry__.build())")
    p = subprocess.run([NODE, os.path.join(ROOT, "webgpu-fft_amd", "js", "test", "fftconv_group.test.mjs")], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
