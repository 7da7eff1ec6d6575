"""CPU tier: the sum over input channels (fftConv.inputChannels) under AddressSanitizer + UBSan.

tests/emu/fftconv_sum_asan_main.cpp is a stand-alone program (its own main, built by tests/emu/fftconv_sum_asan.mk): it runs the host-emulated sum
form of the tile kernel on heap blocks of exactly the plan's extents for complex 150 x 100 (*) 9 x 5 (convolution) and real 150 x 130 (*) 9 x 5
(correlation; the last pair of a row has no partner), batch 2, C = 3, K = 2, and the pointwise multiply-accumulate kernel of the composed routes, and
compares every output with a direct sum over the channels in double precision.  A load from a line beyond batch * C, or a spectrum read beyond
K * C tiles, is a heap-buffer-overflow report and a non-zero exit status.  It also holds the tile launches to the planner's registry (threads, LDS
bytes).  Nothing is loaded into python."""
import os
import subprocess

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


def test_sum_kernels_stay_inside_exactly_sized_buffers():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "-f", "fftconv_sum_asan.mk"])
    p = subprocess.run([os.path.join(EMU_DIR, "fftconv_sum_asan")], cwd=EMU_DIR, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if "rel_l2" in ln]
    assert len(lines) == 3 and p.stdout.strip().endswith("ok"), p.stdout
    assert "tiles-conv-ols-sum[N=64x64,L=56x60,C=3]" in lines[0] and "tiles-rconv-ols-sum[N=64x64,L=56x60,C=3]" in lines[1] and "pointwise-sum" in lines[2], lines
