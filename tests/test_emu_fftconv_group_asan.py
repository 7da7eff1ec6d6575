"""CPU tier: grouped and depthwise convolution (fftConv.groups) under AddressSanitizer + UBSan.

tests/emu/fftconv_group_asan_main.cpp is a stand-alone program (its own main, built by tests/emu/fftconv_group_asan.mk): it runs both host-emulated forms
of the grouped tile kernel on heap blocks of exactly the plan's extents, the sum form on complex 150 x 100 (*) 9 x 5 (convolution, C = 4, K = 4, G = 2) and
the depthwise form on real 150 x 130 (*) 9 x 5 (correlation, C = K = G = 3; the last pair of a row has no partner), batch 2, and the grouped pointwise
multiply-accumulate kernel of the composed routes on the last group of its data, and compares every output with a direct sum over the group's channels in
double precision.  A load from a line beyond batch * C, a spectrum read beyond K * Cg tiles or a store beyond the last output lane is a
heap-buffer-overflow report and a non-zero exit status.  It also holds the launches' threads and LDS bytes to the planner's registry, the step slots to
the request's counts, and the two lists of grouped instances (length, ids, threads, LDS bytes, no 128-point entry) to the registry.  Nothing is loaded into python."""
import os
import subprocess

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


def test_grouped_kernels_stay_inside_exactly_sized_buffers():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "-f", "fftconv_group_asan.mk"])
    p = subprocess.run([os.path.join(EMU_DIR, "fftconv_group_asan")], cwd=EMU_DIR, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if "rel_l2" in ln]
    assert len(lines) == 3 and p.stdout.strip().endswith("ok"), p.stdout
    assert "tiles-conv-ols-group[N=64x64,L=56x60,C=4,G=2,K=4]" in lines[0] and "tiles-rconv-ols-group[N=64x64,L=56x60,C=3,G=3,K=3]" in lines[1], lines
    assert "pointwise-group-sum" in lines[2], lines
    assert "registry: 2 grouped entries per data type, 256 threads, 33728 B of LDS" in p.stdout, p.stdout
