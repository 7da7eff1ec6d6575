"""CPU tier: the circular (WRAP) forms of the real overlap-save tile kernel and of the real overlap-save line kernel under AddressSanitizer + UBSan.

tests/emu/ols_circular_asan_main.cpp is a stand-alone program (its own main, built by tests/emu/ols_circular_asan.mk): it runs the host-emulated
kernels on heap blocks of exactly the plan's extents for real 150 x 130 (*) 9 x 5 and real 8193 (*) 31, circular, as convolution and as
correlation, and compares every output with a direct circular sum in double precision.  A wrapped index outside [0, shape) is a
heap-buffer-overflow report and a non-zero exit status.  Nothing is loaded into python."""
import os
import subprocess

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")


def test_wrap_kernels_stay_inside_exactly_sized_buffers():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "-f", "ols_circular_asan.mk"])
    p = subprocess.run([os.path.join(EMU_DIR, "ols_circular_asan")], cwd=EMU_DIR, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    print(p.stdout)
    print(p.stderr)
    assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if "rel_l2" in ln]
    assert len(lines) == 4 and p.stdout.strip().endswith("ok"), p.stdout
    assert sum("tiles-rconv-ols[N=64x64,L=56x60,wrap]" in ln for ln in lines) == 2 and sum("lines-rconv-ols[N=1024,L=994,wrap]" in ln for ln in lines) == 2, lines
