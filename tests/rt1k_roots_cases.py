"""Case table shared by test_emu_rt1k_roots.py and test_gpu_rt1k_roots.py: fft_xcd_rt1k_kernel (kern_regtile.hpp) with its four-step root
tables staged in LDS (MI355_RT1K_ROOTS_LDS).  The kernel exists at N = 2^20 (1024 x 1024, the instances that take the LDS tables) and
at N = 2^21 (2048 x 1024, which keeps the global tables through the same root lambda), so these are the smallest shapes there are."""
N20, N21 = 1 << 20, 1 << 21
TOL = 1e-5  # the suite's bar (test_emu_kernels.py, test_gpu_parity.py): norm-relative, both norms

# direction x normalize: `none` is the scale 1.0 of the unconditional output multiply, `unitary` a scale that is no power of two
DIRECTION_NORMALIZE = [("forward", "none"), ("forward", "unitary"), ("inverse", "none"), ("inverse", "unitary")]

ROUTE_2P20 = "xcd-fused-rt32[N=1024x1024]"
ROUTE_2P21 = "xcd-fused-rt32[N=2048x1024]"

# host emulation: 3 workgroups in ONE group run 3 transforms: tile shares 11 / 11 / 10 per phase, and the group's only slot is re-used twice
EMU_CUS, EMU_SPLIT, EMU_SLOTS, EMU_BATCH = 3, 1, 1, 3

# GPU: one transform (31 of the 32 groups idle), and 69 over 32 groups: five groups run three transforms, the others two (ragged ends),
# and every group re-uses its slot
GPU_BATCHES = (1, 69)
GPU_BATCH_MAX = max(GPU_BATCHES)


def checked_lines(batch):
    """first, last and one middle transform of a batch"""
    return sorted({0, batch // 2, batch - 1})
