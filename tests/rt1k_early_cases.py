"""Case table shared by test_emu_rt1k_early.py and test_gpu_rt1k_early.py: fft_xcd_rt1k_kernel (kern_regtile.hpp) with the modifier-form butterflies
(MI355_RT1K_LEAN_BFLY) and phase B's head loads between the arrive and the wait of the A | B barrier (MI355_RT1K_EARLY_B, counter bar[gslot][2] of
kern_xcd.hpp; off in the shipped build, on in the emulation that test_emu_rt1k_early.py builds).  The kernel exists only at N = 2^20 (1024 x 1024: 32 tiles of 32 lines per phase), so that is the smallest shape there is."""
N20 = 1 << 20
TOL = 1e-5  # the suite's bar (test_emu_kernels.py, test_gpu_parity.py): norm-relative, both norms

DIRECTION_NORMALIZE = [("forward", "none"), ("forward", "unitary"), ("inverse", "none"), ("inverse", "unitary")]

ROUTE_2P20 = "xcd-fused-rt32[N=1024x1024]"

NT, HEAD = 32, 16  # tiles per phase; row loads of the head (MI355_RT1K_PREFETCH_B / 2), which read what phase-A tiles 0 .. 15 stored


def early_enabled(gsize):
    """the kernel's per-launch condition: every workgroup owns NT / gsize tiles and tiles 0 .. HEAD - 1 lie in rounds before the last"""
    return NT % gsize == 0 and (NT // gsize - 1) * gsize >= HEAD


# host emulation, (workgroups in the one group, slots, transforms):
#   4: 8 tiles per workgroup, the condition holds, and the group's only slot is re-used twice
#   3: tile shares 11 / 11 / 10, 32 % 3 != 0: the path must stay off and the counter untouched
EMU_CONFIGS = [(4, 1, 3), (3, 1, 3)]
assert early_enabled(4) and not early_enabled(3)

# GPU, default grouping (8 workgroups per group, four rounds): one transform (31 of the 32 groups idle), and 69 over 32 groups: five groups run
# three transforms, the others two, and every group re-uses its slot
GPU_BATCHES = (1, 69)
GPU_BATCH_MAX = max(GPU_BATCHES)
# MI355FFT_XCD_SPLIT (groups per XCD; plan.cpp: 1, 2, 4, 8, 16 or 32; 32 workgroups per XCD on a 256-CU device) -> workgroups per group
#   2 -> 16: two rounds, the condition's edge (R - 1) * gsize == HEAD
#   16 -> 2: sixteen rounds
#   1 -> 32: one round, the condition is false
SPLIT_GSIZE = [(2, 16), (16, 2), (1, 32)]
assert early_enabled(16) and early_enabled(2) and not early_enabled(32) and early_enabled(8)


def checked_lines(batch):
    """first, last and one middle transform of a batch"""
    return sorted({0, batch // 2, batch - 1})
