// dispatch.hpp — turns one planned Step (plan.hpp) with resolved pointers into a kernel launch.
//
// Shared by the product launcher (api.hip: HipLauncher enqueues on the device stream or a capturing
// stream — the "hipGraph stage executor" that replaces the per-stage beginComputePass/dispatchWorkgroups
// loop of src/plan.js:1233-1273) and by the host emulation in tests/emu (EmuLauncher).
//
// A Launcher provides:
//   template <class... P, class... A> void launch(void (*kernel)(P...), unsigned grid, unsigned block, unsigned smem, A&&... args);
//   void copy(void* dst, const void* src, size_t bytes);
#pragma once
#include <utility>
#include "kern_f16.hpp"
#include "kern_fftconv.hpp"
#include "kern_generic.hpp"
#include "kern_lines.hpp"
#include "kern_mixed.hpp"
#include "kern_mixed_ct.hpp"
#include "kern_line_reg.hpp"
#include "kern_line32k.hpp"
#include "kern_trig.hpp"
#include "kern_xcd_real.hpp"
#include "kern_regtile.hpp"
#include "kern_xcd_res.hpp"
#include "kern_tiles.hpp"
#include "kern_bricks.hpp"
#include "plan.hpp"

namespace mi355 {

// line-kernel families: one translation unit each so the device code builds in parallel
enum : int { FAM_ROW_SMALL = 0, FAM_ROW_1K = 1, FAM_ROW_BIG = 2, FAM_PASS_A = 3, FAM_PASS_B = 4, FAM_COUNT = 5 };
constexpr int row_family(int N) { return N <= 256 ? FAM_ROW_SMALL : (N <= 1024 ? FAM_ROW_1K : FAM_ROW_BIG); }

// real fftconv line kernel (kern_lines.hpp fft_lines_rconv_kernel) on a forward ROW configuration.  Its instances are built in a
// translation unit of their own (lines_rconv.hip) in the product build: kernels compiled together change each other's register
// allocation, and the family units' device code stays what it was
template <class C, class L> bool launch_lines_rconv(const LineArgs& a, unsigned grid, L& l);
#if defined(MI355_RCONV_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class C, class L> bool launch_lines_rconv(const LineArgs& a, unsigned grid, L& l) {
  if constexpr (!C::IN_COL && !C::OUT_COL && !C::SWAP_IN && !C::SWAP_OUT && C::TWID == TWID_NONE && C::NSTAGES >= 2) {
    l.launch(fft_lines_rconv_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);
    return true;
  } else return false;
}
#endif
// its overlap-save form (fft_lines_rconv_ols_kernel, route lines-rconv-ols): block lengths P = 128 .. 8192 on the same configurations (no scratch
// up to there), in the same unit.  `id`: the registry id of the forward ROW configuration of P / 2 points
template <class L> bool launch_lines_rconv_ols(int id, const RconvOlsArgs& a, unsigned grid, L& l);
#if defined(MI355_RCONV_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_lines_rconv_ols(int id, const RconvOlsArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define LINE_ROW(N, R0, R1, R2, T)                                                                          \
  if (id == cur) {                                                                                          \
    using C = LineCfg<N, R0, R1, R2, T, false, false, false, false, 0>;                                     \
    if constexpr (C::NSTAGES >= 2 && (N) <= 4096) {                                                         \
      l.launch(fft_lines_rconv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);       \
      return true;                                                                                          \
    } else return false;                                                                                    \
  }                                                                                                         \
  cur += 2;
#define LINE_ROW_TRIG(N, R0, R1, R2, T) cur += 1;
#define LINE_PASS_A(N, R0, R1, R2, T) cur += 3;
#define LINE_PASS_B(N, R0, R1, R2, T) cur += 2;
#define LINE_COL_RAGGED(N, R0, R1, R2, T) cur += 2;
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

// its circular form (the kernel on OlsWrap<C>, route lines-rconv-ols[..,wrap]): the block lengths the route's rule names, P = 1024, 2048 and 8192 (half lengths
// 512, 1024 and 4096), in a unit of their own (lines_rconv_ols_wrap.hip)
template <class L> bool launch_lines_rconv_ols_wrap(int id, const RconvOlsArgs& a, unsigned grid, L& l);
#if defined(MI355_RCONV_OLS_WRAP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_lines_rconv_ols_wrap(int id, const RconvOlsArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define LINE_ROW(N, R0, R1, R2, T)                                                                          \
  if (id == cur) {                                                                                          \
    using C = OlsWrap<LineCfg<N, R0, R1, R2, T, false, false, false, false, 0>>;                            \
    if constexpr ((N) == 512 || (N) == 1024 || (N) == 4096) {                                               \
      l.launch(fft_lines_rconv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);       \
      return true;                                                                                          \
    } else return false;                                                                                    \
  }                                                                                                         \
  cur += 2;
#define LINE_ROW_TRIG(N, R0, R1, R2, T) cur += 1;
#define LINE_PASS_A(N, R0, R1, R2, T) cur += 3;
#define LINE_PASS_B(N, R0, R1, R2, T) cur += 2;
#define LINE_COL_RAGGED(N, R0, R1, R2, T) cur += 2;
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

// complex overlap-save (kern_lines.hpp fft_lines_conv_ols_kernel, route lines-conv-ols): block lengths P = 128 .. 4096, in a unit of their own
// (lines_conv_ols.hip).  `id`: the registry id of the forward ROW configuration of P points
template <class L> bool launch_lines_conv_ols(int id, const RconvOlsArgs& a, unsigned grid, L& l);
#if defined(MI355_CONV_OLS_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_lines_conv_ols(int id, const RconvOlsArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define LINE_ROW(N, R0, R1, R2, T)                                                                          \
  if (id == cur) {                                                                                          \
    using C = LineCfg<N, R0, R1, R2, T, false, false, false, false, 0>;                                     \
    if constexpr (C::NSTAGES >= 2 && (N) >= 128 && (N) <= 4096) {                                           \
      l.launch(fft_lines_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);        \
      return true;                                                                                          \
    } else return false;                                                                                    \
  }                                                                                                         \
  cur += 2;
#define LINE_ROW_TRIG(N, R0, R1, R2, T) cur += 1;
#define LINE_PASS_A(N, R0, R1, R2, T) cur += 3;
#define LINE_PASS_B(N, R0, R1, R2, T) cur += 2;
#define LINE_COL_RAGGED(N, R0, R1, R2, T) cur += 2;
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

// its circular form (the kernel on OlsWrap<C>, route lines-conv-ols[..,wrap]): the block lengths plan.cpp conv_ols_block names, 2048 and 4096, in a unit of
// their own again (lines_conv_ols_wrap.hip)
template <class L> bool launch_lines_conv_ols_wrap(int id, const RconvOlsArgs& a, unsigned grid, L& l);
#if defined(MI355_CONV_OLS_WRAP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_lines_conv_ols_wrap(int id, const RconvOlsArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define LINE_ROW(N, R0, R1, R2, T)                                                                          \
  if (id == cur) {                                                                                          \
    using C = OlsWrap<LineCfg<N, R0, R1, R2, T, false, false, false, false, 0>>;                            \
    if constexpr ((N) == 2048 || (N) == 4096) {                                                             \
      l.launch(fft_lines_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);        \
      return true;                                                                                          \
    } else return false;                                                                                    \
  }                                                                                                         \
  cur += 2;
#define LINE_ROW_TRIG(N, R0, R1, R2, T) cur += 1;
#define LINE_PASS_A(N, R0, R1, R2, T) cur += 3;
#define LINE_PASS_B(N, R0, R1, R2, T) cur += 2;
#define LINE_COL_RAGGED(N, R0, R1, R2, T) cur += 2;
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

// overlap-save on rank-2 complex tiles (kern_tiles.hpp fft_tiles_conv_ols_kernel, routes tiles-spectrum / tiles-conv-ols): the instances of
// MI355_TILE_KERNEL_LIST, in a unit of their own (tiles_conv_ols.hip).  `id`: position in that list (plan.cpp find_tile_kernel)
template <class L> bool launch_tiles_conv_ols(int id, const TilesArgs& a, unsigned grid, L& l);
// the real form (fft_tiles_conv_ols_kernel on RTileCfg, routes tiles-rspectrum / tiles-rconv-ols): the same list, in a unit of its own (tiles_rconv_ols.hip)
template <class L> bool launch_tiles_rconv_ols(int id, const TilesArgs& a, unsigned grid, L& l);
// its argument block from an ST_LINES step of mode LM_TILES_CONV_OLS / LM_TILES_SPECTRUM (and their real forms): every geometry slot holds axis 0 in its low 32 bits and axis 1 in its high
inline TilesArgs tiles_args_of(const Step& s, void* const ptr[STEP_PTRS]) {
  TilesArgs ta{};
  ta.in = (const cf*)ptr[LP_IN]; ta.out = (cf*)ptr[LP_OUT]; ta.tw = (const cf*)ptr[LP_TW]; ta.spectrum = (const cf*)ptr[LP_MUL_SPECTRUM];
  ta.num_tiles = s.i[LS_TILES]; ta.scale = s.f[F_SCALE];
  ta.conj = (int)s.i[LS_CONJ]; ta.spectrum_only = s.i[LS_MODE] == LM_TILES_SPECTRUM || s.i[LS_MODE] == LM_TILES_RSPECTRUM;
  for (int x = 0; x < 2; ++x) {
    const OlsAxis g = ols_axis_of(s.i, x);
    ta.ax[x] = TileAxis{(int)g.fN, (int)g.plim, (int)g.nb, (int)g.L, (int)g.w0, (int)g.pre};
  }
  ta.imap = s.imap; ta.omap = s.omap;
  return ta;
}
#if defined(MI355_TILES_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_tiles_conv_ols(int id, const TilesArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define X(P, R0, R1, TH)                                                                              \
  if (id == cur) {                                                                                    \
    using C = TileCfg<P, R0, R1, TH>;                                                                 \
    l.launch(fft_tiles_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);    \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
  MI355_TILE_KERNEL_LIST(X)
#undef X
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

#if defined(MI355_RTILES_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_tiles_rconv_ols(int id, const TilesArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define X(P, R0, R1, TH)                                                                              \
  if (id == cur) {                                                                                    \
    using C = RTileCfg<P, R0, R1, TH>;                                                                \
    l.launch(fft_tiles_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);    \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
  MI355_TILE_KERNEL_LIST(X)
#undef X
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

// the circular forms of both (the kernel on WTileCfg / WRTileCfg, routes tiles-conv-ols[..,wrap] / tiles-rconv-ols[..,wrap]; the spectrum launches stay on
// the linear instances): the same list, each form in a unit of its own (tiles_conv_ols_wrap.hip, tiles_rconv_ols_wrap.hip)
template <class L> bool launch_tiles_conv_ols_wrap(int id, const TilesArgs& a, unsigned grid, L& l);
template <class L> bool launch_tiles_rconv_ols_wrap(int id, const TilesArgs& a, unsigned grid, L& l);
#define MI355_TILE_WRAP_LAUNCHER(NAME, CFG)                                                           \
  template <class L> bool NAME(int id, const TilesArgs& a, unsigned grid, L& l) {                     \
    int cur = 0;                                                                                      \
    MI355_TILE_KERNEL_LIST(X)                                                                         \
    (void)cur; (void)a; (void)grid; (void)l;                                                          \
    return false;                                                                                     \
  }
#if defined(MI355_TILES_WRAP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, R0, R1, TH)                                                                              \
  if (id == cur) {                                                                                    \
    using C = WTileCfg<P, R0, R1, TH>;                                                                \
    l.launch(fft_tiles_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);    \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_TILE_WRAP_LAUNCHER(launch_tiles_conv_ols_wrap, WTileCfg)
#undef X
#endif
#if defined(MI355_RTILES_WRAP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, R0, R1, TH)                                                                              \
  if (id == cur) {                                                                                    \
    using C = WRTileCfg<P, R0, R1, TH>;                                                               \
    l.launch(fft_tiles_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);    \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_TILE_WRAP_LAUNCHER(launch_tiles_rconv_ols_wrap, WRTileCfg)
#undef X
#endif
#undef MI355_TILE_WRAP_LAUNCHER

// the sum forms (fftConv.inputChannels > 1: fft_tiles_conv_ols_sum_kernel on STileCfg / SRTileCfg, routes tiles-conv-ols-sum / tiles-rconv-ols-sum; the spectrum launches stay on
// the single-channel instances): the instances of MI355_TILE_SUM_KERNEL_LIST, each form in a unit of its own (tiles_conv_ols_sum.hip, tiles_rconv_ols_sum.hip).
// `id`: position in that list (plan.cpp find_tile_kernel with `sum`)
template <class L> bool launch_tiles_conv_ols_sum(int id, const TilesSumArgs& a, unsigned grid, L& l);
template <class L> bool launch_tiles_rconv_ols_sum(int id, const TilesSumArgs& a, unsigned grid, L& l);
inline TilesSumArgs tiles_sum_args_of(const Step& s, void* const ptr[STEP_PTRS]) { return TilesSumArgs{tiles_args_of(s, ptr), (int)s.i[LS_TILES_CHANNELS]}; }
#define MI355_TILE_SUM_LAUNCHER(NAME)                                                                 \
  template <class L> bool NAME(int id, const TilesSumArgs& a, unsigned grid, L& l) {                  \
    int cur = 0;                                                                                      \
    MI355_TILE_SUM_KERNEL_LIST(X)                                                                     \
    (void)cur; (void)a; (void)grid; (void)l;                                                          \
    return false;                                                                                     \
  }
#if defined(MI355_TILES_SUM_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, R0, R1, TH)                                                                              \
  if (id == cur) {                                                                                    \
    using C = STileCfg<P, R0, R1, TH>;                                                                \
    l.launch(fft_tiles_conv_ols_sum_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_TILE_SUM_LAUNCHER(launch_tiles_conv_ols_sum)
#undef X
#endif
#if defined(MI355_RTILES_SUM_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, R0, R1, TH)                                                                              \
  if (id == cur) {                                                                                    \
    using C = SRTileCfg<P, R0, R1, TH>;                                                               \
    l.launch(fft_tiles_conv_ols_sum_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_TILE_SUM_LAUNCHER(launch_tiles_rconv_ols_sum)
#undef X
#endif
#undef MI355_TILE_SUM_LAUNCHER

// the grouped forms (fftConv.groups > 1: fft_tiles_conv_ols_group_kernel, routes tiles-conv-ols-group / tiles-rconv-ols-group, every output kernel in one launch; the spectrum
// launches stay on the single-channel instances): the instances of MI355_TILE_GROUP_KERNEL_LIST, each data type in a unit of its own (tiles_conv_ols_group.hip,
// tiles_rconv_ols_group.hip).  `id`: position in that list (plan.cpp find_tile_kernel with `group`)
template <class L> bool launch_tiles_conv_ols_group(int id, const TilesGroupArgs& a, unsigned grid, L& l);
template <class L> bool launch_tiles_rconv_ols_group(int id, const TilesGroupArgs& a, unsigned grid, L& l);
inline TilesGroupArgs tiles_group_args_of(const Step& s, void* const ptr[STEP_PTRS]) {
  const auto lo = [](int64_t v) { return (int)(v & 0xffffffff); };
  const auto hi = [](int64_t v) { return (int)(v >> 32); };
  return TilesGroupArgs{tiles_args_of(s, ptr), lo(s.i[LS_TILES_CHANNELS]), hi(s.i[LS_TILES_CHANNELS]), lo(s.i[LS_TILES_KERNELS]), hi(s.i[LS_TILES_KERNELS]), (long long)s.i[LS_TILES_LANE_K]};
}
#define MI355_TILE_GROUP_LAUNCHER(NAME)                                                               \
  template <class L> bool NAME(int id, const TilesGroupArgs& a, unsigned grid, L& l) {                \
    int cur = 0;                                                                                      \
    MI355_TILE_GROUP_KERNEL_LIST(X)                                                                   \
    (void)cur; (void)a; (void)grid; (void)l;                                                          \
    return false;                                                                                     \
  }
#if defined(MI355_TILES_GROUP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, R0, R1, TH, DW)                                                                          \
  if (id == cur) {                                                                                    \
    using C = GroupTileCfg<P, R0, R1, TH, DW, false>;                                                 \
    l.launch(fft_tiles_conv_ols_group_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_TILE_GROUP_LAUNCHER(launch_tiles_conv_ols_group)
#undef X
#endif
#if defined(MI355_RTILES_GROUP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, R0, R1, TH, DW)                                                                          \
  if (id == cur) {                                                                                    \
    using C = GroupTileCfg<P, R0, R1, TH, DW, true>;                                                  \
    l.launch(fft_tiles_conv_ols_group_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_TILE_GROUP_LAUNCHER(launch_tiles_rconv_ols_group)
#undef X
#endif
#undef MI355_TILE_GROUP_LAUNCHER

// overlap-save on rank-3 bricks (kern_bricks.hpp fft_bricks_conv_ols_kernel, routes bricks-spectrum / bricks-conv-ols and, on an RBrickCfg, bricks-rspectrum /
// bricks-rconv-ols): the instances of MI355_BRICK_KERNEL_LIST, each form in a unit of its own (bricks_conv_ols.hip, bricks_rconv_ols.hip).  `id`: position in
// that list (plan.cpp find_brick_kernel)
template <class L> bool launch_bricks_conv_ols(int id, const BricksArgs& a, unsigned grid, L& l);
template <class L> bool launch_bricks_rconv_ols(int id, const BricksArgs& a, unsigned grid, L& l);
// its argument block from an ST_LINES step of the four brick modes: axes 0 and 1 in the halves of the LS_OLS slots, axis 2 in the LS_OLS2 slots (ols_axis_of)
inline BricksArgs bricks_args_of(const Step& s, void* const ptr[STEP_PTRS]) {
  BricksArgs ba{};
  ba.in = (const cf*)ptr[LP_IN]; ba.out = (cf*)ptr[LP_OUT]; ba.spectrum = (const cf*)ptr[LP_MUL_SPECTRUM];
  ba.num_items = s.i[LS_TILES]; ba.scale = s.f[F_SCALE];
  ba.conj = (int)s.i[LS_CONJ]; ba.spectrum_only = s.i[LS_MODE] == LM_BRICKS_SPECTRUM || s.i[LS_MODE] == LM_BRICKS_RSPECTRUM;
  for (int x = 0; x < 3; ++x) {
    const OlsAxis g = ols_axis_of(s.i, x);
    ba.ax[x] = TileAxis{(int)g.fN, (int)g.plim, (int)g.nb, (int)g.L, (int)g.w0, (int)g.pre};
  }
  ba.imap = s.imap; ba.omap = s.omap;
  return ba;
}
#if defined(MI355_BRICKS_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_bricks_conv_ols(int id, const BricksArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define X(P, TH)                                                                                      \
  if (id == cur) {                                                                                    \
    using C = BrickCfg<P, TH>;                                                                        \
    l.launch(fft_bricks_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);   \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
  MI355_BRICK_KERNEL_LIST(X)
#undef X
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

#if defined(MI355_RBRICKS_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_bricks_rconv_ols(int id, const BricksArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define X(P, TH)                                                                                      \
  if (id == cur) {                                                                                    \
    using C = RBrickCfg<P, TH>;                                                                       \
    l.launch(fft_bricks_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);   \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
  MI355_BRICK_KERNEL_LIST(X)
#undef X
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}
#endif

template <int FAMILY, class L>
bool launch_lines_family(int id, const LineArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define MI_LINE_CASE(FAM, N, R0, R1, R2, T, IC, OC, SI, SO, TW)                          \
  if (id == cur) {                                                                       \
    if constexpr ((FAM) == FAMILY) {                                                     \
      using C = LineCfg<N, R0, R1, R2, T, IC, OC, SI, SO, TW>;                           \
      if constexpr ((TW) == 4) {   /* ROW_ALT_TRIG: only the one-launch DCT / DST kernels exist for these shapes */ \
        if constexpr (!(SI)) {                                                           \
          if (a.real_mode == LM_DCT2 || a.real_mode == LM_DST2) { l.launch(fft_lines_r2c_kernel<C, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); return true; } \
        } else {                                                                         \
          if (a.real_mode == LM_DCT3 || a.real_mode == LM_DST3) { l.launch(fft_lines_c2r_kernel<C, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); return true; } \
        }                                                                                \
        return false;                                                                    \
      } else {                                                                           \
      if constexpr (!(IC) && !(OC) && !(SI) && !(SO) && (TW) == 0 && C::NSTAGES >= 2) {   \
        if (a.real_mode == LM_R2C) {                                                     \
          if (a.mapped) l.launch(fft_lines_r2c_kernel<C, false, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          else if (a.h16) l.launch(fft_lines_r2c_kernel<C, false, false, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          else l.launch(fft_lines_r2c_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          return true;                                                                   \
        }                                                                                \
        if (a.real_mode == LM_DCT2 || a.real_mode == LM_DST2) {                          \
          l.launch(fft_lines_r2c_kernel<C, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          return true;                                                                   \
        }                                                                                \
        if (a.real_mode == LM_RCONV) return launch_lines_rconv<C>(a, grid, l);            \
        if (a.real_mode == LM_MUL) {                                                     \
          if (a.mapped) l.launch(fft_lines_mul_kernel<C, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          else l.launch(fft_lines_mul_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          return true;                                                                   \
        }                                                                                \
      }                                                                                  \
      if constexpr (!(IC) && !(OC) && (SI) && (SO) && (TW) == 0) {                        \
        if (a.real_mode == LM_C2R && !a.mapped) {                                        \
          if (a.h16) l.launch(fft_lines_c2r_kernel<C, false, false, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          else l.launch(fft_lines_c2r_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          return true;                                                                   \
        }                                                                                \
        if constexpr (C::NSTAGES >= 2) {                                                 \
          if (a.real_mode == LM_C2R) {                                                   \
            l.launch(fft_lines_c2r_kernel<C, false, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
            return true;                                                                 \
          }                                                                              \
          if (a.real_mode == LM_DCT3 || a.real_mode == LM_DST3) {                        \
            l.launch(fft_lines_c2r_kernel<C, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
            return true;                                                                 \
          }                                                                              \
        }                                                                                \
      }                                                                                  \
      if (a.real_mode != LM_C2C) return false;                                           \
      if constexpr ((IC) == (OC) && (TW) == 0) {                                         \
        if (a.mapped) {                                                                  \
          l.launch(fft_lines_mapped_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          return true;                                                                   \
        }                                                                                \
      }                                                                                  \
      if (a.mapped) return false;                                                        \
      if (a.h16) {   /* f16-storage: the dense ROW instances only (plan.cpp wrap_f16_storage) */ \
        if constexpr (!(IC) && !(OC) && (SI) == (SO) && (TW) == 0) {                     \
          l.launch(fft_lines_kernel<C, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
          return true;                                                                   \
        }                                                                                \
        return false;                                                                    \
      }                                                                                  \
      l.launch(fft_lines_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a); \
      return true;                                                                       \
      }                                                                                  \
    } else return false;                                                                 \
  }                                                                                      \
  ++cur;
#define LINE_ROW(N, R0, R1, R2, T)                                          \
  MI_LINE_CASE(row_family(N), N, R0, R1, R2, T, false, false, false, false, 0) \
  MI_LINE_CASE(row_family(N), N, R0, R1, R2, T, false, false, true, true, 0)
#define LINE_ROW_TRIG(N, R0, R1, R2, T) \
  MI_LINE_CASE(row_family(N), N, R0, R1, R2, T, false, false, false, false, 4)
#define LINE_PASS_A(N, R0, R1, R2, T)                               \
  MI_LINE_CASE(FAM_PASS_A, N, R0, R1, R2, T, true, true, false, false, 0) \
  MI_LINE_CASE(FAM_PASS_A, N, R0, R1, R2, T, true, true, true, false, 0)  \
  MI_LINE_CASE(FAM_PASS_A, N, R0, R1, R2, T, true, true, true, true, 0)
#define LINE_PASS_B(N, R0, R1, R2, T)                                \
  MI_LINE_CASE(FAM_PASS_B, N, R0, R1, R2, T, false, true, false, false, 2) \
  MI_LINE_CASE(FAM_PASS_B, N, R0, R1, R2, T, false, true, false, true, 2)
#define LINE_COL_RAGGED(N, R0, R1, R2, T)                             \
  MI_LINE_CASE(FAM_PASS_A, N, R0, R1, R2, T, true, true, false, false, 3) \
  MI_LINE_CASE(FAM_PASS_A, N, R0, R1, R2, T, true, true, true, true, 3)
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
#undef MI_LINE_CASE
  (void)cur; (void)a; (void)grid; (void)l;
  return false;
}

inline int family_of_line_kernel(const LineKernelMeta& m) {
  if (m.in_col && m.out_col) return FAM_PASS_A;
  if (!m.in_col && m.out_col) return FAM_PASS_B;
  return row_family(m.N);
}

template <class L> bool launch_fftconv_fused(int id, const FusedConvArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define X(N, R0, R1, TL)                                                                               \
  if (id == cur++) {                                                                                   \
    using C = ConvCfg<N, R0, R1, TL>;                                                                  \
    l.launch(fftconv_fused_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);        \
    return true;                                                                                       \
  }
  MI355_CONV_KERNEL_LIST(X)
#undef X
  (void)cur;
  return false;
}

// XCD-fused kernels: instance ONLY of xcd_kernels.def (plan.hpp XCD_INSTANCES), one case per kind.
// In the product build EVERY instance is compiled in its own translation unit (lines_xcd_one.hip with -DMI355_XCD_ID=k):
// these kernels sit at the edge of the 256-VGPR budget and the register allocation of one and the same kernel changed with
// the other kernels of its translation unit (e.g. 1024x2048 c2c: 247 VGPRs and no scratch alone, 256 VGPRs and 92 B of scratch
// per lane in a unit with eleven siblings; r2c 1024x2048: 88 B against 264 B).
template <int ONLY, class L> bool launch_xcd_sel(int id, const XcdFusedArgs& a, unsigned grid, L& l);

#if defined(MI355_XCD_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <int ONLY, class L> bool launch_xcd_sel(int id, const XcdFusedArgs& a, unsigned grid, L& l) {
  constexpr XcdInstance k = XCD_INSTANCES[ONLY];
  if (id != ONLY) return false;
  if constexpr (k.kind <= XK_VIEW) {   // LDS-resident passes; 2-D: pass B is a ROW kernel, natural order out
    using CA = LineCfg<k.N1, k.ra[0], k.ra[1], k.ra[2], k.ta, true, true, k.inverse, false, 0>;
    using CB = LineCfg<k.N2, k.rb[0], k.rb[1], k.rb[2], k.tb, false, k.kind != XK_TWO_D, false, k.inverse, 0>;
    using F = XcdFusedCfg<CA, CB>;
    if constexpr (k.kind == XK_R2C) l.launch_concurrent(fft_xcd_r2c_kernel<CA, CB>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
    else if constexpr (k.kind == XK_C2R) l.launch_concurrent(fft_xcd_c2r_kernel<CA, CB>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
    else l.launch_concurrent(fft_xcd_fused_kernel<CA, CB, k.kind == XK_VIEW>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
  } else if constexpr (k.kind == XK_RT) {
    using F = XcdRtCfg<k.N1, k.inverse>;
    l.launch_concurrent(fft_xcd_rt_kernel<k.N1, k.inverse>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
  } else if constexpr (k.kind == XK_RT_R2C || k.kind == XK_RT_C2R) {
    using F = XcdRtR2cCfgN<k.N1>;
    if constexpr (k.kind == XK_RT_R2C) l.launch_concurrent(fft_xcd_rt_r2c_kernel<k.N1>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
    else l.launch_concurrent(fft_xcd_rt_c2r_kernel<k.N1>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
  } else if constexpr (k.kind == XK_HX) {
    l.launch_concurrent(fft_xcd_hx_kernel<k.inverse>, grid, (unsigned)HxCfg::THREADS, (unsigned)HxCfg::LDS_BYTES, a);
  } else if constexpr (k.kind == XK_CONV) {
    using F = Rt1kCfgT<k.tb>;
    l.launch_concurrent(fft_xcd_conv1m_kernel<k.N1>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
  } else if constexpr (k.kind == XK_CONV_VIEW) {
    using F = Rt1kCfgT<k.tb>;
    l.launch_concurrent(fft_xcd_conv1m_kernel<k.N1, true>, grid, (unsigned)F::THREADS, (unsigned)F::LDS_BYTES, a);
  } else {   // XK_RT1K, XK_RT1K_16, XK_RT1K_VIEW, XK_RT1K_2048: Tb-line register tiles along the 1024-point rows
    using F = Rt1kCfgT<k.tb>;
    constexpr unsigned smem = F::LDS_BYTES + (k.N1 == 2048 ? RtCfg::TW2_ELEMS * 8 : 0) + rt1k_root_lds_elems(k.tb, k.kind == XK_RT1K_VIEW, k.N1) * 8;   // (2048-point columns: their stage-2 roots too; MI355_RT1K_ROOTS_LDS: the four-step tables)
    l.launch_concurrent(fft_xcd_rt1k_kernel<k.inverse, k.tb, k.kind == XK_RT1K_VIEW, k.N1>, grid, (unsigned)F::THREADS, smem, a);
  }
  return true;
}
#endif

template <class L, int... Is>
bool launch_xcd_fold(int id, const XcdFusedArgs& a, unsigned grid, L& l, std::integer_sequence<int, Is...>) {
  return ((id == Is && launch_xcd_sel<Is, L>(id, a, grid, l)) || ...);
}
template <class L> bool launch_xcd_fused(int id, const XcdFusedArgs& a, unsigned grid, L& l) {
  return launch_xcd_fold(id, a, grid, l, std::make_integer_sequence<int, XCD_INSTANCE_COUNT>{});
}

// XCD-resident kernel (kern_xcd_res.hpp): variant bit 0 = inverse, bit 1 = data-movement skeleton.  Own translation unit
// (xcd_res_kernel.hip) in the product build, like the fused instances.
template <class L> bool launch_xcd_res(int variant, const XcdFusedArgs& a, unsigned grid, L& l);
#if defined(MI355_XCD_RES_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_xcd_res(int variant, const XcdFusedArgs& a, unsigned grid, L& l) {
  constexpr unsigned T = (unsigned)XcdResCfg::THREADS, S = (unsigned)XcdResCfg::LDS_BYTES;
  switch (variant) {
    case 0: l.launch_concurrent(fft_xcd_res_kernel<false, true>, grid, T, S, a); return true;
    case 1: l.launch_concurrent(fft_xcd_res_kernel<true, true>, grid, T, S, a); return true;
    case 2: l.launch_concurrent(fft_xcd_res_kernel<false, false>, grid, T, S, a); return true;
    case 3: l.launch_concurrent(fft_xcd_res_kernel<true, false>, grid, T, S, a); return true;
    case 4: l.launch_concurrent(fft_xcd_res_kernel<false, true, true>, grid, T, S, a); return true;    // diagnostic: in-kernel phase stamps
    case 6: l.launch_concurrent(fft_xcd_res_kernel<false, false, true>, grid, T, S, a); return true;
  }
  return false;
}
#endif

// mixed-radix kernels with compile-time plans: own translation unit (mixed_ct_kernels.hip) in the product build
template <class L> bool launch_mixedct(int id, const MixedArgs& a, unsigned grid, L& l);
#if defined(MI355_MIXEDCT_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class L> bool launch_mixedct(int id, const MixedArgs& a, unsigned grid, L& l) {
  int cur = 0;
#define X(N, T, TH, ...)                                                                                   \
  if (id == cur++) {                                                                                       \
    using M = MixedCt<N, T, TH, __VA_ARGS__>;                                                              \
    l.launch(fft_lines_mixedct_kernel<M>, grid, (unsigned)M::THREADS, (unsigned)M::LDS_BYTES, a);        \
    return true;                                                                                           \
  }
  MI355_MIXEDCT_LIST(X)
#undef X
  (void)cur;
  return false;
}
#endif
// lines of 2^13 / 2^14 / 2^15 points held in the registers of one workgroup (kern_line_reg.hpp); same translation unit as the
// mixed-radix instances.  lg = log2 N.
template <class L> bool launch_line_reg(int lg, const MixedArgs& a, unsigned grid, L& l);
#if defined(MI355_MIXEDCT_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
template <class C, class L> void launch_line_reg_cfg(const MixedArgs& a, unsigned grid, L& l) {
  if (a.swap_in) l.launch(fft_line_reg_kernel<C, true>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);
  else l.launch(fft_line_reg_kernel<C, false>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);
}
template <class L> bool launch_line_reg(int lg, const MixedArgs& a, unsigned grid, L& l) {
  if (lg == 12) { launch_line_reg_cfg<LineRegCfg<4096, 16, 8>>(a, grid, l); return true; }
  if (lg == 13) { launch_line_reg_cfg<LineRegCfg<8192, 16, 16>>(a, grid, l); return true; }
  if (lg == 14) { launch_line_reg_cfg<LineRegCfg<16384, 32, 16>>(a, grid, l); return true; }
  if (lg == 15) {   // the dedicated form of the same scheme (kern_line32k.hpp): the generic template spills 344 B per lane at this size (177 vs 288 GPoints/s)
    if (a.swap_in) l.launch(fft_line32k_kernel<true>, grid, (unsigned)Line32kCfg::THREADS, (unsigned)Line32kCfg::LDS_BYTES, a);
    else l.launch(fft_line32k_kernel<false>, grid, (unsigned)Line32kCfg::THREADS, (unsigned)Line32kCfg::LDS_BYTES, a);
    return true;
  }
  return false;
}
#endif

template <class L> bool launch_stage(int radix, const StageArgs& a, unsigned grid, L& l) {
  switch (radix) {
#define MI_STAGE_CASE(R) case R: l.launch(stockham_stage_kernel<R>, grid, 256u, 0u, a); return true;
    MI_STAGE_CASE(2) MI_STAGE_CASE(3) MI_STAGE_CASE(4) MI_STAGE_CASE(5) MI_STAGE_CASE(7) MI_STAGE_CASE(8)
    MI_STAGE_CASE(11) MI_STAGE_CASE(13) MI_STAGE_CASE(16) MI_STAGE_CASE(32)
#undef MI_STAGE_CASE
  }
  return false;
}

// LinesFn: bool(int family, int id, const LineArgs&, unsigned grid) — supplied by the caller because the
// per-family instantiations live in different translation units in the product build.
// the circular forms of both (the kernel on WBrickCfg / WRBrickCfg, routes bricks-conv-ols[..,wrap] / bricks-rconv-ols[..,wrap]): each in a unit of its own
// (bricks_conv_ols_wrap.hip, bricks_rconv_ols_wrap.hip)
template <class L> bool launch_bricks_conv_ols_wrap(int id, const BricksArgs& a, unsigned grid, L& l);
template <class L> bool launch_bricks_rconv_ols_wrap(int id, const BricksArgs& a, unsigned grid, L& l);
#define MI355_BRICK_WRAP_LAUNCHER(NAME)                                                               \
  template <class L> bool NAME(int id, const BricksArgs& a, unsigned grid, L& l) {                    \
    int cur = 0;                                                                                      \
    MI355_BRICK_KERNEL_LIST(X)                                                                        \
    (void)cur; (void)a; (void)grid; (void)l;                                                          \
    return false;                                                                                     \
  }
#if defined(MI355_BRICKS_WRAP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, TH)                                                                                      \
  if (id == cur) {                                                                                    \
    using C = WBrickCfg<P, TH>;                                                                       \
    l.launch(fft_bricks_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);   \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_BRICK_WRAP_LAUNCHER(launch_bricks_conv_ols_wrap)
#undef X
#endif
#if defined(MI355_RBRICKS_WRAP_DEFINE_INSTANCES) || defined(MI355_HOST_EMU)
#define X(P, TH)                                                                                      \
  if (id == cur) {                                                                                    \
    using C = WRBrickCfg<P, TH>;                                                                      \
    l.launch(fft_bricks_conv_ols_kernel<C>, grid, (unsigned)C::THREADS, (unsigned)C::LDS_BYTES, a);   \
    return true;                                                                                      \
  }                                                                                                   \
  ++cur;
MI355_BRICK_WRAP_LAUNCHER(launch_bricks_rconv_ols_wrap)
#undef X
#endif
#undef MI355_BRICK_WRAP_LAUNCHER

template <class L, class LinesFn, class XcdFn>
bool dispatch_step(const Step& s, void* const ptr[STEP_PTRS], L& l, LinesFn&& lines_fn, XcdFn&& xcd_fn) {
  switch (s.kind) {
    case ST_XCD_RES:
    case ST_XCD_FUSED: {
      XcdFusedArgs a{};
      a.in = (const cf*)ptr[XP_IN]; a.out = (cf*)ptr[XP_OUT]; a.wslots = (cf*)ptr[XP_WSLOTS]; a.ctl = (XcdCtl*)ptr[XP_CTL];
      const char* tb = (const char*)ptr[XP_TABLE];
      a.tw_a = (const cf*)(tb + s.i[XS_TW_A_OFF]); a.tw_b = (const cf*)(tb + s.i[XS_TW_B_OFF]); a.tw_lo = (const cf*)(tb + s.i[XS_TW_LO_OFF]); a.tw_hi = (const cf*)(tb + s.i[XS_TW_HI_OFF]);
      a.num_transforms = s.i[XS_TRANSFORMS]; a.N = s.i[XS_N]; a.fs_shift = (int)s.i[XS_FS_SHIFT]; a.fs_lo_mask = (unsigned)s.i[XS_FS_LO_MASK];
      a.in_pitch = s.i[XS_IN_PITCH]; a.out_pitch = s.i[XS_OUT_PITCH];
      a.scale = s.f[F_SCALE];
      a.sticky_error = l.sticky_error_word();
      a.spin_limit = s.i[XS_SPIN_LIMIT] > 0 ? (unsigned)s.i[XS_SPIN_LIMIT] : 4000000u;
      a.split = (unsigned)s.i[XS_SPLIT]; a.slots = (unsigned)s.i[XS_SLOTS]; a.solo = (unsigned)s.i[XS_SOLO];
      a.conv_k = (unsigned)s.i[XS_CONV_K]; a.conv_conj = (unsigned)s.i[XS_CONV_CONJ]; a.out_kernel_pitch = s.i[XS_OUT_KERNEL_PITCH];
      a.mul = a.conv_k ? (const cf*)((const char*)ptr[XP_WSLOTS] + s.i[XS_MUL_OFF]) : nullptr;   // the kernel spectra sit in the same workspace arena as the slots
      a.v_in_lo = (int)s.imap.lo[0]; a.v_in_hi = (int)s.imap.hi[0]; a.v_out_lo = (int)s.omap.lo[0]; a.v_out_hi = (int)s.omap.hi[0];
      a.v_zlo = (int)s.omap.zlo[0]; a.v_zhi = (int)s.omap.zhi[0];   // (VIEW instances only; the planner fills the two maps)
      a.v_split = (int)s.i[XS_V_SPLIT]; a.v_shift = (int)s.i[XS_V_SHIFT];              // (CONV_VIEW only)
      if (s.kind == ST_XCD_RES) return launch_xcd_res(s.variant, a, s.grid, l);
      return xcd_fn(s.variant, a, s.grid);
    }
    case ST_LINES: {
      LineArgs a{};
      a.in = (const cf*)ptr[LP_IN]; a.out = (cf*)ptr[LP_OUT]; a.tw = (const cf*)ptr[LP_TW]; a.tw_lo = (const cf*)ptr[LP_TW_LO]; a.tw_hi = (const cf*)ptr[LP_TW_HI];
      a.num_tiles = s.i[LS_TILES]; a.num_lines = s.i[LS_LINES];
      a.in_S = s.i[LS_IN_S]; a.in_outer_stride = s.i[LS_IN_OUTER]; a.out_S = s.i[LS_OUT_S]; a.out_outer_stride = s.i[LS_OUT_OUTER];
      a.fs_shift = (int)s.i[LS_FS_SHIFT]; a.fs_lo_mask = (unsigned)s.i[LS_FS_LO_MASK]; a.fs_group = s.i[LS_FS_GROUP] ? s.i[LS_FS_GROUP] : 1; a.real_mode = (int)s.i[LS_MODE];
      // (LM_MUL and Bluestein's mapped launches have no four-step roots: i[LS_MUL_CONJ], i[LS_CHIRP_FLAGS] are these two slots, and the kernels read
      // them as a.mul_conj, a.chirp_flags, the second names of the same two fields)
      a.mapped = (int)s.i[LS_MAPPED];
      if (a.mapped) { a.imap = s.imap; a.omap = s.omap; }
      a.h16 = (int)s.i[LS_H16];
      a.scale = s.f[F_SCALE];
      if (a.real_mode == LM_RCONV) {   // real fftconv line: p[LP_RCONV_SPECTRUM] (tw_hi) is the packed kernel spectrum; the HI roots sit directly behind the 1024 LO roots (one table)
        a.conj = (int)s.i[LS_CONJ]; a.rconv_split = (int)s.i[LS_RCONV_SPLIT]; a.rconv_padD = (int)s.i[LS_RCONV_PADD];
      }
      if (a.real_mode == LM_RCONV_OLS || a.real_mode == LM_CONV_OLS) {
        // overlap-save on real lines (LM_RCONV's pointers) and on complex ones (p[LP_MUL_SPECTRUM] (tw_lo) is the kernel spectrum on P points): no padded domain;
        // the block geometry in an argument block of its own (kern_lines.hpp RconvOls)
        RconvOlsArgs oa{};
        a.conj = (int)s.i[LS_CONJ];
        oa.a = a;
        const OlsAxis g = ols_axis_of(s.i, 0);
        oa.o.fN = (int)g.fN; oa.o.plim = (int)g.plim; oa.o.nb = (int)g.nb; oa.o.L = (int)g.L; oa.o.w0 = (int)g.w0; oa.o.pre = (int)g.pre;
        if (s.i[LS_OLS_WRAP]) return a.real_mode == LM_RCONV_OLS ? launch_lines_rconv_ols_wrap(s.variant, oa, s.grid, l) : launch_lines_conv_ols_wrap(s.variant, oa, s.grid, l);   // circular: the WRAP instances
        return a.real_mode == LM_RCONV_OLS ? launch_lines_rconv_ols(s.variant, oa, s.grid, l) : launch_lines_conv_ols(s.variant, oa, s.grid, l);
      }
      if (s.i[LS_OLS_WRAP]) {   // circular tiles and bricks (the spectrum launches never carry the flag)
        if (a.real_mode == LM_TILES_CONV_OLS) return launch_tiles_conv_ols_wrap(s.variant, tiles_args_of(s, ptr), s.grid, l);
        if (a.real_mode == LM_TILES_RCONV_OLS) return launch_tiles_rconv_ols_wrap(s.variant, tiles_args_of(s, ptr), s.grid, l);
        if (a.real_mode == LM_BRICKS_CONV_OLS) return launch_bricks_conv_ols_wrap(s.variant, bricks_args_of(s, ptr), s.grid, l);
        if (a.real_mode == LM_BRICKS_RCONV_OLS) return launch_bricks_rconv_ols_wrap(s.variant, bricks_args_of(s, ptr), s.grid, l);
        return false;
      }
      if (s.i[LS_TILES_KERNELS] != 0 && (a.real_mode == LM_TILES_CONV_OLS || a.real_mode == LM_TILES_RCONV_OLS)) {   // fftConv.groups: every output kernel in this launch (linear tiles only)
        return a.real_mode == LM_TILES_CONV_OLS ? launch_tiles_conv_ols_group(s.variant, tiles_group_args_of(s, ptr), s.grid, l)
                                                : launch_tiles_rconv_ols_group(s.variant, tiles_group_args_of(s, ptr), s.grid, l);
      }
      if (s.i[LS_TILES_CHANNELS] > 1) {   // the sum over input channels (linear tiles only; the spectrum launches never carry the count)
        if (a.real_mode == LM_TILES_CONV_OLS) return launch_tiles_conv_ols_sum(s.variant, tiles_sum_args_of(s, ptr), s.grid, l);
        if (a.real_mode == LM_TILES_RCONV_OLS) return launch_tiles_rconv_ols_sum(s.variant, tiles_sum_args_of(s, ptr), s.grid, l);
      }
      if (a.real_mode == LM_TILES_CONV_OLS || a.real_mode == LM_TILES_SPECTRUM) return launch_tiles_conv_ols(s.variant, tiles_args_of(s, ptr), s.grid, l);   // rank-2 overlap-save tiles
      if (a.real_mode == LM_TILES_RCONV_OLS || a.real_mode == LM_TILES_RSPECTRUM) return launch_tiles_rconv_ols(s.variant, tiles_args_of(s, ptr), s.grid, l);   // and on real tile pairs
      if (a.real_mode == LM_BRICKS_CONV_OLS || a.real_mode == LM_BRICKS_SPECTRUM) return launch_bricks_conv_ols(s.variant, bricks_args_of(s, ptr), s.grid, l);   // rank-3 overlap-save bricks
      if (a.real_mode == LM_BRICKS_RCONV_OLS || a.real_mode == LM_BRICKS_RSPECTRUM) return launch_bricks_rconv_ols(s.variant, bricks_args_of(s, ptr), s.grid, l);   // and on real brick pairs
      const LineKernelMeta& m = line_kernel_registry()[(size_t)s.variant];
      return lines_fn(family_of_line_kernel(m), s.variant, a, s.grid);
    }
    case ST_TRIG_PRE:
    case ST_TRIG_POST: {
      TrigArgs a{};
      a.x = (const float*)ptr[TGP_X]; a.z = (cf*)ptr[TGP_Z]; a.y = (float*)ptr[TGP_Y];
      a.lines = s.i[TG_LINES]; a.N = s.i[TG_N]; a.L = s.i[TG_L]; a.S = s.i[TG_S]; a.kind = (int)s.i[TG_KIND]; a.scale = s.f[F_SCALE]; a.stride = s.i[TG_STRIDE] ? s.i[TG_STRIDE] : 1;
      if (a.kind >= TK_REAL && a.stride > 1) {
        if (s.kind == ST_TRIG_PRE) l.launch(trig_real_pre_tiled_kernel, s.grid, 256u, 0u, a); else l.launch(trig_real_post_tiled_kernel, s.grid, 256u, 0u, a);
      } else if (a.kind >= TK_REAL) {
        if (s.kind == ST_TRIG_PRE) l.launch(trig_real_pre_kernel, s.grid, 256u, 0u, a); else l.launch(trig_real_post_kernel, s.grid, 256u, 0u, a);
      } else if (s.kind == ST_TRIG_PRE) l.launch(trig_pre_kernel, s.grid, 256u, 0u, a); else l.launch(trig_post_kernel, s.grid, 256u, 0u, a);
      return true;
    }
    case ST_LINES_MIXED: {
      MixedArgs a{};
      a.in = (const cf*)ptr[P_SRC]; a.out = (cf*)ptr[P_DST]; a.tw = (const cf*)ptr[P_TW];
      a.lines = s.i[MX_LINES]; a.N = (int)s.i[MX_N]; a.S = s.i[MX_S]; a.T = (int)s.i[MX_T]; a.nst = (int)s.i[MX_NST];
      a.swap_in = a.swap_out = (int)s.i[MX_SWAP];
      a.scale = s.f[F_SCALE];
      if (s.variant >= 1000) return launch_line_reg(s.variant - 1000, a, s.grid, l);   // 2^13 .. 2^15 in one workgroup's registers (kern_line_reg.hpp)
      if (s.variant > 0) return launch_mixedct(s.variant - 1, a, s.grid, l);   // compile-time plan: nothing else to pass
      {
        const auto rcp = [](unsigned d) { return d > 1 ? (unsigned)((0x100000000ull + d - 1) / d) : 0u; };
        unsigned nsp = 1;
        for (int k = 0; k < a.nst; ++k) {
          a.radix[k] = (int)(s.i[MX_RADIX0 + k] >> 32); a.tw_off[k] = (int)(s.i[MX_RADIX0 + k] & 0xffffffff);
          a.rcp_nb[k] = rcp((unsigned)(a.N / a.radix[k])); a.rcp_nsp[k] = rcp(nsp);
          nsp *= (unsigned)a.radix[k];
        }
      }
      a.lds_bytes = (int)s.i[MX_LDS_BYTES]; a.tw_total = (int)s.i[MX_TW_TOTAL];
      l.launch(fft_lines_mixed_kernel, s.grid, (unsigned)s.i[MX_THREADS], (unsigned)(a.lds_bytes + MIXED_MAX_T * 8 + a.tw_total * 8), a);
      return true;
    }
    case ST_STAGE: {
      StageArgs a{};
      a.in = (const cf*)ptr[P_SRC]; a.out = (cf*)ptr[P_DST]; a.tw = (const cf*)ptr[P_TW];
      a.total = s.i[SG_TOTAL]; a.N = s.i[SG_N]; a.S = s.i[SG_S]; a.Nsp = s.i[SG_NSP]; a.swap_in = (int)s.i[SG_SWAP_IN]; a.swap_out = (int)s.i[SG_SWAP_OUT];
      a.scale = s.f[F_SCALE];
      return launch_stage(s.variant, a, s.grid, l);
    }
    case ST_R2C_POST: {
      R2cPostArgs a{};
      a.z = (const cf*)ptr[P_SRC]; a.x = (cf*)ptr[P_DST]; a.tw_lo = (const cf*)ptr[RSP_TW_LO]; a.tw_hi = (const cf*)ptr[RSP_TW_HI];
      a.H = s.i[RS_H]; a.batch = s.i[RS_BATCH]; a.x_line_stride = s.i[RS_LINE_STRIDE]; a.scale = s.f[F_SCALE]; a.shift = (int)s.i[RS_SHIFT]; a.mask = (unsigned)s.i[RS_MASK];
      l.launch(r2c_post_kernel, s.grid, 256u, 0u, a);
      return true;
    }
    case ST_C2R_PRE: {
      C2rPreArgs a{};
      a.x = (const cf*)ptr[P_SRC]; a.z = (cf*)ptr[P_DST]; a.tw_lo = (const cf*)ptr[RSP_TW_LO]; a.tw_hi = (const cf*)ptr[RSP_TW_HI];
      a.H = s.i[RS_H]; a.batch = s.i[RS_BATCH]; a.x_line_stride = s.i[RS_LINE_STRIDE]; a.shift = (int)s.i[RS_SHIFT]; a.mask = (unsigned)s.i[RS_MASK];
      l.launch(c2r_pre_kernel, s.grid, 256u, 0u, a);
      return true;
    }
    case ST_REAL_TO_COMPLEX:
      l.launch(real_to_complex_kernel, s.grid, 256u, 0u, (const float*)ptr[P_SRC], (cf*)ptr[P_DST], (long long)s.i[S_COUNT]);
      return true;
    case ST_COMPLEX_TO_REAL:
      l.launch(complex_to_real_kernel, s.grid, 256u, 0u, (const cf*)ptr[P_SRC], (float*)ptr[P_DST], (long long)s.i[S_COUNT], s.f[F_SCALE]);
      return true;
    case ST_PACK_HALF:
      l.launch(pack_half_kernel, s.grid, 256u, 0u, (const cf*)ptr[P_SRC], (cf*)ptr[P_DST], (long long)s.i[PH_N], (long long)s.i[PH_P], (long long)s.i[PH_BATCH],
               (long long)s.i[PH_PACKED_STRIDE], s.f[F_SCALE]);
      return true;
    case ST_UNPACK_HERM:
      l.launch(unpack_hermitian_kernel, s.grid, 256u, 0u, (const cf*)ptr[P_SRC], (cf*)ptr[P_DST], (long long)s.i[PH_N], (long long)s.i[PH_P],
               (long long)s.i[PH_BATCH], (long long)s.i[PH_PACKED_STRIDE]);
      return true;
    case ST_POINTWISE:
      if (s.i[PW_ITEM_LINES] > 0) {  // fftConv.groups: the product summed over one group's channels out of the item's PW_ITEM_LINES lines
        l.launch(pointwise_group_sum_kernel, s.grid, 256u, 0u, (const cf*)ptr[P_SRC], (cf*)ptr[P_DST], (const cf*)ptr[PWP_KERNEL], (long long)s.i[PW_L], (long long)s.i[PW_TOTAL],
                 (int)s.i[PW_CHANNELS], (int)s.i[PW_ITEM_LINES], (int)s.i[PW_CONJ], s.f[F_SCALE]);
        return true;
      }
      if (s.i[PW_CHANNELS] > 1) {    // fftConv.inputChannels: the product summed over the input channels
        l.launch(pointwise_sum_kernel, s.grid, 256u, 0u, (const cf*)ptr[P_SRC], (cf*)ptr[P_DST], (const cf*)ptr[PWP_KERNEL], (long long)s.i[PW_L], (long long)s.i[PW_TOTAL],
                 (int)s.i[PW_CHANNELS], (int)s.i[PW_CONJ], s.f[F_SCALE]);
        return true;
      }
      l.launch(pointwise_mul_kernel, s.grid, 256u, 0u, (const cf*)ptr[P_SRC], (cf*)ptr[P_DST], (const cf*)ptr[PWP_KERNEL], (long long)s.i[PW_L], (long long)s.i[PW_TOTAL],
               (int)s.i[PW_CONJ], s.f[F_SCALE]);
      return true;
    case ST_GATHER:
    case ST_SCATTER: {
      StridedArgs a{};
      a.src = ptr[P_SRC]; a.dst = ptr[P_DST];
      a.total = s.i[GS_TOTAL]; a.per = s.i[GS_PER]; a.rank = (int)s.i[GS_RANK];
      a.phys_offset = s.i[GS_PHYS_OFFSET]; a.phys_batch_stride = s.i[GS_PHYS_BATCH_STRIDE]; a.dense_offset = s.i[GS_DENSE_OFFSET]; a.dense_batch_stride = s.i[GS_DENSE_BATCH_STRIDE];
      for (int d = 0; d < 8; ++d) { a.shape[d] = s.shape[d] ? s.shape[d] : 1; a.phys_stride[d] = s.sa[d]; a.dense_stride[d] = s.sb[d]; }
      const bool real = s.i[GS_REAL] != 0;     // element type: 0 complex, 1 real (r2c input / c2r output sides)
      if (s.kind == ST_GATHER) { if (real) l.launch(strided_copy_kernel<true, float>, s.grid, 256u, 0u, a); else l.launch(strided_copy_kernel<true, cf>, s.grid, 256u, 0u, a); }
      else { if (real) l.launch(strided_copy_kernel<false, float>, s.grid, 256u, 0u, a); else l.launch(strided_copy_kernel<false, cf>, s.grid, 256u, 0u, a); }
      return true;
    }
    case ST_FFTCONV_FUSED: {
      FusedConvArgs a{};
      a.in = (const cf*)ptr[FCP_IN]; a.kern = (const cf*)ptr[FCP_KERN]; a.out = (cf*)ptr[FCP_OUT]; a.tw = (const cf*)ptr[FCP_TW];
      a.batch = s.i[FC_BATCH]; a.K = (int)s.i[FC_K]; a.kern_len = (int)s.i[FC_KERN_LEN]; a.conj_kernel = (int)s.i[FC_CONJ];
      a.in_offset = s.i[FC_IN_OFFSET]; a.in_batch_stride = s.i[FC_IN_BATCH_STRIDE]; a.in_stride = s.i[FC_IN_STRIDE];
      a.out_offset = s.i[FC_OUT_OFFSET]; a.out_kernel_stride = s.i[FC_OUT_KERNEL_STRIDE]; a.out_batch_stride = s.i[FC_OUT_BATCH_STRIDE]; a.out_stride = s.i[FC_OUT_STRIDE];
      a.scale = s.f[F_SCALE];
      return launch_fftconv_fused(s.variant, a, s.grid, l);
    }
    case ST_CHIRP_PRE:
    case ST_CHIRP_POST: {
      ChirpArgs a{};
      a.in = (const cf*)ptr[P_SRC]; a.out = (cf*)ptr[P_DST]; a.chirp = (const cf*)ptr[CHP_CHIRP];
      a.N = s.i[CH_N]; a.M = s.i[CH_M]; a.lines = s.i[CH_LINES]; a.swap_in = (int)s.i[CH_SWAP_IN]; a.swap_out = (int)s.i[CH_SWAP_OUT]; a.scale = s.f[F_SCALE];
      if (s.kind == ST_CHIRP_PRE) l.launch(bluestein_pre_kernel, s.grid, 256u, 0u, a);
      else l.launch(bluestein_post_kernel, s.grid, 256u, 0u, a);
      return true;
    }
    case ST_ZERO_OUTSIDE: {
      ZeroOutsideArgs a{};
      a.data = ptr[P_DATA]; a.total = s.i[ZO_TOTAL]; a.per = s.i[ZO_PER]; a.rank = (int)s.i[ZO_RANK];
      for (int d = 0; d < 8; ++d) { a.shape[d] = s.shape[d] ? s.shape[d] : 1; a.start[d] = s.sa[d]; a.end[d] = d < a.rank ? s.sb[d] : 1; }
      if (s.i[ZO_REAL]) l.launch(zero_outside_kernel<float>, s.grid, 256u, 0u, a); else l.launch(zero_outside_kernel<cf>, s.grid, 256u, 0u, a);
      return true;
    }
    case ST_ZERO:
      l.launch(zero_kernel, s.grid, 256u, 0u, (float*)ptr[P_DATA], (long long)s.i[S_COUNT]);
      return true;
    case ST_SCALE:
      l.launch(scale_kernel, s.grid, 256u, 0u, (float*)ptr[P_DATA], (long long)s.i[S_COUNT], s.f[F_SCALE]);
      return true;
    case ST_COPY:
      if (ptr[P_SRC] != ptr[P_DST]) l.copy(ptr[P_DST], ptr[P_SRC], (size_t)s.i[S_COUNT]);
      return true;
    case ST_F16_TO_F32:
      l.launch(f16_to_f32_kernel, s.grid, 256u, 0u, (const _Float16*)ptr[P_SRC], (float*)ptr[P_DST], (long long)s.i[S_COUNT]);
      return true;
    case ST_F32_TO_F16:
      l.launch(f32_to_f16_kernel, s.grid, 256u, 0u, (const float*)ptr[P_SRC], (_Float16*)ptr[P_DST], (long long)s.i[S_COUNT]);
      return true;
  }
  return false;
}

}  // namespace mi355
