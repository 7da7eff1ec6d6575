// plan.hpp — host-side planner: turns a createPlan option block into a list of kernel launches.
//
// Replaces the reference's runtime planners for the hot path:
//   src/runtime/plans/c2c.js  (C2CPlan ctor :533-1229, exec :3607-4211)   -> build_c2c
//   src/runtime/plans/r2c.js  (:52-512, core :1518-1557)                  -> build_r2c
//   src/runtime/plans/c2r.js  (:146-, core :1743-1763)                    -> build_c2r
//   src/runtime/plans/fftconv.js (:308-709, exec :1415-1712)              -> build_fftconv
//   src/plan.js factorizeRadices (:20-33) / createFftPlan (:1298-1512)    -> emit_axis + radix factoring
// The reference's ~75 % of planner code that works around WebGPU binding/buffer limits (large_policy,
// segmented_io, BufferView windows) has no counterpart: one HIP allocation spans 288 GB.
//
// This file has no HIP dependency: the same planner drives the HIP launcher (api.hip) and the host
// emulation used by the CPU tests (tests/emu).
#pragma once
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/mi355fft.h"

namespace mi355 {

struct float2h { float x, y; };

struct LineKernelMeta {
  int id;
  int N, R0, R1, R2, T;
  bool in_col, out_col, swap_in, swap_out;
  int twid;
  int threads, lds_bytes, tw_elems;
};
const std::vector<LineKernelMeta>& line_kernel_registry();
const LineKernelMeta* find_line_kernel(int N, bool in_col, bool out_col, bool swap_in, bool swap_out, int twid);

// fused single-launch fftconv kernels (kern_fftconv.hpp): X(N, R0, R1, TL)
#define MI355_CONV_KERNEL_LIST(X) \
  X(64, 8, 8, 4) X(64, 8, 8, 16) X(128, 16, 8, 4) X(128, 16, 8, 16) X(256, 16, 16, 4) X(256, 16, 16, 16) \
  X(512, 32, 16, 4) X(512, 32, 16, 16) X(1024, 32, 32, 4) X(1024, 32, 32, 16)
struct ConvKernelMeta { int id, N, R0, R1, TL; };
// overlap-save tile kernels of rank-2 fftconv (kern_tiles.hpp fft_tiles_conv_ols_kernel): X(P, R0, R1, threads), id = position in the list.
// LDS: the P x P tile at a pitch of P + 1 elements and the stage-1 roots
#define MI355_TILE_KERNEL_LIST(X) X(64, 8, 8, 256) X(128, 16, 8, 1024)
constexpr int tile_kernel_lds_bytes(int P, int R0, int R1) { return (P * (P + 1) + (R1 - 1) * R0) * 8; }
// the sum form (fftConv.inputChannels > 1: STileCfg / SRTileCfg, a loop over the input channels around load, forward and multiply-accumulate, one inverse and
// one store a tile): a list, ids and units of its own (tiles_conv_ols_sum.hip, tiles_rconv_ols_sum.hip).  P = 64 alone: the accumulators are E more complex
// registers a thread, which P = 128 on 1024 threads (124 of 128 VGPRs) cannot hold
#define MI355_TILE_SUM_KERNEL_LIST(X) X(64, 8, 8, 256)
// the grouped forms (fftConv.groups > 1: fft_tiles_conv_ols_group_kernel, every output kernel in ONE launch, a work item carrying its kernel index): X(P, R0, R1,
// threads, depthwise).  depthwise = 0: Cg = C / G > 1 channels summed per item (GTileCfg / GRTileCfg, the sum form's accumulators); 1: Cg = 1 (DTileCfg /
// DRTileCfg: the single-channel form, no accumulators).  A list, ids and units of its own (tiles_conv_ols_group.hip, tiles_rconv_ols_group.hip); P = 64 alone
#define MI355_TILE_GROUP_KERNEL_LIST(X) X(64, 8, 8, 256, 0) X(64, 8, 8, 256, 1)
struct TileKernelMeta { int id, P, R0, R1, threads, lds_bytes; bool real; bool sum; int group = 0; };   // group: 0 none, 1 the grouped sum form, 2 the grouped depthwise form
// `real`: the same list as instances of fft_tiles_conv_ols_kernel on an RTileCfg (real fftconv: two real tiles as re / im of a complex one), a unit of their own
// (tiles_rconv_ols.hip); an id counts positions in the list for both forms, and the step's line mode says which form is launched
const TileKernelMeta* find_tile_kernel(int P, bool real = false, bool sum = false, int group = 0);
// overlap-save brick kernels of rank-3 fftconv (kern_bricks.hpp fft_bricks_conv_ols_kernel): X(P, threads), id = position in the list.  LDS: the P^3 brick
// at pitches of P + 1 and P (P + 1) elements.  `real`: the same list on an RBrickCfg (bricks_rconv_ols.hip), as with the tiles
#define MI355_BRICK_KERNEL_LIST(X) X(16, 256)
constexpr int brick_kernel_lds_bytes(int P) { return P * P * (P + 1) * 8; }
struct BrickKernelMeta { int id, P, threads, lds_bytes; bool real; };
const BrickKernelMeta* find_brick_kernel(int P, bool real = false);
// mixed-radix line kernels with compile-time plans (kern_mixed_ct.hpp): id = position in the list
// instances: X(N, lines per workgroup, threads, radices...).  Tile shapes keep every stage's butterfly count (T * N / R) at or
// above the thread count and two workgroups per CU inside the LDS.
#define MI355_MIXEDCT_LIST(X)                                                                                                   \
  X(96, 32, 256, 8, 4, 3) X(192, 16, 256, 8, 8, 3) X(384, 4, 128, 16, 8, 3) X(768, 4, 256, 8, 8, 4, 3) X(1536, 2, 256, 8, 8, 8, 3)       \
  X(3072, 2, 512, 16, 8, 8, 3) X(160, 16, 256, 8, 4, 5) X(320, 8, 256, 8, 8, 5) X(640, 4, 256, 8, 8, 2, 5) X(1280, 2, 256, 8, 8, 4, 5)  \
  X(2560, 1, 256, 8, 8, 8, 5) X(1000, 4, 256, 8, 5, 5, 5) X(2000, 4, 512, 16, 5, 5, 5) X(3000, 2, 512, 8, 5, 5, 5, 3)                   \
  X(105, 32, 256, 7, 5, 3) X(1001, 8, 512, 13, 11, 7) X(360, 8, 256, 8, 5, 3, 3) X(1920, 4, 512, 16, 8, 5, 3) X(2187, 1, 256, 3, 3, 3, 3, 3, 3, 3) \
  X(500, 8, 256, 4, 5, 5, 5) X(1500, 2, 256, 4, 5, 5, 5, 3) X(120, 32, 256, 8, 5, 3) X(240, 16, 256, 4, 4, 5, 3) X(480, 8, 256, 8, 4, 5, 3) X(720, 4, 256, 16, 5, 3, 3) X(1440, 2, 256, 8, 4, 5, 3, 3) \
  /* r03: 2187 = 9*9*9*3 (radix 9 by direct evaluation with literal roots: 4 LDS passes instead of 7): 180 -> 194 GPoints/s.  Listed after the plan it \
     replaces: the registry walk takes the last match (MI355FFT_MIXED_CT=2: the first).  3000 = 8*25*15 and 1500 = 4*25*15 measured SLOWER than their \
     five-stage plans (168 vs 192, 145 vs 203: profiles/r03_mixed_radix_composite.log) and are not instantiated */ \
  X(2187, 2, 512, 9, 9, 9, 3)

struct MixedCtMeta { int id, N, T, threads, lds_bytes; std::vector<int> radices; };
const std::vector<MixedCtMeta>& mixedct_registry();

// XCD-fused four-step kernels: one entry per instance id, in id order (xcd_kernels.def, where the kinds are described)
enum XcdKind : int {
  XK_FUSED, XK_R2C, XK_C2R, XK_TWO_D, XK_VIEW,                 // LDS-resident passes (kern_xcd.hpp, kern_xcd_real.hpp)
  XK_RT, XK_RT_R2C, XK_RT_C2R, XK_HX, XK_RT1K, XK_RT1K_16, XK_RT1K_VIEW, XK_RT1K_2048, XK_CONV, XK_CONV_VIEW   // register tiles (kern_regtile.hpp)
};
struct XcdInstance { XcdKind kind; int N1, ra[3], ta, N2, rb[3], tb; bool inverse; };
constexpr XcdInstance XCD_INSTANCES[] = {
#define XCD_KERNEL(KIND, N1, A0, A1, A2, TA, N2, B0, B1, B2, TB, INV) {XK_##KIND, N1, {A0, A1, A2}, TA, N2, {B0, B1, B2}, TB, INV},
#include "xcd_kernels.def"
#undef XCD_KERNEL
};
constexpr int XCD_INSTANCE_COUNT = (int)(sizeof XCD_INSTANCES / sizeof XCD_INSTANCES[0]);
struct XcdKernelMeta : XcdInstance { int id, threads, lds_bytes; };   // + the launch shape (plan.cpp xcd_kernel_registry)
const std::vector<XcdKernelMeta>& xcd_kernel_registry();
const std::vector<ConvKernelMeta>& conv_kernel_registry();
// fft_xcd_rt1k_kernel (kern_regtile.hpp): the four-step root tables HI and LO staged in LDS once per launch, so that a row tile's six roots are LDS
// reads and not global loads queued behind the previous tile's stores.  Only where the instance fixes their size and they fit beside the exchange
// half: the 32-line 1024 x 1024 instances without predicates (N = 2^20: shift 10, 1024 + 1024 entries, 16 KB; plan.cpp xcd_roots).  0: global tables.
#ifndef MI355_RT1K_ROOTS_LDS
#define MI355_RT1K_ROOTS_LDS 1
#endif
// Same instances (the kernel's PIPE condition), both bit-identical to their 0 forms (profiles/rt1k_early_bfly_ab.log, one box, five interleaved rounds):
//   MI355_RT1K_LEAN_BFLY  the four radix-32 DFTs of a tile take their K = 4, 8, 12 butterflies from Rt1kBfly (kern_regtile.hpp): the re/im crossing and the
//                         negations are source modifiers of the packed adds and fmas instead of a sign-bit xor and a register copy per butterfly.
//                         1: 217.9 - 218.7 against the parent's 215.4 - 215.9 GPoints/s (+1.4 %), 240 VGPRs, no scratch: the default.
//   MI355_RT1K_EARLY_B    phase B's first 16 row loads are requested between the arrive and the wait of the A | B barrier when the counter bar[gslot][2]
//                         (kern_xcd.hpp) already certifies the columns they read; otherwise after the wait, as with 0.  1: 215.4 - 216.3 alone, 218.3 - 219.1
//                         on top of LEAN_BFLY (medians +0.1 %, ranges overlap both times): off by the project's rule.
#ifndef MI355_RT1K_LEAN_BFLY
#define MI355_RT1K_LEAN_BFLY 1
#endif
#ifndef MI355_RT1K_EARLY_B
#define MI355_RT1K_EARLY_B 0
#endif
constexpr int RT1K_ROOT_SHIFT = 10, RT1K_ROOT_HI = 1024, RT1K_ROOT_LO = 1 << RT1K_ROOT_SHIFT;
constexpr int rt1k_root_lds_elems(int tb, bool view, int N1) { return MI355_RT1K_ROOTS_LDS && tb == 32 && !view && N1 == 1024 ? RT1K_ROOT_HI + RT1K_ROOT_LO : 0; }

enum BufId : int { BUF_NONE = -1, BUF_INPUT = 0, BUF_OUTPUT = 1, BUF_WORK = 2, BUF_KERNEL = 3, BUF_TABLE = 4 };
struct PtrRef {
  int buf = BUF_NONE;
  int64_t off = 0;  // bytes
  PtrRef() {}
  PtrRef(int b, int64_t o) : buf(b), off(o) {}
  PtrRef plus(int64_t bytes) const { return PtrRef(buf, off + bytes); }
  bool same(const PtrRef& o) const { return buf == o.buf && off == o.off; }
};

// A side of a line-kernel launch as a map from logical coordinates to physical storage (layout strides,
// ioView, zeroPad fused into the first load / last store instead of separate gather / embed / zero / extract / scatter passes).
// Line G of the launch (all dims except `ax` in axis-0-fastest order, then the batch) and position idx along `ax`:
//   reads : inside [lo, hi) on every dim -> phys[offset + sum i_d * stride_d + b * batch_stride], else 0
//   writes: inside [lo, hi) on every dim -> stored, with the value replaced by 0 outside [zlo, zhi); else not stored
// a three-stage line kernel keeps its last stage table in LDS up to this many bytes (LineCfg::TW2_IN_LDS, plan.cpp make_meta)
#ifndef MI355_TW2_LDS_MAX
#define MI355_TW2_LDS_MAX (32 * 1024)
#endif

struct SideMap {
  int rank = 0, ax = 0;
  int dims[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  int lo[8] = {0}, hi[8] = {0}, zlo[8] = {0}, zhi[8] = {0};
  long long stride[8] = {0};
  long long offset = 0, batch_stride = 0;
};

enum StepKind : int {
  ST_LINES, ST_STAGE, ST_R2C_POST, ST_C2R_PRE, ST_REAL_TO_COMPLEX, ST_COMPLEX_TO_REAL, ST_PACK_HALF, ST_UNPACK_HERM,
  ST_POINTWISE, ST_GATHER, ST_SCATTER, ST_ZERO, ST_COPY, ST_SCALE, ST_FFTCONV_FUSED, ST_CHIRP_PRE, ST_CHIRP_POST, ST_ZERO_OUTSIDE, ST_XCD_FUSED, ST_LINES_MIXED, ST_TRIG_PRE, ST_TRIG_POST, ST_XCD_RES,
  ST_F16_TO_F32, ST_F32_TO_F16   // f16-storage plans: i[0] scalars widened / rounded to nearest even (kern_f16.hpp)
};

// ---- the step contract: what the planner (plan.cpp) writes into a Step's p[] / i[] / f[] slots and the dispatcher (dispatch.hpp) reads.
// One enum of slot names per step kind; two names with one value mark a slot that means different things per mode.  Names of i[] slots
// carry their kind's prefix (LS_, XS_, TG_, ...), names of p[] slots that prefix with a P (LP_, XP_, TGP_, ...; P_ where kinds share them).
constexpr int STEP_PTRS = 5, STEP_INTS = 20, STEP_FLOATS = 2;

// every kind: f[F_SCALE]; the kinds with one source and one destination (or one array worked on in place) and a count in i[S_COUNT]:
// ST_ZERO / ST_SCALE (32-bit words), ST_COPY (bytes), ST_REAL_TO_COMPLEX / ST_COMPLEX_TO_REAL / ST_F16_TO_F32 / ST_F32_TO_F16 (elements)
enum StepSlot { P_SRC = 0, P_DATA = 0, P_DST = 1, P_TW = 2, S_COUNT = 0, F_SCALE = 0 };
static_assert(P_TW < STEP_PTRS && S_COUNT < STEP_INTS && F_SCALE < STEP_FLOATS, "shared slots");

// what a line-kernel launch computes (LineArgs::real_mode, Step::i[LS_MODE])
enum LineMode : int {
  LM_C2C = 0,
  LM_R2C = 1,         // r2c: the split behind the last stage (fft_lines_r2c_kernel)
  LM_C2R = 2,         // c2r: the pre-split in the first-stage loads (fft_lines_c2r_kernel)
  LM_MUL = 4,         // c2c times a spectrum in the last store (fft_lines_mul_kernel): fftconv products, Bluestein's forward launch
  LM_DCT2 = 5, LM_DST2 = 6,   // one-launch DCT-II / DST-II on the r2c kernel
  LM_DCT3 = 7, LM_DST3 = 8,   // one-launch DCT-III / DST-III on the c2r kernel
  LM_RCONV = 9,       // real fftconv line: r2c, product and c2r in one launch (fft_lines_rconv_kernel)
  LM_RCONV_OLS = 10,  // its overlap-save form (fft_lines_rconv_ols_kernel)
  LM_CONV_OLS = 11,   // overlap-save on complex lines: forward FFT, product and inverse FFT of a block in one launch (fft_lines_conv_ols_kernel)
  LM_TILES_CONV_OLS = 12,   // overlap-save on rank-2 complex tiles (kern_tiles.hpp fft_tiles_conv_ols_kernel): `variant` is a TileKernelMeta id, not a line kernel's
  LM_TILES_SPECTRUM = 13,   // its forward half on the zero-padded kernels: the K spectra in the order the product reads them
  LM_TILES_RCONV_OLS = 14,  // overlap-save on rank-2 real tiles, two of them as re / im of a complex tile (kern_tiles.hpp fft_tiles_conv_ols_kernel on an RTileCfg); `variant` as above
  LM_TILES_RSPECTRUM = 15,  // its forward half on the zero-padded real kernels, one a work item: the K complex spectra as LM_TILES_SPECTRUM stores them
  LM_BRICKS_CONV_OLS = 16,  // overlap-save on rank-3 complex bricks (kern_bricks.hpp fft_bricks_conv_ols_kernel): `variant` is a BrickKernelMeta id
  LM_BRICKS_SPECTRUM = 17,  // its forward half on the zero-padded kernels: the K spectra in the order the product reads them
  LM_BRICKS_RCONV_OLS = 18, // overlap-save on rank-3 real bricks, two of them as re / im of a complex brick (the kernel on an RBrickCfg)
  LM_BRICKS_RSPECTRUM = 19  // its forward half on the zero-padded real kernels, one a work item
};
// Bluestein's two mapped launches: bits of i[LS_CHIRP_FLAGS] (LineArgs::fs_lo_mask)
enum : unsigned { LINES_CHIRP = 1, LINES_CHIRP_SWAP = 2 };   // multiply by the chirp in p[LP_CHIRP]; inverse transform: the chirp's conjugate

// ST_LINES
enum LinesSlot {
  LS_TILES = 0, LS_LINES, LS_IN_S, LS_IN_OUTER, LS_OUT_S, LS_OUT_OUTER,
  LS_FS_SHIFT = 6, LS_MUL_CONJ = 6, LS_OLS2_FN_PLIM = 6, LS_TILES_LANE_K = 6,   // four-step roots: HI[m >> shift]; LM_MUL: multiply by the spectrum's conjugate; the brick modes: axis 2's fN (low 32 bits) and plim
  LS_FS_LO_MASK = 7, LS_CHIRP_FLAGS = 7, LS_OLS2_NB_L = 7, LS_TILES_KERNELS = 7, // ... LO[m & mask]; mapped LM_C2C / LM_MUL of Bluestein: LINES_CHIRP bits; the brick modes: axis 2's nb and L
  LS_FS_GROUP = 8, LS_OLS2_W0_PRE = 8, LS_TILES_CHANNELS = 8,   // PASS_B: rows per transform; COL_RAGGED: tiles per group (0 reads as 1); the brick modes: axis 2's w0 and pre;
                                             // LM_TILES_CONV_OLS / LM_TILES_RCONV_OLS: input channels summed per tile (0, 1: none; above: the sum instances, `variant` an id of their list)
                                             // The grouped tile launch (fftConv.groups > 1, all output kernels in one launch: LS_TILES_KERNELS != 0, `variant` an id of
                                             // MI355_TILE_GROUP_KERNEL_LIST): LS_TILES_CHANNELS holds Cg (low 32 bits) and C, LS_TILES_KERNELS K (low) and Kg = K / G,
                                             // LS_TILES_LANE_K the step between the output lanes of consecutive kernels (ConvGeom::lane_k)
  LS_MODE = 9,                               // LineMode
  LS_MAPPED = 10,                            // sides through Step::imap / omap
  LS_H16 = 11,                               // binary16 sides (f16-storage)
  LS_CONJ = 12,                              // LM_RCONV, LM_RCONV_OLS, LM_CONV_OLS, LM_TILES_CONV_OLS, LM_TILES_RCONV_OLS: correlation
  LS_RCONV_SPLIT = 13, LS_OLS_FN = 13,       // LM_RCONV: ConvGeom split / padD;  the overlap-save modes: the block geometry, written and read by ols_store / ols_axis_of
  LS_RCONV_PADD = 14, LS_OLS_PLIM = 14,      // below and by nothing else
  LS_OLS_NB = 15, LS_OLS_L = 16, LS_OLS_W0 = 17, LS_OLS_PRE = 18,
  LS_OLS_WRAP = 19,                          // the overlap-save modes: circular boundary, a block's signal indices are taken modulo fN (the kernels' WRAP instances)
  LS_LAST = LS_OLS_WRAP
};
static_assert(LS_LAST < STEP_INTS, "ST_LINES slots");
// axis 2 of the brick modes sits on the four-step slots, which no tile or brick kernel reads (they have no root tables), outside the six LS_OLS slots
static_assert(LS_OLS2_FN_PLIM == LS_FS_SHIFT && LS_OLS2_FN_PLIM < LS_MODE, "axis 2: fN, plim");
static_assert(LS_OLS2_NB_L == LS_FS_LO_MASK && LS_OLS2_NB_L < LS_MODE, "axis 2: nb, L");
static_assert(LS_OLS2_W0_PRE == LS_FS_GROUP && LS_OLS2_W0_PRE < LS_MODE && LS_MODE < LS_OLS_FN, "axis 2: w0, pre");
// the grouped tile launch sits on the same three slots (a tile has no axis 2 and no root tables of four-step)
static_assert(LS_TILES_CHANNELS == LS_FS_GROUP && LS_TILES_CHANNELS == LS_OLS2_W0_PRE, "grouped tiles: Cg, C");
static_assert(LS_TILES_KERNELS == LS_FS_LO_MASK && LS_TILES_KERNELS == LS_OLS2_NB_L, "grouped tiles: K, Kg");
static_assert(LS_TILES_LANE_K == LS_FS_SHIFT && LS_TILES_LANE_K == LS_OLS2_FN_PLIM && LS_TILES_LANE_K < LS_MODE, "grouped tiles: lane_k");
// The block geometry of one axis of an overlap-save launch, host side (the kernels take it as RconvOls, kern_lines.hpp, or per axis as TileAxis, kern_tiles.hpp,
// where the index map is): fN logical points cut into nb blocks, block j holding signal indices [j L - pre, j L - pre + P) and giving L results from its
// window [w0, w0 + L), signal indices kept below plim
struct OlsAxis { int64_t fN = 0, plim = 0, nb = 0, L = 0, w0 = 0, pre = 0; };
// The six LS_OLS slots of a step's i[]: each holds axis 0 in its low 32 bits and axis 1 in its high (the line modes have one axis: the value itself).
// The brick modes pass a third axis: its six values, two a slot, in the three LS_OLS2 slots, which are written for them alone
inline void ols_store(int64_t (&i)[STEP_INTS], const OlsAxis& a0, const OlsAxis& a1 = OlsAxis(), const OlsAxis* a2 = nullptr) {
  const auto both = [](int64_t v0, int64_t v1) { return (int64_t)((uint64_t)(uint32_t)v0 | ((uint64_t)(uint32_t)v1 << 32)); };
  i[LS_OLS_FN] = both(a0.fN, a1.fN); i[LS_OLS_PLIM] = both(a0.plim, a1.plim); i[LS_OLS_NB] = both(a0.nb, a1.nb);
  i[LS_OLS_L] = both(a0.L, a1.L); i[LS_OLS_W0] = both(a0.w0, a1.w0); i[LS_OLS_PRE] = both(a0.pre, a1.pre);
  if (a2) { i[LS_OLS2_FN_PLIM] = both(a2->fN, a2->plim); i[LS_OLS2_NB_L] = both(a2->nb, a2->L); i[LS_OLS2_W0_PRE] = both(a2->w0, a2->pre); }
}
inline OlsAxis ols_axis_of(const int64_t (&i)[STEP_INTS], int axis) {
  const auto half = [](int64_t v, int h) { return (int64_t)(int)(uint32_t)((uint64_t)v >> (32 * h)); };
  OlsAxis a;
  if (axis == 2) {
    a.fN = half(i[LS_OLS2_FN_PLIM], 0); a.plim = half(i[LS_OLS2_FN_PLIM], 1); a.nb = half(i[LS_OLS2_NB_L], 0); a.L = half(i[LS_OLS2_NB_L], 1);
    a.w0 = half(i[LS_OLS2_W0_PRE], 0); a.pre = half(i[LS_OLS2_W0_PRE], 1);
    return a;
  }
  a.fN = half(i[LS_OLS_FN], axis); a.plim = half(i[LS_OLS_PLIM], axis); a.nb = half(i[LS_OLS_NB], axis); a.L = half(i[LS_OLS_L], axis);
  a.w0 = half(i[LS_OLS_W0], axis); a.pre = half(i[LS_OLS_PRE], axis);
  return a;
}
enum LinesPtr {
  LP_IN = 0, LP_OUT = 1, LP_TW = 2,
  LP_TW_LO = 3, LP_MUL_SPECTRUM = 3,         // four-step / split LO roots (LM_RCONV*: LO and HI in one table); LM_MUL, LM_CONV_OLS, the tile and brick modes: the spectrum multiplied in
  LP_TW_HI = 4, LP_CHIRP = 4, LP_RCONV_SPECTRUM = 4,   // HI roots; Bluestein: the chirp; LM_RCONV*: the packed kernel spectrum
  LP_LAST = LP_RCONV_SPECTRUM
};
static_assert(LP_LAST < STEP_PTRS, "ST_LINES pointers");

// ST_XCD_FUSED / ST_XCD_RES
enum XcdSlot {
  XS_TRANSFORMS = 0, XS_N, XS_FS_SHIFT, XS_FS_LO_MASK,
  XS_TW_A_OFF, XS_TW_B_OFF, XS_TW_LO_OFF, XS_TW_HI_OFF,     // byte offsets into p[XP_TABLE]
  XS_SPLIT = 8, XS_IN_PITCH, XS_OUT_PITCH, XS_SLOTS, XS_SOLO, XS_SPIN_LIMIT,
  XS_MUL_OFF = 14, XS_CONV_K, XS_CONV_CONJ, XS_OUT_KERNEL_PITCH,   // fftconv pipeline (CONV, CONV_VIEW): spectra at p[XP_WSLOTS] + offset
  XS_V_SPLIT = 18, XS_V_SHIFT = 19,                                  // CONV_VIEW only
  XS_LAST = XS_V_SHIFT
};
static_assert(XS_LAST < STEP_INTS, "ST_XCD_* slots");
enum XcdPtr { XP_IN = 0, XP_OUT, XP_WSLOTS, XP_CTL, XP_TABLE, XP_LAST = XP_TABLE };
static_assert(XP_LAST < STEP_PTRS, "ST_XCD_* pointers");

// ST_LINES_MIXED (p: P_SRC, P_DST, P_TW)
enum MixedSlot {
  MX_LINES = 0, MX_N, MX_S, MX_T, MX_NST, MX_SWAP, MX_LDS_BYTES, MX_THREADS,
  MX_RADIX0 = 8,        // run-time plans: (radix << 32 | table offset) per stage, i[MX_RADIX0 + k]
  MX_TW_TOTAL = 19,     // table elements staged in LDS (0: read through the caches)
  MX_LAST = MX_TW_TOTAL
};
static_assert(MX_LAST < STEP_INTS, "ST_LINES_MIXED slots");

// ST_STAGE (p: P_SRC, P_DST, P_TW)
enum StageSlot { SG_TOTAL = 0, SG_N, SG_S, SG_NSP, SG_SWAP_IN, SG_SWAP_OUT, SG_LAST = SG_SWAP_OUT };
static_assert(SG_LAST < STEP_INTS, "ST_STAGE slots");

// ST_TRIG_PRE / ST_TRIG_POST (kern_trig.hpp TrigArgs).  The real-FFT kinds (>= TK_REAL) put the packed line length P and the FFT
// length M where the general kinds have L and S, and the axis stride behind the kind
enum TrigSlot { TG_LINES = 0, TG_N, TG_L = 2, TG_REAL_P = 2, TG_S = 3, TG_REAL_M = 3, TG_KIND, TG_STRIDE, TG_LAST = TG_STRIDE };
static_assert(TG_LAST < STEP_INTS, "ST_TRIG_* slots");
enum TrigPtr { TGP_X = 0, TGP_Z, TGP_Y, TGP_LAST = TGP_Y };
static_assert(TGP_LAST < STEP_PTRS, "ST_TRIG_* pointers");
// i[TG_KIND]: the table at the top of kern_trig.hpp.  The kernels there compare a.kind as a number (kind < 10, kind >= 14, kind & 1 for the
// sine kinds): the values and their order are part of the contract, a new kind goes behind the last
enum TrigKind : int {
  TK_DCT1 = 0, TK_DCT2_FWD, TK_DCT2_INV, TK_DCT4, TK_DST1, TK_DST2_FWD, TK_DST2_INV, TK_DST4,
  TK_REAL = 8,          // from here on: through a real (or half-length complex) FFT of dense or tiled lines
  TK_REAL_DCT2_FWD = 8, TK_REAL_DST2_FWD, TK_REAL_DCT2_INV, TK_REAL_DST2_INV, TK_REAL_DCT4, TK_REAL_DST4, TK_REAL_DCT1, TK_REAL_DST1
};

// ST_GATHER / ST_SCATTER (p: P_SRC, P_DST; kern_generic.hpp StridedArgs)
enum StridedSlot { GS_TOTAL = 0, GS_PER, GS_RANK, GS_PHYS_OFFSET, GS_PHYS_BATCH_STRIDE, GS_DENSE_OFFSET, GS_DENSE_BATCH_STRIDE, GS_REAL, GS_LAST = GS_REAL };
static_assert(GS_LAST < STEP_INTS, "ST_GATHER / ST_SCATTER slots");

// ST_ZERO_OUTSIDE (p: P_DATA)
enum ZeroOutsideSlot { ZO_TOTAL = 0, ZO_PER, ZO_RANK, ZO_REAL, ZO_LAST = ZO_REAL };
static_assert(ZO_LAST < STEP_INTS, "ST_ZERO_OUTSIDE slots");

// ST_FFTCONV_FUSED (kern_fftconv.hpp FusedConvArgs)
enum FusedConvSlot {
  FC_BATCH = 0, FC_K, FC_KERN_LEN, FC_CONJ, FC_IN_OFFSET, FC_IN_BATCH_STRIDE, FC_IN_STRIDE,
  FC_OUT_OFFSET, FC_OUT_KERNEL_STRIDE, FC_OUT_BATCH_STRIDE, FC_OUT_STRIDE, FC_LAST = FC_OUT_STRIDE
};
static_assert(FC_LAST < STEP_INTS, "ST_FFTCONV_FUSED slots");
enum FusedConvPtr { FCP_IN = 0, FCP_KERN, FCP_OUT, FCP_TW, FCP_LAST = FCP_TW };
static_assert(FCP_LAST < STEP_PTRS, "ST_FFTCONV_FUSED pointers");

// ST_R2C_POST / ST_C2R_PRE (p: P_SRC, P_DST, then the split roots)
enum SplitSlot { RS_H = 0, RS_BATCH, RS_LINE_STRIDE, RS_SHIFT, RS_MASK, RS_LAST = RS_MASK };
static_assert(RS_LAST < STEP_INTS, "ST_R2C_POST / ST_C2R_PRE slots");
enum SplitPtr { RSP_TW_LO = 2, RSP_TW_HI = 3, RSP_LAST = RSP_TW_HI };
static_assert(RSP_LAST < STEP_PTRS, "ST_R2C_POST / ST_C2R_PRE pointers");

// ST_PACK_HALF / ST_UNPACK_HERM (p: P_SRC, P_DST)
enum PackSlot { PH_N = 0, PH_P, PH_BATCH, PH_PACKED_STRIDE, PH_LAST = PH_PACKED_STRIDE };
static_assert(PH_LAST < STEP_INTS, "ST_PACK_HALF / ST_UNPACK_HERM slots");

// ST_POINTWISE (p: P_SRC, P_DST, PWP_KERNEL)
enum PointwiseSlot { PW_L = 0, PW_TOTAL, PW_CONJ, PW_CHANNELS, PW_ITEM_LINES, PW_LAST = PW_ITEM_LINES };   // PW_CHANNELS C > 1: out[b][i] = sum_c data[b C + c][i] (conj?)kernel[c][i] (pointwise_sum_kernel)
// PW_ITEM_LINES (fftConv.groups; 0: none): the data lines of an item, of which the PW_CHANNELS of one group are summed, PW_CHANNELS = 1 included (pointwise_group_sum_kernel)
static_assert(PW_LAST < STEP_INTS, "ST_POINTWISE slots");
enum PointwisePtr { PWP_KERNEL = 2, PWP_LAST = PWP_KERNEL };
static_assert(PWP_LAST < STEP_PTRS, "ST_POINTWISE pointers");

// ST_CHIRP_PRE / ST_CHIRP_POST (p: P_SRC, P_DST, CHP_CHIRP)
enum ChirpSlot { CH_N = 0, CH_M, CH_LINES, CH_SWAP_IN, CH_SWAP_OUT, CH_LAST = CH_SWAP_OUT };
static_assert(CH_LAST < STEP_INTS, "ST_CHIRP_* slots");
enum ChirpPtr { CHP_CHIRP = 2, CHP_LAST = CHP_CHIRP };
static_assert(CHP_LAST < STEP_PTRS, "ST_CHIRP_* pointers");

// One recorded launch, pointers still symbolic.  Scalar fields are kind-specific: the slot enums above.
struct Step {
  StepKind kind;
  int variant = 0;           // ST_LINES: registry id; ST_STAGE: radix
  PtrRef p[STEP_PTRS];       // kind-specific pointer slots
  int64_t i[STEP_INTS] = {0};     // kind-specific integers
  float f[STEP_FLOATS] = {1.0f, 1.0f}; // kind-specific floats
  int64_t shape[8] = {0}, sa[8] = {0}, sb[8] = {0};  // ST_GATHER / ST_SCATTER
  SideMap imap, omap;        // ST_LINES with i[LS_MAPPED] != 0: mapped sides (kern_lines.hpp fft_lines_mapped_kernel)
  unsigned grid = 1;
};

struct PlanIR {
  mi355fft_plan_desc desc;
  std::vector<Step> steps;
  std::vector<float2h> table;     // all twiddle tables, uploaded once at plan creation
  uint64_t work_bytes = 0;        // plan.getWorkspaceSizeBytes()
  uint64_t in_bytes = 0, out_bytes = 0, kernel_bytes = 0;  // minimum extents the exec buffers must cover
  std::string route;              // human-readable route description (plan_describe)
};

struct PlannerOptions {
  uint64_t chunk_bytes = 1ull << 30;   // two-pass: bytes of inter-pass intermediate per launch pair (measured: larger is faster)
  int compute_units = 256;
  int fuse_views = 1;                  // c2c: strided layouts / ioView / zeroPad ride the first load and last store of the line kernels where the axis route allows (0: staging passes)
  int lines_tiles_per_wg = 0;          // line kernels: 0 = resident grid (CUs x workgroups per CU) walking the tiles; k > 0 = one workgroup per k tiles
  int force_generic = 0;               // tests: route everything through the global-memory stage kernels
  int xcd_fused = 1;                   // N = N1*N2 with an XCD-fused kernel available: both passes in one persistent launch
  int xcd_shared = 1;                  // 0: no kernel whose workgroups wait for each other (shared-mode XCD kernels); solo instances stay
  unsigned xcd_spin_limit = 4000000u;  // polls before a bounded wait of the XCD kernels gives up (sticky error); tests force 1
  int line32k = 1;                     // N = 2^15 c2c lines in one workgroup (kern_line32k.hpp) instead of the solo four-step
  int trig_alt = 1;                    // one-launch DCT / DST: use the alternate ROW shapes where the registry has them (ROW_ALT_TRIG)
  int xcd_res = 0;                     // N = 2^20: XCD-resident kernel (kern_xcd_res.hpp): 1 on, 2 = its data-movement skeleton without arithmetic (measurement only)
  int xcd_res_depth = 4;               // exchange channels in flight per XCD (1, 2, 4): 1 MiB of L2-resident buffer each
  int xcd_split = 0;                   // groups per XCD in the fused kernels (1..8); 0 = chosen per plan from the workspace footprint
  int xcd_rt = 1;                      // 2048-point sides on register tiles (kern_regtile.hpp) where an instance exists (0: the LDS-resident 8-line tiles / two-pass route;
                                       // c2c 2^21 stays on the LDS-resident instance unless 2: 1024 x 2048 on register tiles, 3: 2048 x 1024 on register tiles)
  int xcd_hx = 2;                      // N = 2^20: 2 = 32-line register tiles (kern_regtile.hpp fft_xcd_rt1k_kernel; r03 default: 199 vs 194 GPoints/s), 1 = two workgroups per CU on 16-line
                                       // register tiles (fft_xcd_hx_kernel: 171), 0 = the LDS-resident fused kernel (kern_xcd.hpp)
  int xcd_2d = 1;                      // 2-D c2c planes with an instance: both axes in one fused launch
  int xcd_r2c = 1;                     // r2c: real four-step kernel where an instance exists (0: half-length c2c + split)
  int solo_cap_mb = 256;               // solo mode: all workgroups' workspace slots together (MiB) = the Infinity Cache (r02: 2^16 203 vs 189 GPoints/s with 1024; below 256 occupancy collapses)
  int solo_max_kb_2d = 1024;           // 2-D planes up to this size run in solo mode (unchanged from round 1)
  int solo_max_kb = 512;               // c2c transforms (and 2-D planes) up to this size run in solo mode; r2c up to half of it, c2r up to this many KB of REAL line
                                       // (r02, same box: c2c 2^17 shared 171 vs solo 147, r2c 2^17 281 vs 250, c2r 2^17 solo 318 vs 278, c2c 2^16 solo 206 vs 156)
  int xcd_slots = 0;                   // workspace slots per group: 0 = per route (r03: one slot and twice the groups; the 2048-point register-tile instances two), 1: two barriers per transform, 2: one barrier
  int mixed_ct = 1;                    // mixed-radix lengths with a compile-time-plan instance (kern_mixed_ct.hpp) use it (dense lines)
  int mixed_lds_kb = 0;                // experiments: LDS per workgroup of the mixed-radix line kernel (0 = per-length rule)
  int mixed_threads = 256;
  int64_t conv_fused_max_points = (int64_t)1 << 20;   // fftconv-fused (one launch, latency route) up to this many points B*N*K; above: forward-mul + inverse line launches
  int conv_pipeline = 1;               // fftconv on a 2^20-point FFT domain, dense sides: forward, products and inverses in one persistent launch (kern_regtile.hpp fft_xcd_conv1m_kernel;
                                       // the linear modes and zeroPad through its VIEW form); 0: the composed route
  int conv_pad = 1;                    // fftconv, rank 1, linear modes with 16384 < shape + kernelShape - 1 <= 2^22: transform on the next power of two (0: the exact length)
#ifdef MI355_HOST_EMU
  // the emulation harness builds its options without planner_options_from_env(): the switch's emulation twin is read here
  int rconv_fused = std::getenv("MI355_EMU_RCONV_FUSED") ? std::atoi(std::getenv("MI355_EMU_RCONV_FUSED")) : 1;
#else
  int rconv_fused = 1;
#endif
                                       // real fftconv (MI355FFT_FFTCONV_REAL), rank 1, power-of-two FFT length 128..8192 (16384, 32768: strided sides only): r2c, product and c2r of a
                                       // line in one launch per kernel (kern_lines.hpp fft_lines_rconv_kernel); 0: the composed route rconv[K]; 2: the line route up to 32768 as well
#ifdef MI355_HOST_EMU
  int rconv_ols = std::getenv("MI355_EMU_RCONV_OLS") ? std::atoi(std::getenv("MI355_EMU_RCONV_OLS")) : 1;
#else
  int rconv_ols = 1;
#endif
                                       // real fftconv, rank 1, linear boundaries: overlap-save on blocks of P points, one launch per kernel whatever the line's length
                                       // (kern_lines.hpp fft_lines_rconv_ols_kernel); 1: where measured ahead (plan.cpp build_fftconv_real); 0: never; a power of two
                                       // 128..8192: that block length on every request it fits (tests and measurement).  rconv_fused = 0 / 2 come first
#ifdef MI355_HOST_EMU
  int conv_ols = std::getenv("MI355_EMU_CONV_OLS") ? std::atoi(std::getenv("MI355_EMU_CONV_OLS")) : 1;
#else
  int conv_ols = 1;
#endif
                                       // fftconv, rank 1, linear boundaries: overlap-save on blocks of P complex points, one launch per kernel whatever the line's length
                                       // (kern_lines.hpp fft_lines_conv_ols_kernel); 1: where measured ahead (plan.cpp build_fftconv); 0: never; a power of two
                                       // 128..4096: that block length on every request it fits (tests and measurement).  conv_lines = 0 and force_generic come first
#ifdef MI355_HOST_EMU
  int conv_ols2d = std::getenv("MI355_EMU_CONV_OLS2D") ? std::atoi(std::getenv("MI355_EMU_CONV_OLS2D")) : 1;
#else
  int conv_ols2d = 1;
#endif
                                       // fftconv, rank 2, linear boundaries: overlap-save on P x P complex tiles, one launch per kernel whatever the image's size
                                       // (kern_tiles.hpp fft_tiles_conv_ols_kernel); 1: where measured ahead (plan.cpp conv_tiles_block); 0: never; 64 or 128: that
                                       // tile on every request it fits (tests and measurement).  conv_lines = 0 and force_generic come first
#ifdef MI355_HOST_EMU
  int rconv_ols2d = std::getenv("MI355_EMU_RCONV_OLS2D") ? std::atoi(std::getenv("MI355_EMU_RCONV_OLS2D")) : 1;
#else
  int rconv_ols2d = 1;
#endif
                                       // real fftconv, rank 2, linear boundaries: overlap-save on P x P tiles, two real tiles as re / im of a complex one, one launch
                                       // per kernel whatever the image's size (kern_tiles.hpp fft_tiles_conv_ols_kernel on an RTileCfg); 1: where measured ahead (plan.cpp
                                       // rconv_tiles_block); 0: never; 64 or 128: that tile on every request it fits (tests and measurement).  rconv_fused = 0 and
                                       // force_generic come first
#ifdef MI355_HOST_EMU
  int sum_ols2d = std::getenv("MI355_EMU_SUM_OLS2D") ? std::atoi(std::getenv("MI355_EMU_SUM_OLS2D")) : 1;
#else
  int sum_ols2d = 1;
#endif
                                       // fftconv / real fftconv with fftConv.inputChannels > 1, rank 2, linear boundaries: the sum form of the tile kernel, one launch per
                                       // OUTPUT kernel (kern_tiles.hpp on an STileCfg / SRTileCfg); 1: where measured ahead (plan.cpp sum_tiles_block); 0: the composed
                                       // routes fftconv-sum / rconv-sum; 64 or 128: that tile on every request it fits and an instance exists for (tests and measurement).
                                       // conv_ols2d / rconv_ols2d = 0 and the switches in front of them come first
#ifdef MI355_HOST_EMU
  int group_ols2d = std::getenv("MI355_EMU_GROUP_OLS2D") ? std::atoi(std::getenv("MI355_EMU_GROUP_OLS2D")) : 1;
#else
  int group_ols2d = 1;
#endif
                                       // fftconv / real fftconv with fftConv.groups > 1, rank 2, linear boundaries: the grouped tile kernel, every output kernel in one
                                       // launch (kern_tiles.hpp fft_tiles_conv_ols_group_kernel); 1: where measured ahead (plan.cpp group_tiles_block); 0: never (depthwise
                                       // requests take the single-channel overlap-save routes through a per-kernel load map, the rest the composed routes); 64: that tile
                                       // on every request it fits; any other value: never.  conv_ols2d / rconv_ols2d = 0 and the switches in front of them come first
#ifdef MI355_HOST_EMU
  int conv_ols3d = std::getenv("MI355_EMU_CONV_OLS3D") ? std::atoi(std::getenv("MI355_EMU_CONV_OLS3D")) : 1;
  int rconv_ols3d = std::getenv("MI355_EMU_RCONV_OLS3D") ? std::atoi(std::getenv("MI355_EMU_RCONV_OLS3D")) : 1;
#else
  int conv_ols3d = 1, rconv_ols3d = 1;
#endif
                                       // fftconv / real fftconv, rank 3, linear boundaries: overlap-save on 16^3 complex bricks (real: two real bricks as re / im of one),
                                       // one launch per kernel whatever the volume's size (kern_bricks.hpp fft_bricks_conv_ols_kernel); 1: where measured ahead (plan.cpp
                                       // conv_bricks_block, rconv_bricks_block); 0: never; 16: the brick on every request it fits (tests and measurement).  conv_lines = 0
                                       // and force_generic (complex), rconv_fused = 0 and force_generic (real) come first
#ifdef MI355_HOST_EMU
  int ols_circular = std::getenv("MI355_EMU_OLS_CIRCULAR") ? std::atoi(std::getenv("MI355_EMU_OLS_CIRCULAR")) : 1;
#else
  int ols_circular = 1;
#endif
                                       // fftconv / real fftconv, circular boundary: the wrapping form of the overlap-save routes above (block sizes and kernel bounds of their rules,
                                       // shape[a] >= 2 P on every axis); 1: where measured ahead (plan.cpp ols_circular_block); 0: never; 2: every request inside those bounds,
                                       // power-of-two domains included (tests and measurement).  A route's own switch at 0 and the switches in front of it turn its circular form off too
  int conv_lines = 1;                  // fftconv: kernel-spectrum product fused behind the forward line FFT (1-D, power-of-two FFT length <= max_line)
  int trig_fused = 1;                  // dct2 / dst2 of dense lines (half length a line-kernel size): permutation + real FFT + phase in one launch
  int trig_real = 1;                   // dct2/dst2/dct3/dst3 along a dense even axis through a real FFT of length N (kern_trig.hpp)
  int lines_c2r = 1;                   // c2r twin (pre-split from global into LDS before the first stage): half lengths <= 16384 (3: <= 8192, the round-1 choice)
                                       // (N = 256: 528 vs 133 G real points/s, 1024: 471 vs 243, 2^14: 312 vs 270); 2 forces it at 2^15 too
  int lines_r2c = 1;                   // r2c with a half length of 64..max_line: split fused into the line kernel
  int max_line = 16384;                // longest power-of-two line given to a single workgroup (4096: N = 8192, 16384 take the four-step routes)
  int mixed_lines = 1;                 // mixed-radix lengths <= 4096: one LDS line kernel instead of one global pass per radix
  int only_pass = 0;                   // measurement aid (bench.py per-kernel timing): 1 = emit pass A only, 2 = pass B only
};
PlannerOptions planner_options_from_env();

// returns MI355FFT_OK or an error status with `err` filled (message style follows the reference's throws)
int build_plan(const mi355fft_plan_desc& desc, const PlannerOptions& opt, PlanIR& out, std::string& err);

// An out-of-place c2c plan may be run with output and input in one buffer (exec exempts c2c from "different buffers"); in_off / out_off are
// the two ranges' byte offsets in it.  What such an exec does:
//   ALIAS_AS_IS    the plan's own steps.  Disjoint ranges; strided layouts (the element sets are the caller's: lanes of one tensor); dense
//                  sides on ONE range (same offset): every dense route reads a line, tile or transform whole before it stores it to the
//                  same addresses, or goes through the workspace (tests/exec_contract_cases.py runs each route that way)
//   ALIAS_STAGED   ioView on overlapping ranges: the view sides differ in shape, and the mapped launches clear and store the output view
//                  while input elements are still unread.  The same request planned with fuse_views = 0 runs instead: its input side is
//                  staged into the workspace before the first store to the output
//   ALIAS_REFUSED  dense sides on ranges that overlap at different offsets: `err` says why
enum AliasVariant { ALIAS_AS_IS = 0, ALIAS_STAGED = 2, ALIAS_REFUSED = -1 };
AliasVariant alias_variant(const PlanIR& ir, uint64_t in_off, uint64_t out_off, std::string& err);

// radix factorisation of the generic route: greedy largest-first over {32,16,8,4,2,13,11,7,5,3}
// (superset of src/plan.js:20-33's {13,11,8,7,5,4,3,2}); empty when n has another prime factor
std::vector<int> factorize_radices(int64_t n, int max_radix = 32);

// e^{-2 pi i m / M} rounded to f32 from an 80-bit evaluation
float2h root_of_unity(int64_t m, int64_t M);

}  // namespace mi355
