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

// One recorded launch, pointers still symbolic.  Scalar fields are kind-specific (see dispatch.hpp).
struct Step {
  StepKind kind;
  int variant = 0;           // ST_LINES: registry id; ST_STAGE: radix
  PtrRef p[5];               // kind-specific pointer slots
  int64_t i[20] = {0};     // kind-specific integers
  float f[2] = {1.0f, 1.0f}; // kind-specific floats
  int64_t shape[8] = {0}, sa[8] = {0}, sb[8] = {0};  // ST_GATHER / ST_SCATTER
  SideMap imap, omap;        // ST_LINES with i[10] != 0: mapped sides (kern_lines.hpp fft_lines_mapped_kernel)
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
