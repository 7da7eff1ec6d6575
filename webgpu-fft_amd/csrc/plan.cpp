// plan.cpp — see plan.hpp.  Pure host C++ (no HIP).
#include "plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace mi355 {

// ---- registry --------------------------------------------------------------------------------------
namespace {
constexpr int cmax3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
constexpr int ilog2c(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }

LineKernelMeta make_meta(int id, int N, int R0, int R1, int R2, int T, bool ic, bool oc, bool si, bool so, int twid) {
  // mirrors LineCfg in kern_lines.hpp (checked against the device constants by tests/emu and at library load)
  LineKernelMeta m{};
  m.id = id; m.N = N; m.R0 = R0; m.R1 = R1; m.R2 = R2; m.T = T;
  m.in_col = ic; m.out_col = oc; m.swap_in = si; m.swap_out = so; m.twid = twid;
  const int nst = R1 == 1 ? 1 : (R2 == 1 ? 2 : 3);
  const int rmax = cmax3(R0, R1, R2);
  const int tpl = N / rmax;
  m.threads = T * tpl;
  const bool idx_major = ic && oc;
  const int padsh = ilog2c(R0);
  const int pitch_raw = N + (N >> padsh);
  const int pmod = (!ic && oc && T <= 32) ? 32 / T : 2;
  const int pitch = ((pitch_raw + 31) / 32) * 32 + pmod;
  const int data = nst == 1 ? 0 : (idx_major ? N * T : T * pitch);
  const int tw1 = nst >= 2 ? (R1 - 1) * R0 : 0;
  const int tw2 = nst == 3 ? (R2 - 1) * R0 * R1 : 0;
  m.tw_elems = tw1 + tw2;
  const int lo = twid == 1 ? 1024 : 0;
  const int tw_lds = tw1 + (tw2 * 8 <= (twid == 4 ? 8 * 1024 : MI355_TW2_LDS_MAX) ? tw2 : 0);        // LineCfg::TW2_IN_LDS
  m.lds_bytes = (data + tw_lds + lo) * 8;
  return m;
}
}  // namespace

const std::vector<LineKernelMeta>& line_kernel_registry() {
  static const std::vector<LineKernelMeta> reg = [] {
    std::vector<LineKernelMeta> r;
    int id = 0;
#define LINE_ROW(N, R0, R1, R2, T)                                             \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, false, false, false, false, 0)); \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, false, false, true, true, 0));
#define LINE_ROW_TRIG(N, R0, R1, R2, T)                                        \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, false, false, false, false, 4));
#define LINE_PASS_A(N, R0, R1, R2, T)                                        \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, true, true, false, false, 0)); \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, true, true, true, false, 0));  \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, true, true, true, true, 0));
#define LINE_PASS_B(N, R0, R1, R2, T)                                         \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, false, true, false, false, 2)); \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, false, true, false, true, 2));
#define LINE_COL_RAGGED(N, R0, R1, R2, T)                                    \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, true, true, false, false, 3)); \
  r.push_back(make_meta(id++, N, R0, R1, R2, T, true, true, true, true, 3));
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
    return r;
  }();
  return reg;
}

const LineKernelMeta* find_line_kernel(int N, bool in_col, bool out_col, bool swap_in, bool swap_out, int twid) {
  for (const auto& m : line_kernel_registry())
    if (m.N == N && m.in_col == in_col && m.out_col == out_col && m.swap_in == swap_in && m.swap_out == swap_out && m.twid == twid)
      return &m;
  return nullptr;
}

const std::vector<ConvKernelMeta>& conv_kernel_registry() {
  static const std::vector<ConvKernelMeta> reg = [] {
    std::vector<ConvKernelMeta> r;
    int id = 0;
#define X(N, R0, R1, TL) r.push_back(ConvKernelMeta{id++, N, R0, R1, TL});
    MI355_CONV_KERNEL_LIST(X)
#undef X
    return r;
  }();
  return reg;
}

const TileKernelMeta* find_tile_kernel(int P, bool real, bool sum, int group) {
  static const std::vector<TileKernelMeta> reg = [] {
    std::vector<TileKernelMeta> r;
    for (int real = 0; real < 2; ++real) {   // both forms instantiate the whole list: an id is the position in it
      int id = 0;
#define X(P, R0, R1, TH) r.push_back(TileKernelMeta{id++, P, R0, R1, TH, tile_kernel_lds_bytes(P, R0, R1), real != 0, false});
      MI355_TILE_KERNEL_LIST(X)
#undef X
      id = 0;                                // the sum forms: ids of their own list
#define X(P, R0, R1, TH) r.push_back(TileKernelMeta{id++, P, R0, R1, TH, tile_kernel_lds_bytes(P, R0, R1), real != 0, true});
      MI355_TILE_SUM_KERNEL_LIST(X)
#undef X
      id = 0;                                // the grouped forms: ids of their own list
#define X(P, R0, R1, TH, DW) r.push_back(TileKernelMeta{id++, P, R0, R1, TH, tile_kernel_lds_bytes(P, R0, R1), real != 0, DW == 0, DW ? 2 : 1});
      MI355_TILE_GROUP_KERNEL_LIST(X)
#undef X
    }
    return r;
  }();
  for (const auto& m : reg) if (m.P == P && m.real == real && m.sum == sum && m.group == group) return &m;
  return nullptr;
}

const BrickKernelMeta* find_brick_kernel(int P, bool real) {
  static const std::vector<BrickKernelMeta> reg = [] {
    std::vector<BrickKernelMeta> r;
    for (int real = 0; real < 2; ++real) {   // both forms instantiate the whole list: an id is the position in it
      int id = 0;
#define X(P, TH) r.push_back(BrickKernelMeta{id++, P, TH, brick_kernel_lds_bytes(P), real != 0});
      MI355_BRICK_KERNEL_LIST(X)
#undef X
    }
    return r;
  }();
  for (const auto& m : reg) if (m.P == P && m.real == real) return &m;
  return nullptr;
}

namespace {
// launch shape of an XCD-fused instance: host copies of the Cfg constants its case in dispatch.hpp launches with (kern_xcd.hpp
// XcdFusedCfg, kern_regtile.hpp), checked against them by tests/emu (emu_check_xcd_registry)
XcdKernelMeta xcd_meta(int id, const XcdInstance& k) {
  XcdKernelMeta m{k, id, 0, 0};
  constexpr int RT_HALF = 16 * 32 * 32, RT_TW2 = 31 * 64, TW1_1K = 31 * 32;   // RtCfg::HALF_ELEMS, RtCfg::TW2_ELEMS, Rt1kCfgT::TW1_ELEMS
  if (k.kind <= XK_VIEW) {   // XcdFusedCfg: the larger of the two passes' tiles + their stage tables (one copy if the passes are the same)
    const LineKernelMeta ma = make_meta(0, k.N1, k.ra[0], k.ra[1], k.ra[2], k.ta, true, true, k.inverse, false, 0);
    const LineKernelMeta mb = make_meta(0, k.N2, k.rb[0], k.rb[1], k.rb[2], k.tb, false, k.kind != XK_TWO_D, false, k.inverse, 0);
    const int da = ma.lds_bytes - ma.tw_elems * 8, db = mb.lds_bytes - mb.tw_elems * 8;
    const bool shared = k.N1 == k.N2 && k.ra[0] == k.rb[0] && k.ra[1] == k.rb[1] && k.ra[2] == k.rb[2];
    m.threads = ma.threads;
    m.lds_bytes = std::max(da, db) + (ma.tw_elems + (shared ? 0 : mb.tw_elems)) * 8 + 64;
  } else if (k.kind == XK_RT || k.kind == XK_RT_R2C || k.kind == XK_RT_C2R) {   // XcdRtCfg: max(pass A's LDS tile, one exchange half) + tables
    const bool a_rt = k.N1 == 2048;   // (2048-point pass A on register tiles too: no LDS tile, no line table)
    const LineKernelMeta ma = make_meta(0, a_rt ? 1024 : k.N1, 32, (a_rt ? 1024 : k.N1) / 32, 1, 16, true, true, k.inverse, false, 0);
    m.threads = 512;
    m.lds_bytes = std::max(a_rt ? 0 : ma.lds_bytes - ma.tw_elems * 8, RT_HALF * 8) + (a_rt ? 0 : ma.tw_elems * 8) + RT_TW2 * 8 + 64;
  } else if (k.kind == XK_HX) {   // HxCfg: 16-line tiles, 512 threads
    m.threads = 512;
    m.lds_bytes = (16 * 32 * 16 + TW1_1K) * 8 + 64;
  } else {   // Rt1kCfgT<Tb>: Tb-line tiles, 16 Tb threads; 2048 x 1024 adds the stage-2 roots of its 2048-point columns, the plain 32-line 1024 x 1024 instances the four-step tables
    m.threads = 16 * k.tb;
    m.lds_bytes = (k.tb * 32 * 16 + TW1_1K + (k.N1 == 2048 ? RT_TW2 : 0) + (k.kind == XK_CONV || k.kind == XK_CONV_VIEW ? 0 : rt1k_root_lds_elems(k.tb, k.kind == XK_RT1K_VIEW, k.N1))) * 8 + 64;
  }
  return m;
}
}  // namespace

const std::vector<XcdKernelMeta>& xcd_kernel_registry() {
  static const std::vector<XcdKernelMeta> reg = [] {
    std::vector<XcdKernelMeta> r;
    for (const XcdInstance& k : XCD_INSTANCES) r.push_back(xcd_meta((int)r.size(), k));
    return r;
  }();
  return reg;
}

PlannerOptions planner_options_from_env() {
  PlannerOptions o;
  if (const char* s = std::getenv("MI355FFT_CHUNK_BYTES")) { const int64_t v = std::atoll(s); if (v > 0) o.chunk_bytes = (uint64_t)v; }
  if (const char* s = std::getenv("MI355FFT_FORCE_GENERIC")) o.force_generic = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_MIXED_LINES")) o.mixed_lines = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_MIXED_CT")) o.mixed_ct = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_LINES_R2C")) o.lines_r2c = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_LINES_C2R")) o.lines_c2r = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_TRIG_REAL")) o.trig_real = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_TRIG_FUSED")) o.trig_fused = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_CONV_LINES")) o.conv_lines = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_CONV_FUSED_MAX_POINTS")) { const long long v = std::atoll(s); if (v >= 0) o.conv_fused_max_points = v; }
  if (const char* s = std::getenv("MI355FFT_MAX_LINE")) { const int v = std::atoi(s); if (v >= 4096) o.max_line = v; }
  if (const char* s = std::getenv("MI355FFT_MIXED_LDS_KB")) { const int v = std::atoi(s); if (v >= 8 && v <= 128) o.mixed_lds_kb = v; }
  if (const char* s = std::getenv("MI355FFT_MIXED_THREADS")) { const int v = std::atoi(s); if (v >= 64 && v <= 512 && v % 64 == 0) o.mixed_threads = v; }
  if (const char* s = std::getenv("MI355FFT_ONLY_PASS")) o.only_pass = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_FUSE_VIEWS")) o.fuse_views = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_LINES_TILES_PER_WG")) { const int v = std::atoi(s); if (v >= -1) o.lines_tiles_per_wg = v; }
  if (const char* s = std::getenv("MI355FFT_XCD_FUSED")) o.xcd_fused = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_TRIG_ALT")) o.trig_alt = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_LINE32K")) o.line32k = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_XCD_RES")) o.xcd_res = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_XCD_SPIN_LIMIT")) { const long long v = std::atoll(s); if (v >= 1 && v <= 0x7fffffffll) o.xcd_spin_limit = (unsigned)v; }
  if (const char* s = std::getenv("MI355FFT_XCD_RES_DEPTH")) { const int v = std::atoi(s); if (v == 1 || v == 2 || v == 4) o.xcd_res_depth = v; }
  if (const char* s = std::getenv("MI355FFT_XCD_SPLIT")) { const int v = std::atoi(s); if (v >= 0 && v <= 32) o.xcd_split = v; }
  if (const char* s = std::getenv("MI355FFT_XCD_R2C")) o.xcd_r2c = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_XCD_2D")) o.xcd_2d = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_XCD_RT")) o.xcd_rt = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_XCD_HX")) o.xcd_hx = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_CONV_PIPELINE")) o.conv_pipeline = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_CONV_PAD")) o.conv_pad = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_RCONV_FUSED")) o.rconv_fused = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_RCONV_OLS")) o.rconv_ols = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_CONV_OLS")) o.conv_ols = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_CONV_OLS2D")) o.conv_ols2d = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_RCONV_OLS2D")) o.rconv_ols2d = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_SUM_OLS2D")) o.sum_ols2d = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_GROUP_OLS2D")) o.group_ols2d = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_CONV_OLS3D")) o.conv_ols3d = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_RCONV_OLS3D")) o.rconv_ols3d = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_OLS_CIRCULAR")) o.ols_circular = std::atoi(s);
  if (const char* s = std::getenv("MI355FFT_SOLO_MAX_KB")) { const int v = std::atoi(s); if (v >= 0) o.solo_max_kb = v; }
  if (const char* s = std::getenv("MI355FFT_SOLO_CAP_MB")) { const int v = std::atoi(s); if (v >= 1) o.solo_cap_mb = v; }
  if (const char* s = std::getenv("MI355FFT_XCD_SLOTS")) { const int v = std::atoi(s); if (v >= 0 && v <= 2) o.xcd_slots = v; }
  return o;
}

const std::vector<MixedCtMeta>& mixedct_registry() {
  static const std::vector<MixedCtMeta> reg = [] {
    std::vector<MixedCtMeta> r;
    int id = 0;
#define X(N_, T_, TH_, ...) { MixedCtMeta m; m.id = id++; m.N = N_; m.T = T_; m.threads = TH_; m.radices = std::vector<int>{__VA_ARGS__}; \
    int tw = 0, nsp = 1; for (int R : m.radices) { tw += R * nsp; nsp *= R; } m.lds_bytes = (2 * T_ * (N_ + (N_ >> 5) + 1) + tw) * 8; r.push_back(m); }
    MI355_MIXEDCT_LIST(X)
#undef X
    return r;
  }();
  return reg;
}

// max_radix < 32: the one-launch mixed-radix kernel keeps a line in LDS, where a stage is cheap but its parallelism is
// N / radix butterflies per line — radices above 8 starve the workgroup (measured: N = 640 as 32*4*5 30 GPoints/s)
std::vector<int> factorize_radices(int64_t n, int max_radix) {
  static const int allowed[] = {32, 16, 8, 4, 2, 13, 11, 7, 5, 3};
  std::vector<int> out;
  for (int r : allowed) {
    if (r > max_radix && (r & (r - 1)) == 0) continue;
    while (n % r == 0 && n > 1) { out.push_back(r); n /= r; }
  }
  if (n != 1) out.clear();
  return out;
}
float2h root_of_unity(int64_t m, int64_t M) {
  m %= M;
  if (m < 0) m += M;
  const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)M;
  float2h r;
  r.x = (float)cosl(ang);
  r.y = (float)sinl(ang);
  // exact values on the axes (cosl(pi/2) is ~1e-20, harmless, but keep tables clean)
  if (4 * m == M) { r.x = 0.0f; r.y = -1.0f; }
  if (2 * m == M) { r.x = -1.0f; r.y = 0.0f; }
  if (4 * m == 3 * M) { r.x = 0.0f; r.y = 1.0f; }
  if (m == 0) { r.x = 1.0f; r.y = 0.0f; }
  return r;
}

// ---- builder ---------------------------------------------------------------------------------------
namespace {

bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }
int lg2(int64_t n) { int l = 0; while (((int64_t)1 << l) < n) ++l; return l; }
int64_t prodv(const int64_t* s, int rank) { int64_t p = 1; for (int d = 0; d < rank; ++d) p *= s[d]; return p; }
uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

struct Builder {
  PlanIR& ir;
  const PlannerOptions& opt;
  uint64_t work_top = 0;
  // rank-1 lane layouts on the four-step sizes (build_c2c): the pitches between consecutive lines that the fused kernel of the next
  // emit_axis should use instead of N; lane_used reports that a fused launch took them (any other route ignores them)
  int64_t lane_in_pitch = 0, lane_out_pitch = 0;
  bool lane_used = false;
  Builder(PlanIR& i, const PlannerOptions& o) : ir(i), opt(o) {}

  PtrRef alloc_work(uint64_t bytes) {
    PtrRef r(BUF_WORK, (int64_t)work_top);
    work_top = align_up(work_top + bytes, 256);
    if (work_top > ir.work_bytes) ir.work_bytes = work_top;
    return r;
  }
  PtrRef add_table(const std::vector<float2h>& t) {
    // 256-byte aligned start so LDS staging loads stay aligned
    while ((ir.table.size() * sizeof(float2h)) % 256 != 0) ir.table.push_back(float2h{0, 0});
    PtrRef r(BUF_TABLE, (int64_t)(ir.table.size() * sizeof(float2h)));
    ir.table.insert(ir.table.end(), t.begin(), t.end());
    return r;
  }
  // element-wise kernels (grid-stride loops of 256 threads): one element per thread.  Round 1 capped the grid at 16 workgroups per
  // CU; one-shot grids stream 15-20 % faster on this chip (profiles/r02_copy_ceiling.log), so the cap is only an overflow guard.
  // HIP refuses a launch whose grid x block reaches 2^32 threads: every kernel here walks its items with a grid-stride loop, so
  // grids are capped well below that for workgroups of up to 1024 threads
  static constexpr int64_t MAX_BLOCKS = ((int64_t)1 << 22) - 1;
  unsigned generic_grid(int64_t total) const {
    const int64_t blocks = (total + 255) / 256;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, MAX_BLOCKS));
  }
  // streaming kernels whose work items are independent chunks: one short-lived workgroup per item.  One-shot grids stream at
  // 6.2-6.5 TB/s on this chip where resident grid-stride loops reach 5.3-5.5 (profiles/r02_copy_ceiling.log)
  // work items of r2c_post_kernel / c2r_pre_kernel (kern_generic.hpp): 512 bin pairs each; lines of at most 256 pairs sit side by side
  static int64_t split_items(int64_t lines, int64_t H) {
    const int64_t pairs = H / 4 + 1;
    if (pairs > 256) return lines * ((pairs + 511) / 512);
    int sh = 0;
    while (((int64_t)1 << sh) < pairs) ++sh;
    const int64_t per_item = 2 * (256 >> sh);
    return (lines + per_item - 1) / per_item;
  }
  unsigned oneshot_grid(int64_t items) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(items, MAX_BLOCKS)); }
  Step& push(StepKind k) { ir.steps.emplace_back(); ir.steps.back().kind = k; return ir.steps.back(); }
  // clears `scalars` 32-bit words at ptr
  Step& zero(PtrRef ptr, int64_t scalars) { Step& z = push(ST_ZERO); z.p[P_DATA] = ptr; z.i[S_COUNT] = scalars; z.grid = generic_grid(scalars); return z; }

  // stage-2 roots of the register-tile passes (kern_regtile.hpp): e^{-2 pi i q2 j2/2048}, rows q2 = 1..31, j2 = 0..63 fastest
  PtrRef regtile_table() {
    std::vector<float2h> t((size_t)31 * 64);
    for (int q = 1; q < 32; ++q) for (int j = 0; j < 64; ++j) t[(size_t)(q - 1) * 64 + j] = root_of_unity((int64_t)q * j, 2048);
    return add_table(t);
  }
  // stage tables of a line kernel: stage 1 [R1-1][R0] roots of order R0*R1, stage 2 [R2-1][R0*R1] of order N
  PtrRef line_tables(const LineKernelMeta& m) {
    std::vector<float2h> t;
    if (m.R1 > 1) {
      const int64_t ns = (int64_t)m.R0 * m.R1;
      for (int q = 1; q < m.R1; ++q) for (int k = 0; k < m.R0; ++k) t.push_back(root_of_unity((int64_t)q * k, ns));
    }
    if (m.R2 > 1) {
      const int64_t nsp = (int64_t)m.R0 * m.R1;
      for (int q = 1; q < m.R2; ++q) for (int64_t k = 0; k < nsp; ++k) t.push_back(root_of_unity(q * k, m.N));
    }
    if (t.empty()) t.push_back(float2h{1, 0});
    return add_table(t);
  }

  // e^{-2 pi i k/M} for k < count as HI[k >> 10] * LO[k & 1023]: tables into slots p[RSP_TW_LO], p[RSP_TW_HI], i[RS_SHIFT], i[RS_MASK]
  void split_roots(Step& st, int64_t M, int64_t count) {
    std::vector<float2h> lo(1024), hi((size_t)((count + 1023) >> 10));
    for (int64_t l = 0; l < 1024; ++l) lo[(size_t)l] = root_of_unity(l, M);
    for (size_t h = 0; h < hi.size(); ++h) hi[h] = root_of_unity((int64_t)h << 10, M);
    const PtrRef plo = add_table(lo), phi = add_table(hi);   // add_table may reallocate ir.steps? no: tables live in ir.table
    st.p[RSP_TW_LO] = plo; st.p[RSP_TW_HI] = phi; st.i[RS_SHIFT] = 10; st.i[RS_MASK] = 1023;
  }

  // the real fftconv line kernels' roots e^{-2 pi i k/P} = HI[k >> 10] LO[k & 1023], k <= P/2: the HI factors directly behind the 1024 LO factors
  // (one table: dispatch.hpp)
  PtrRef rconv_roots(int64_t P) {
    std::vector<float2h> roots(1024 + (size_t)std::max<int64_t>(1, (P / 2 + 1023) >> 10));
    for (int64_t l = 0; l < 1024; ++l) roots[(size_t)l] = root_of_unity(l, P);
    for (size_t h = 1024; h < roots.size(); ++h) roots[h] = root_of_unity((int64_t)(h - 1024) << 10, P);
    return add_table(roots);
  }

  unsigned lines_grid(const LineKernelMeta& m, int64_t tiles, bool plain_c2c = false) const {
    int64_t per_cu = 8;
    if (m.lds_bytes > 0) per_cu = std::min<int64_t>(per_cu, (160 * 1024) / m.lds_bytes);
    per_cu = std::min<int64_t>(per_cu, 2048 / m.threads);
    per_cu = std::max<int64_t>(per_cu, 1);
    // lines_tiles_per_wg > 0: a short-lived workgroup per `lines_tiles_per_wg` tiles instead of a resident grid walking the batch
    // (one-shot grids stream at 6.2-6.5 TB/s where persistent loops reach 5.3-5.5: profiles/r02_copy_ceiling.log)
    // default (0): ROW kernels of up to 1024 points take one tile per workgroup (measured +10...+14 % at N = 64..512, +6 % at 1024:
    // profiles/r02_oneshot_grids.log); longer lines would re-stage tables of a quarter of a tile or more per workgroup and the
    // PASS kernels hoist per-launch state, so they stay resident.  -1 keeps every line kernel resident.
    int tpw = opt.lines_tiles_per_wg;
    if (tpw == 0 && plain_c2c && !m.in_col && !m.out_col && m.twid == 0 && m.N <= 1024) tpw = 1;   // (the r2c / c2r / product variants measured better resident)
    if (tpw > 0) return (unsigned)std::max<int64_t>(1, std::min<int64_t>((tiles + tpw - 1) / tpw, MAX_BLOCKS));
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, per_cu * opt.compute_units));
  }
  // One ST_LINES launch of kernel `m` over `lines` lines with its own stage tables: each side as (S, outer stride), LM_C2C, dense.  `oneshot`:
  // a plain c2c launch that may take lines_grid's one-shot grid.  `tiles` where it is not lines / T rounded up (exact column tiles, per-group
  // tiles on COL_RAGGED).  The caller adds the slots of its mode.
  struct LineSide { int64_t S, outer; };
  Step& push_lines(const LineKernelMeta& m, PtrRef src, PtrRef dst, int64_t lines, LineSide in, LineSide out, float scale, bool oneshot = false, int64_t tiles = -1) {
    Step& st = push(ST_LINES);
    st.variant = m.id;
    st.p[LP_IN] = src; st.p[LP_OUT] = dst; st.p[LP_TW] = line_tables(m);
    if (tiles < 0) tiles = (lines + m.T - 1) / m.T;
    st.i[LS_TILES] = tiles; st.i[LS_LINES] = lines; st.i[LS_IN_S] = in.S; st.i[LS_IN_OUTER] = in.outer; st.i[LS_OUT_S] = out.S; st.i[LS_OUT_OUTER] = out.outer;
    st.f[F_SCALE] = scale;
    st.grid = lines_grid(m, tiles, oneshot);
    return st;
  }

  // batched 1-D FFT along an axis of a dense array: `lines` = S*outer lines of length N, element stride S.
  //   src/dst may be the same location.  inverse => e^{+...}.  scale fused into the last launch.
  // groups per XCD for the fused kernels.  Measured (profiles/r01_xcd_fused_ab.log): more, smaller groups are better as long
  // as all their workspace slots together stay within the 256 MiB Infinity Cache (8 XCDs x split x slots x slot bytes)
  // r03 (profiles/r03_headline_rt32_ab.log): at EQUAL footprint, twice the groups with ONE slot each (two barriers per transform) beat
  // half the groups with two slots (one barrier): c2c 2^20 184 -> 194 (LDS-resident kernel), 2^17 179 -> 192, r2c 2^21 216 -> 245,
  // c2r 2^20 289 -> 300.  So: one slot per group, and as many groups per XCD (a power of two, at most 16) as keep all slots of the chip
  // within the 256 MiB Infinity Cache.  The 2048-point register-tile instances keep two slots (their single group per XCD measured
  // the same either way).  MI355FFT_XCD_SPLIT / MI355FFT_XCD_SLOTS override.
  void xcd_groups(const XcdKernelMeta& xm, uint64_t slot_bytes, int64_t& split, int64_t& slots) const {
    const bool two_slot_default = xm.kind == XK_RT;
    slots = opt.xcd_slots > 0 ? opt.xcd_slots : (two_slot_default ? 2 : 1);
    if (opt.xcd_split > 0) { split = opt.xcd_split; return; }
    // 2048 x 2048 real transforms: two groups per XCD with one slot each (8 x 2 x 16.8 MB, a little over the Infinity Cache) measured
    // ahead of one group with two slots on three of four boxes (r2c 288 vs 279, 282 vs 270, 269 vs 264, 232 vs 238: profiles/r03_regtile_ab.log)
    if ((xm.kind == XK_RT_R2C || xm.kind == XK_RT_C2R) && xm.N1 == 2048 && opt.xcd_slots <= 0) { split = 2; return; }
    // fftconv pipeline, groups per XCD x data lines per round (two slots per line, W and W2), same box, GPoints/s (profiles/r03_fftconv_pipeline_ab.log):
    // 2 x 1 101-104 (8 x 2 x 2 x 8 MiB = the Infinity Cache), 1 x 2 95-97, 2 x 2 92-96, 1 x 1 87-89, 4 x 1 68; three launches 70-73
    if (xm.kind == XK_CONV || xm.kind == XK_CONV_VIEW) { split = 2; return; }
    split = 16;
    while (split > 1 && (uint64_t)(8 * slots * split) * slot_bytes > ((uint64_t)(two_slot_default ? 320 : 256) << 20)) split >>= 1;
  }

  // One XCD-fused launch (kern_xcd.hpp, kern_xcd_real.hpp, kern_regtile.hpp): grouping, workspace, control block and tables.
  static constexpr int XCC_IDS = 16;                     // workspace slot sets: one per XCC id a workgroup can read (4 bits)
  static constexpr uint64_t XCD_CTL_BYTES = 40960;       // control block of a shared-mode launch (kern_xcd.hpp XcdCtl)
  static constexpr int64_t XCD_CTL_ZERO_FLOATS = 9216;   // the part of it the ST_ZERO before every such launch clears (all of XcdCtl)
  struct XcdLaunch {
    bool solo;
    int64_t grid, split = 1, slots = 1;
    PtrRef wslots, ctl, ta, tb, lo, hi;   // tables: pass A's and pass B's stage roots, the four-step roots as HI[m >> shift] * LO[m & mask]
    int shift = 0;
  };
  // Solo: every workgroup walks whole transforms alone (no registration, no cross-workgroup barrier, so no co-residency requirement
  // and as many workgroups per CU as fit), one slot of `slot_elems` points each, all of them within the Infinity Cache.  Shared: the
  // groups of an XCD share each transform; `split` groups of `slots` slots per XCC id, every workgroup co-resident — one per CU, two
  // where 256 threads and <= 80 KB of LDS leave room.
  XcdLaunch xcd_launch(const XcdKernelMeta& xm, bool solo, int64_t slot_elems, int64_t transforms) {
    XcdLaunch x{solo, opt.compute_units};
    if (solo) {
      const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((160 * 1024) / xm.lds_bytes, 2048 / xm.threads), 4));
      x.grid = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((int64_t)opt.compute_units * per_cu, ((int64_t)opt.solo_cap_mb << 20) / (slot_elems * 8)), transforms));
      x.wslots = alloc_work((uint64_t)x.grid * slot_elems * 8);
      x.ctl = alloc_work(256);
    } else {
      xcd_groups(xm, (uint64_t)slot_elems * 8, x.split, x.slots);
      x.wslots = alloc_work((uint64_t)(XCC_IDS * x.slots * x.split) * slot_elems * 8);
      x.ctl = alloc_work(XCD_CTL_BYTES);
      if (opt.xcd_fused != 2 && ((xm.threads <= 256 && xm.lds_bytes <= 80 * 1024) || xm.kind == XK_HX)) x.grid *= 2;
    }
    return x;
  }
  // four-step roots e^{-2 pi i m/N}: 2^shift LO roots (shift = 10 from 2^20 up, half of log2 N below), HI of N >> shift
  // (N = 2^20: 1024 + 1024 entries, the RT1K_ROOT_* constants of plan.hpp with which fft_xcd_rt1k_kernel stages both tables in LDS)
  void xcd_roots(XcdLaunch& x, int64_t N) {
    x.shift = N >= (1 << 20) ? RT1K_ROOT_SHIFT : lg2(N) / 2;
    std::vector<float2h> lo((size_t)1 << x.shift), hi((size_t)std::max<int64_t>(1, N >> x.shift));
    for (size_t l = 0; l < lo.size(); ++l) lo[l] = root_of_unity((int64_t)l, N);
    for (size_t h = 0; h < hi.size(); ++h) hi[h] = root_of_unity((int64_t)h << x.shift, N);
    x.lo = add_table(lo);
    x.hi = add_table(hi);
  }
  // the ST_ZERO of the control block (shared mode) and the launch with the fields every fused emitter fills (dispatch.hpp
  // ST_XCD_FUSED); the caller adds the scale, pitches other than N (i[XS_IN_PITCH], i[XS_OUT_PITCH]) and its own fields
  Step& push_xcd(StepKind kind, int variant, const XcdLaunch& x, PtrRef src, PtrRef dst, int64_t transforms, int64_t N) {
    if (!x.solo) zero(x.ctl, XCD_CTL_ZERO_FLOATS).grid = 1;   // (8 KiB: one workgroup)
    Step& st = push(kind);
    st.variant = variant;
    st.p[XP_IN] = src; st.p[XP_OUT] = dst; st.p[XP_WSLOTS] = x.wslots; st.p[XP_CTL] = x.ctl; st.p[XP_TABLE] = PtrRef(BUF_TABLE, 0);
    st.i[XS_TRANSFORMS] = transforms; st.i[XS_N] = N; st.i[XS_FS_SHIFT] = x.shift; st.i[XS_FS_LO_MASK] = ((int64_t)1 << x.shift) - 1;
    st.i[XS_TW_A_OFF] = x.ta.off; st.i[XS_TW_B_OFF] = x.tb.off; st.i[XS_TW_LO_OFF] = x.lo.off; st.i[XS_TW_HI_OFF] = x.hi.off; st.i[XS_SPLIT] = x.split; st.i[XS_IN_PITCH] = N; st.i[XS_OUT_PITCH] = N;
    st.i[XS_SLOTS] = x.slots; st.i[XS_SOLO] = x.solo ? 1 : 0; st.i[XS_SPIN_LIMIT] = opt.xcd_spin_limit;
    st.grid = (unsigned)x.grid;
    return st;
  }
  // route names of the 1-D c2c kinds in shared mode (bench.py and the tests match on them)
  static const char* xcd_c2c_route(XcdKind k) {
    switch (k) {
      case XK_RT: return "xcd-fused-rt";
      case XK_HX: return "xcd-fused-2wg";
      case XK_RT1K: case XK_RT1K_2048: return "xcd-fused-rt32";
      case XK_RT1K_16: return "xcd-fused-rt16x2";
      default: return "xcd-fused";
    }
  }

  // 2-D c2c planes [N1][N0] (axis 0 = N0 fastest) through the fused kernel's TWO_D instances; false if none applies
  bool emit_xcd_2d(PtrRef src, PtrRef dst, int64_t N0, int64_t N1, int64_t planes, bool inverse, float scale) {
    if (opt.force_generic || opt.xcd_fused != 1 || opt.only_pass || !opt.xcd_2d) return false;
    const XcdKernelMeta* xm = nullptr;
    for (const auto& m : xcd_kernel_registry()) if (m.kind == XK_TWO_D && m.N1 == N1 && m.N2 == N0 && m.inverse == inverse) xm = &m;
    if (!xm) return false;
    const int64_t N = N0 * N1;
    const LineKernelMeta ma = make_meta(0, xm->N1, xm->ra[0], xm->ra[1], xm->ra[2], xm->ta, true, true, false, false, 0);
    const LineKernelMeta mb = make_meta(0, xm->N2, xm->rb[0], xm->rb[1], xm->rb[2], xm->tb, false, false, false, false, 0);
    const bool solo = (uint64_t)N * 8 <= ((uint64_t)opt.solo_max_kb_2d << 10);
    if (!solo && !opt.xcd_shared) return false;
    XcdLaunch x = xcd_launch(*xm, solo, N, planes);
    x.ta = line_tables(ma);
    x.tb = line_tables(mb);
    x.lo = x.hi = add_table(std::vector<float2h>(1, float2h{1, 0}));   // no four-step roots (shift 0)
    Step& st = push_xcd(ST_XCD_FUSED, xm->id, x, src, dst, planes, N);
    st.f[F_SCALE] = scale;
    ir.route += std::string(solo ? "xcd-2d-solo[" : "xcd-2d[") + std::to_string(N0) + "x" + std::to_string(N1) + "] ";
    return true;
  }

  // XCD-fused r2c of `lines` dense real lines of length N into packed spectra of N/2+1 bins; false if no instance applies
  bool emit_xcd_r2c(PtrRef src, PtrRef dst, int64_t N, int64_t lines, float scale, bool c2r = false) {
    if (opt.force_generic || !opt.xcd_fused || !opt.xcd_r2c || opt.only_pass || N < 4096 || (N & (N - 1))) return false;
    const int lgf = lg2(N);
    const int64_t F1 = (int64_t)1 << (lgf / 2), F2 = N / F1;
    const XcdKind kind = c2r ? XK_C2R : XK_R2C, kind_rt = c2r ? XK_RT_C2R : XK_RT_R2C;
    const XcdKernelMeta* xm = nullptr;
    for (const auto& m : xcd_kernel_registry())
      if ((m.kind == kind || (m.kind == kind_rt && opt.xcd_rt && opt.xcd_shared)) && m.N1 == F1 && m.N2 == F2) xm = &m;
    if (!xm || (N <= 8192 && opt.xcd_fused != 2)) return false;
    const bool rt = xm->kind == kind_rt;
    const LineKernelMeta ma = make_meta(0, rt ? 1024 : xm->N1, rt ? 32 : xm->ra[0], xm->ra[1], xm->ra[2], xm->ta, true, true, false, false, 0);
    const LineKernelMeta mb = make_meta(0, rt ? 1024 : xm->N2, rt ? 32 : xm->rb[0], xm->rb[1], xm->rb[2], xm->tb, false, true, false, false, 0);
    const int64_t wsize = c2r ? (rt ? (F1 / 2) * F2 : F1 * (F2 / 2 + 16)) : (F1 / 2 + 1) * F2;   // r2c: rows 0..N1/2; c2r: columns 0..N2/2 (+ padding; register tiles: N1/2 packed full rows)
    // small transforms: one workgroup per transform (solo mode, see emit_axis); the real line is N*4 bytes
    const bool solo = (uint64_t)N * 4 <= ((uint64_t)opt.solo_max_kb << 10) / (c2r ? 1 : 2) && opt.xcd_fused != 2;
    if (!solo && !opt.xcd_shared) return false;
    XcdLaunch x = xcd_launch(*xm, solo, wsize, lines);
    x.tb = rt ? regtile_table() : line_tables(mb);
    x.ta = rt && xm->N1 == 2048 ? x.tb : line_tables(ma);
    xcd_roots(x, N);
    Step& st = push_xcd(ST_XCD_FUSED, xm->id, x, src, dst, lines, N);
    st.i[XS_IN_PITCH] = c2r ? N / 2 + 1 : N / 2; st.i[XS_OUT_PITCH] = c2r ? N / 2 : N / 2 + 1;        // pitches in complex elements
    st.f[F_SCALE] = scale;
    ir.route += std::string(c2r ? "xcd-c2r" : "xcd-r2c") + (solo ? "-solo" : rt ? "-rt" : "") + "[N=" + std::to_string(xm->N1) + "x" + std::to_string(xm->N2) + "] ";
    return true;
  }

  // r2c of dense real lines of length N = 2H, H a power of two in 64..max_line: the ROW line kernel of length H with the split
  // fused behind its last stage (one launch instead of FFT + r2c_post_kernel)
  // (c2r: the mirror — the pre-split rides the first-stage loads of the INVERSE line kernel, any power-of-two half length >= 2)
  // trig = LM_DCT2 / LM_DST2 (c2r: LM_DCT3 / LM_DST3; 0: none): the same launch as a whole DCT-II / DST-II of the real lines (kern_lines.hpp fft_lines_r2c_kernel<C, TRIG>)
  // im / om (optional, both or none): the launch reads its input side through im and writes through om (fft_lines_r2c_kernel /
  // fft_lines_c2r_kernel <.., MAPPED>; the real side's map counts floats, the packed side's complex bins)
  const LineKernelMeta* lines_r2c_kernel(int64_t N, bool c2r, bool mapped) const {
    const int64_t H = N / 2;
    if (opt.force_generic || !(c2r ? opt.lines_c2r : opt.lines_r2c) || (N & 1) || !is_pow2(H) || H < (c2r ? 2 : 64) || H > opt.max_line || (opt.xcd_fused == 2 && N == 4096)) return nullptr;
    // (N = 2^15 c2r: round 1 kept the Hermitian four-step in solo mode there, 322 vs 304; with the 16-byte pre-split accesses of r02
    // the line kernel is ahead, 347 vs 320; lines_c2r = 3 restores the old choice)   // xcd_fused == 2: emulation tests of the fused instances
    if (c2r && H > 8192 && opt.lines_c2r == 3 && !mapped) return nullptr;
    const LineKernelMeta* m = find_line_kernel((int)H, false, false, c2r, c2r, 0);
    if (!m || (!c2r && m->lds_bytes == 0)) return nullptr;
    if (mapped && (!opt.fuse_views || m->lds_bytes == 0 || m->R1 <= 1)) return nullptr;   // the mapped forms keep the line in LDS
    return m;
  }
  bool emit_lines_r2c(PtrRef src, PtrRef dst, int64_t N, int64_t lines, float scale, bool c2r = false, int trig = 0,
                      const SideMap* im = nullptr, const SideMap* om = nullptr) {
    const int64_t H = N / 2;
    const LineKernelMeta* m = lines_r2c_kernel(N, c2r, im != nullptr);
    if (!m) return false;
    // DCT-II / DST-II launches: the alternate shapes (DCT-III / DST-III on the c2r kernel measured -9...+5 % with them and keep the plain ones)
    if (trig && !c2r && opt.trig_alt) { if (const LineKernelMeta* alt = find_line_kernel((int)H, false, false, false, false, 4)) m = alt; }
    std::vector<float2h> lo(1024), hi((size_t)std::max<int64_t>(1, (H + 1023) >> 10));
    for (int64_t l = 0; l < 1024; ++l) lo[(size_t)l] = root_of_unity(l, N);
    for (size_t h = 0; h < hi.size(); ++h) hi[h] = root_of_unity((int64_t)h << 10, N);
    // trig: the DCT phases e^{-i pi m/2N} = e^{-2 pi i m/4N}, m = 0..N/2, f64-built, directly behind the 1024 LO roots (one table)
    if (trig) for (int64_t mm = 0; mm <= H; ++mm) lo.push_back(root_of_unity(mm, 4 * N));
    Step& st = push_lines(*m, src, dst, lines, {1, c2r ? H + 1 : H}, {1, c2r ? H : H + 1}, scale);
    st.p[LP_TW_LO] = add_table(lo); st.p[LP_TW_HI] = add_table(hi);
    st.i[LS_FS_SHIFT] = 10; st.i[LS_FS_LO_MASK] = 1023;
    st.i[LS_MODE] = trig ? trig : (c2r ? LM_C2R : LM_R2C);
    if (im) {
      st.i[LS_MAPPED] = 1; st.imap = *im; st.omap = *om; st.imap.ax = st.omap.ax = 0;
      ir.route += std::string(c2r ? "lines-c2r-mapped[N=" : "lines-r2c-mapped[N=") + std::to_string(N) + "] ";
      return true;
    }
    ir.route += std::string(trig == LM_DCT2 ? "lines-dct2[N=" : trig == LM_DST2 ? "lines-dst2[N=" : trig == LM_DCT3 ? "lines-dct3[N=" : trig == LM_DST3 ? "lines-dst3[N=" : c2r ? "lines-c2r[N=" : "lines-r2c[N=") + std::to_string(N) + "] ";
    return true;
  }

  // 1-D r2c of `lines` dense real lines of even length N into packed spectra (N/2+1 bins): fused line kernel, real four-step,
  // or the half-length complex FFT + split
  int emit_r2c_even(PtrRef in, PtrRef out, int64_t N, int64_t lines, float scale, std::string& err) {
    if (emit_lines_r2c(in, out, N, lines, scale)) return MI355FFT_OK;   // one launch: split fused behind the last stage (fft_lines_r2c_kernel)
    // N = 2^16: the half-length route over the single-workgroup line of 2^15 points measured 318 vs 269 G real points/s for the
    // real four-step in solo mode (c2r: 318 vs 305)
    const bool half32k = N == 65536 && opt.line32k && opt.max_line >= 16384 && !opt.force_generic && !opt.only_pass && opt.xcd_fused != 2;
    if (!half32k && emit_xcd_r2c(in, out, N, lines, scale)) return MI355FFT_OK;     // one persistent launch: real four-step (kern_xcd_real.hpp)
    const int64_t H = N / 2, P = H + 1;
    PtrRef z = alloc_work((uint64_t)lines * H * 8);
    // the real input, read as `lines` complex lines of length H: z[n] = x[2n] + i x[2n+1]
    int rc = emit_axis(in, z, H, 1, lines, false, 1.0f, err);
    if (rc) return rc;
    Step& st = push(ST_R2C_POST);
    st.p[P_SRC] = z; st.p[P_DST] = out;
    split_roots(st, N, H / 2 + 1);
    st.i[RS_H] = H; st.i[RS_BATCH] = lines; st.i[RS_LINE_STRIDE] = P; st.f[F_SCALE] = scale;
    st.grid = oneshot_grid(split_items(lines, H));      // items of 512 bin pairs (r2c_post_kernel)
    ir.route += "r2c-split ";
    return MI355FFT_OK;
  }
  // the mirror: packed spectra -> real lines (unnormalised inverse times `scale`)
  int emit_c2r_even(PtrRef packed, PtrRef out, int64_t N, int64_t lines, float scale, std::string& err) {
    if (emit_lines_r2c(packed, out, N, lines, scale, true)) return MI355FFT_OK;   // pre-split in the first-stage loads (fft_lines_c2r_kernel)
    const bool half32k = N == 65536 && opt.line32k && opt.max_line >= 16384 && !opt.force_generic && !opt.only_pass && opt.xcd_fused != 2;
    if (!half32k && emit_xcd_r2c(packed, out, N, lines, scale, true)) return MI355FFT_OK;     // Hermitian four-step (kern_xcd_real.hpp)
    const int64_t H = N / 2, P = H + 1;
    PtrRef z = alloc_work((uint64_t)lines * H * 8);
    Step& st = push(ST_C2R_PRE);
    st.p[P_SRC] = packed; st.p[P_DST] = z;
    split_roots(st, N, H / 2 + 1);
    st.i[RS_H] = H; st.i[RS_BATCH] = lines; st.i[RS_LINE_STRIDE] = P;
    st.grid = oneshot_grid(split_items(lines, H));      // items of 512 bin pairs (c2r_pre_kernel)
    // unnormalised inverse of length H lands x[2n] + i x[2n+1]: exactly the real output, read as complex
    int rc = emit_axis(z, out, H, 1, lines, true, scale, err);
    if (rc) return rc;
    ir.route += "c2r-split ";
    return MI355FFT_OK;
  }

  // Lane layouts (channel-lane presets, whdcn with unit stride along the line): contiguous power-of-two lines that sit at
  // arbitrary pitches on either side need no gather / scatter pass — the ROW line kernels take the two pitches as they are.
  // rank-1 view of a four-step line (ioView / zeroPad / unit-stride lanes) on a VIEW instance of the fused kernels: the maps' ranges are
  // predicates of pass A's loads and pass B's stores — no embed / zero / extract launch.  false: no instance for this length.
  bool emit_xcd_view(PtrRef in, PtrRef out, int64_t N, int64_t lines, bool inverse, float scale, const SideMap& im, const SideMap& om) {
    if (opt.force_generic || opt.xcd_fused != 1 || !opt.xcd_shared || !opt.fuse_views || opt.only_pass) return false;
    const XcdKernelMeta* xm = nullptr;
    for (const auto& m : xcd_kernel_registry())
      if ((m.kind == XK_VIEW || m.kind == XK_RT1K_VIEW) && (int64_t)m.N1 * m.N2 == N && m.inverse == inverse) xm = &m;
    if (!xm) return false;
    XcdLaunch x = xcd_launch(*xm, false, N, lines);
    const LineKernelMeta ml = make_meta(0, xm->N1, xm->ra[0], xm->ra[1], xm->ra[2], xm->ta, true, true, false, false, 0);
    const LineKernelMeta mr = make_meta(0, xm->N2, xm->rb[0], xm->rb[1], xm->rb[2], xm->tb, false, true, false, false, 0);
    x.ta = line_tables(ml);
    x.tb = line_tables(mr);
    xcd_roots(x, N);
    Step& st = push_xcd(ST_XCD_FUSED, xm->id, x, in.plus(im.offset * 8), out.plus(om.offset * 8), lines, N);
    st.i[XS_IN_PITCH] = im.batch_stride; st.i[XS_OUT_PITCH] = om.batch_stride;
    st.f[F_SCALE] = scale;
    st.imap = im; st.omap = om;
    ir.route += "xcd-fused-view[N=" + std::to_string(xm->N1) + "x" + std::to_string(xm->N2) + "] ";
    return true;
  }
  bool emit_lines_pitched(PtrRef src, PtrRef dst, int64_t N, int64_t lines, bool inverse, float scale, int64_t in_pitch, int64_t out_pitch) {
    if (opt.force_generic || !is_pow2(N) || N < 2 || N > opt.max_line || (opt.xcd_fused == 2 && N == 4096)) return false;
    const LineKernelMeta* m = find_line_kernel((int)N, false, false, inverse, inverse, 0);
    if (!m) return false;
    push_lines(*m, src, dst, lines, {1, in_pitch}, {1, out_pitch}, scale, true);
    ir.route += "lines[N=" + std::to_string(N) + ",pitch=" + std::to_string(in_pitch) + "/" + std::to_string(out_pitch) + "] ";
    return true;
  }

  // ---- mapped sides: strided layouts, ioView and zeroPad carried by the first load / last store -------
  // Can the pass over an axis of length N with element stride S be a line-kernel launch (ROW for S == 1, column tiles above)?
  bool axis_mappable(int64_t N, int64_t S, bool inverse) const {
    if (opt.force_generic || !opt.fuse_views || !is_pow2(N) || N < 2) return false;
    if (S == 1) return N <= opt.max_line && !(opt.xcd_fused == 2 && N == 4096) && find_line_kernel((int)N, false, false, inverse, inverse, 0) != nullptr;
    return find_line_kernel((int)N, true, true, inverse, inverse, 0) != nullptr;
  }
  static SideMap dense_map(const int64_t* shape, int rank) {
    SideMap m;
    m.rank = rank;
    int64_t st = 1;
    for (int d = 0; d < rank; ++d) { m.dims[d] = (int)shape[d]; m.stride[d] = st; m.lo[d] = m.zlo[d] = 0; m.hi[d] = m.zhi[d] = (int)shape[d]; st *= shape[d]; }
    m.batch_stride = st;
    return m;
  }
  // first and last axis emit_nd will transform (-1: none)
  static void nd_first_last(const int64_t* shape, int rank, uint32_t axes_mask, int& first, int& last) {
    first = last = -1;
    for (int a = 0; a < rank; ++a)
      if (shape[a] > 1 && (axes_mask == 0 || ((axes_mask >> a) & 1u))) { if (first < 0) first = a; last = a; }
  }
  // one line-kernel launch over axis `ax` with both sides given as maps (kern_lines.hpp fft_lines_mapped_kernel)
  int emit_axis_mapped(PtrRef src, PtrRef dst, int64_t N, int64_t S, int64_t outer, bool inverse, float scale, SideMap im, SideMap om, int ax) {
    const bool col = S > 1;
    const LineKernelMeta* m = find_line_kernel((int)N, col, col, inverse, inverse, 0);
    if (!m) return MI355FFT_ERR_UNSUPPORTED;
    im.ax = om.ax = ax;
    Step& st = push_lines(*m, src, dst, S * outer, {S, S * N}, {S, S * N}, scale);
    st.i[LS_MAPPED] = 1;
    st.imap = im; st.omap = om;
    ir.route += std::string(col ? "columns-mapped[N=" : "lines-mapped[N=") + std::to_string(N) + (col ? ",S=" + std::to_string(S) : "") + "] ";
    return MI355FFT_OK;
  }

  int emit_axis(PtrRef src, PtrRef dst, int64_t N, int64_t S, int64_t outer, bool inverse, float scale, std::string& err) {
    const int64_t lines = S * outer;
    // work buffers taken inside one axis transform are temporaries: released on every exit
    struct Scope { uint64_t& top; uint64_t mark; ~Scope() { top = mark; } } scope{work_top, work_top};
    if (N == 1) {
      if (!src.same(dst)) { Step& c = push(ST_COPY); c.p[P_SRC] = src; c.p[P_DST] = dst; c.i[S_COUNT] = lines * 8; }
      if (scale != 1.0f) { Step& s = push(ST_SCALE); s.p[P_DATA] = dst; s.i[S_COUNT] = lines * 2; s.f[F_SCALE] = scale; s.grid = generic_grid(lines * 2); }
      return MI355FFT_OK;
    }
    const bool p2 = is_pow2(N);
    // N = 2^15 and 2^13 (line32k >= 1; 2^14 too with line32k == 2: measured equal to its ROW kernel), dense lines: the whole line in the
    // registers of one workgroup of N/64 threads, exchanges through LDS in halves (kern_line32k.hpp, kern_line_reg.hpp).  2^15: one HBM
    // round trip where the solo four-step makes two (288 vs 210 GPoints/s); 2^13: four 128-thread workgroups per CU instead of two
    // 256-thread ones with the line in LDS (330 vs 288)
    if (!opt.force_generic && opt.max_line >= 16384 && S == 1 && !opt.only_pass && opt.xcd_fused != 2 &&
        ((opt.line32k >= 1 && (N == 32768 || N == 8192)) || (opt.line32k == 2 && (N == 16384 || N == 4096)))) {
      const int lg = lg2(N);
      const int R0 = 32, R1 = N <= 8192 ? 16 : 32;
      std::vector<float2h> t;
      for (int q = 1; q < R1; ++q) for (int k = 0; k < R0; ++k) t.push_back(root_of_unity((int64_t)q * k, (int64_t)R0 * R1));
      for (int64_t l = 0; l < 1024; ++l) t.push_back(root_of_unity(l, N));
      for (int64_t h = 0; h < N / 1024; ++h) t.push_back(root_of_unity(h << 10, N));
      Step& st = push(ST_LINES_MIXED);
      st.variant = 1000 + lg;
      st.p[P_SRC] = src; st.p[P_DST] = dst; st.p[P_TW] = add_table(t);
      st.i[MX_LINES] = lines; st.i[MX_N] = N; st.i[MX_S] = 1; st.i[MX_T] = 1; st.i[MX_NST] = 3;
      st.i[MX_SWAP] = inverse ? 1 : 0; st.i[MX_THREADS] = N / 64;
      st.f[F_SCALE] = scale;
      const int64_t per_cu = N == 32768 ? 1 : (N == 16384 ? 2 : (N == 8192 ? 4 : 8));
      st.grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(lines, (int64_t)opt.compute_units * per_cu));
      ir.route += (N == 32768 ? std::string("line32k[N=32768] ") : "line-reg[N=" + std::to_string(N) + "] ");
      return MI355FFT_OK;
    }
    if (!opt.force_generic && S == 1 && p2 && N <= opt.max_line && !(opt.xcd_fused == 2 && N == 4096)) {   // xcd_fused == 2: emulation tests
      const LineKernelMeta* m = find_line_kernel((int)N, false, false, inverse, inverse, 0);
      if (m) {
        push_lines(*m, src, dst, lines, {1, N}, {1, N}, scale, true);
        ir.route += "lines[N=" + std::to_string(N) + "] ";
        return MI355FFT_OK;
      }
    }
    // the column line kernels address a tile with 32-bit element offsets (kern_lines.hpp: voff = idx * S): a strided axis whose
    // plane spans 2^32 elements or more (32 GiB of complex data) stays on the stage route, which indexes with 64 bits
    const bool col_span_ok = (uint64_t)N * (uint64_t)S < (1ull << 32);
    if (!opt.force_generic && S > 1 && p2 && col_span_ok) {
      // an axis with stride S > 1 (N-D transforms): T adjacent lines form a column tile
      const LineKernelMeta* m = find_line_kernel((int)N, true, true, inverse, inverse, 0);
      if (m && S % m->T == 0) {
        push_lines(*m, src, dst, lines, {S, S * N}, {S, S * N}, scale, false, lines / m->T);
        ir.route += "columns[N=" + std::to_string(N) + ",S=" + std::to_string(S) + "] ";
        return MI355FFT_OK;
      }
      // S not a multiple of the tile width (the packed axis 0 of an N-D r2c: S = N0/2 + 1): per-group tiles, ragged last one
      const LineKernelMeta* mr = find_line_kernel((int)N, true, true, inverse, inverse, 3);
      if (mr && S >= mr->T) {
        const int64_t tpg = (S + mr->T - 1) / mr->T;
        push_lines(*mr, src, dst, lines, {S, S * N}, {S, S * N}, scale, false, outer * tpg).i[LS_FS_GROUP] = tpg;
        ir.route += "columns-ragged[N=" + std::to_string(N) + ",S=" + std::to_string(S) + "] ";
        return MI355FFT_OK;
      }
    }
    if (!opt.force_generic && S == 1 && N == (1 << 20) && opt.xcd_res && opt.xcd_shared && !opt.only_pass && opt.compute_units % 32 == 0) {
      // XCD-resident route (kern_xcd_res.hpp): the transform stays in the registers and LDS of one XCD's 32 workgroups between
      // its passes; hand-offs go through a 4 MiB L2-resident exchange buffer per XCD.  One workgroup per CU, all co-resident.
      XcdLaunch x{false, opt.compute_units, opt.xcd_res_depth, 1};
      x.wslots = alloc_work((uint64_t)XCC_IDS * 4 * (1 << 20));   // 4 channels of 1 MiB per XCC id
      x.ctl = alloc_work(XCD_CTL_BYTES);
      x.ta = x.tb = line_tables(make_meta(0, 1024, 32, 32, 1, 16, true, true, false, false, 0));
      xcd_roots(x, N);
      const int variant = (inverse ? 1 : 0) + (opt.xcd_res == 2 || opt.xcd_res == 4 ? 2 : 0) + (opt.xcd_res >= 3 && !inverse ? 4 : 0);   // 3: stamps, 4: stamps on the skeleton
      Step& st = push_xcd(ST_XCD_RES, variant, x, src, dst, lines, N);
      st.f[F_SCALE] = scale;
      ir.route += "xcd-resident[N=1024x1024,depth=" + std::to_string(opt.xcd_res_depth) + (opt.xcd_res == 2 || opt.xcd_res == 4 ? ",skeleton" : "") + (opt.xcd_res >= 3 ? ",stamps" : "") + "] ";
      return MI355FFT_OK;
    }
    if (!opt.force_generic && S == 1 && p2 && N >= 4096 && opt.xcd_fused && !opt.only_pass) {
      // XCD-fused route: both passes in one persistent launch, one transform per XCD at a time (kern_xcd.hpp)
      const int lgf = lg2(N);
      const int64_t F1 = (int64_t)1 << (lgf / 2), F2 = N / F1;
      // the LDS-resident kernel, or a register-tile form where the options select it and shared mode is allowed (the VIEW instances
      // serve emit_xcd_view, 2048 x 1024 the 2^21 choice below)
      const auto usable = [&](XcdKind k) {
        switch (k) {
          case XK_FUSED: return true;
          case XK_RT: return opt.xcd_rt != 0 && opt.xcd_shared;
          case XK_HX: return opt.xcd_hx == 1 && opt.xcd_shared;
          case XK_RT1K: return opt.xcd_hx == 2 && opt.xcd_shared;
          case XK_RT1K_16: return opt.xcd_hx == 3 && opt.xcd_shared;
          default: return false;
        }
      };
      const XcdKernelMeta* xm = nullptr;
      for (const auto& m : xcd_kernel_registry()) if (usable(m.kind) && m.N1 == F1 && m.N2 == F2 && m.inverse == inverse) xm = &m;
      // c2c 2^21: with two groups per XCD and one slot each the LDS-resident 1024 x 2048 instance (8-line tiles taken in pairs) runs at 177
      // GPoints/s, ahead of both register-tile forms — 2048 x 1024 (16-line tiles down the columns, 32-line tiles along the rows;
      // MI355FFT_XCD_RT=3) 172, 1024 x 2048 (MI355FFT_XCD_RT=2) 162: profiles/r03_regtile_ab.log.  So the register tiles serve 2^22 only.
      if (N == ((int64_t)1 << 21) && opt.xcd_rt != 2) {
        xm = nullptr;
        for (const auto& m : xcd_kernel_registry())
          if (m.inverse == inverse && ((opt.xcd_rt == 3 && opt.xcd_shared) ? m.kind == XK_RT1K_2048 : (m.kind == XK_FUSED && m.N1 == F1 && m.N2 == F2))) xm = &m;
      }
      if (xm && (N > 4096 || opt.xcd_fused == 2) &&
          (opt.xcd_shared || ((uint64_t)N * 8 <= ((uint64_t)opt.solo_max_kb << 10) && opt.xcd_fused != 2))) {
        const bool rt = xm->kind == XK_RT, a_rt = rt && xm->N1 == 2048;   // register-tile passes take their stage-2 table instead of a line kernel's
        const LineKernelMeta ma = make_meta(0, a_rt ? 1024 : xm->N1, xm->ra[0], a_rt ? 32 : xm->ra[1], xm->ra[2], xm->ta, true, true, false, false, 0);
        const LineKernelMeta mb = make_meta(0, rt ? 1024 : xm->N2, rt ? 32 : xm->rb[0], xm->rb[1], xm->rb[2], xm->tb, false, true, false, false, 0);
        // transforms of at most 1 MiB run in solo mode (xcd_launch); larger ones are shared by the groups of an XCD
        const bool solo = (uint64_t)N * 8 <= ((uint64_t)opt.solo_max_kb << 10) && opt.xcd_fused != 2;
        XcdLaunch x = xcd_launch(*xm, solo, N, lines);
        x.tb = rt ? regtile_table() : line_tables(mb);
        x.ta = a_rt ? x.tb : xm->kind == XK_RT1K_2048 ? regtile_table() : line_tables(ma);
        xcd_roots(x, N);
        Step& st = push_xcd(ST_XCD_FUSED, xm->id, x, src, dst, lines, N);
        if (lane_in_pitch) st.i[XS_IN_PITCH] = lane_in_pitch;
        if (lane_out_pitch) st.i[XS_OUT_PITCH] = lane_out_pitch;
        if (lane_in_pitch || lane_out_pitch) lane_used = true;
        st.f[F_SCALE] = scale;
        ir.route += std::string(solo ? "xcd-solo" : xcd_c2c_route(xm->kind)) + "[N=" + std::to_string(xm->N1) + "x" + std::to_string(xm->N2) + "] ";
        return MI355FFT_OK;
      }
    }
    if (!opt.force_generic && S == 1 && p2 && N > 4096) {
      const int lg = lg2(N);
      const int64_t N1 = (int64_t)1 << (lg / 2), N2 = N / N1;
      const LineKernelMeta* ma = find_line_kernel((int)N1, true, true, inverse, false, 0);
      const LineKernelMeta* mb = find_line_kernel((int)N2, false, true, false, inverse, 2);
      if (ma && mb && N2 % ma->T == 0 && N1 % mb->T == 0) {
        int64_t chunk = (int64_t)(opt.chunk_bytes / (uint64_t)(N * 8));
        chunk = std::max<int64_t>(1, std::min(chunk, lines));
        const PtrRef w = alloc_work((uint64_t)chunk * N * 8);
        const PtrRef ta = line_tables(*ma), tb = line_tables(*mb);
        // four-step roots e^{-2 pi i m/N}, m = n2*k1 < N, as HI[m >> 10] * LO[m & 1023]
        std::vector<float2h> lo(1024), hi((size_t)(N >> 10));
        for (int64_t l = 0; l < 1024; ++l) lo[(size_t)l] = root_of_unity(l, N);
        for (int64_t h = 0; h < (N >> 10); ++h) hi[(size_t)h] = root_of_unity(h << 10, N);
        const PtrRef tlo = add_table(lo), thi = add_table(hi);
        for (int64_t t0 = 0; t0 < lines; t0 += chunk) {
          const int64_t c = std::min(chunk, lines - t0);
          if (opt.only_pass != 2) {
          Step& a = push(ST_LINES);
          a.variant = ma->id;
          a.p[LP_IN] = src.plus(t0 * N * 8); a.p[LP_OUT] = w; a.p[LP_TW] = ta;
          a.i[LS_TILES] = c * N2 / ma->T; a.i[LS_LINES] = c * N2; a.i[LS_IN_S] = N2; a.i[LS_IN_OUTER] = N; a.i[LS_OUT_S] = N2; a.i[LS_OUT_OUTER] = N;
          a.f[F_SCALE] = 1.0f;
          a.grid = lines_grid(*ma, a.i[LS_TILES]);
          }
          if (opt.only_pass == 1) continue;
          Step& b = push(ST_LINES);
          b.variant = mb->id;
          b.p[LP_IN] = w; b.p[LP_OUT] = dst.plus(t0 * N * 8); b.p[LP_TW] = tb; b.p[LP_TW_LO] = tlo; b.p[LP_TW_HI] = thi;
          b.i[LS_TILES] = c * N1 / mb->T; b.i[LS_LINES] = c * N1; b.i[LS_IN_S] = 1; b.i[LS_IN_OUTER] = N2; b.i[LS_OUT_S] = N1; b.i[LS_OUT_OUTER] = N; b.i[LS_FS_SHIFT] = 10; b.i[LS_FS_LO_MASK] = 1023;
          b.f[F_SCALE] = scale;
          b.grid = lines_grid(*mb, b.i[LS_TILES]);
          // four-step roots e^{-2 pi i k1 n2/N} enter at pass B's loads; with a grid that is a multiple of the
          // tiles per transform every workgroup keeps the same rows k1 and computes its roots once per launch
          const int64_t tpt = N1 / mb->T;
          if ((int64_t)b.grid >= tpt) b.grid = (unsigned)((b.grid / tpt) * tpt);
          b.i[LS_FS_GROUP] = N1;
        }
        ir.route += "two-pass[N=" + std::to_string(N1) + "x" + std::to_string(N2) + ",chunk=" + std::to_string(chunk) + "] ";
        return MI355FFT_OK;
      }
    }
    // generic: one global-memory Stockham stage per radix
    const std::vector<int> radices = factorize_radices(N);
    if (radices.empty()) return emit_bluestein(src, dst, N, S, outer, inverse, scale, err);
    int ns = (int)radices.size();
    const std::vector<int> lds_radices = factorize_radices(N, 8);
    // (short lines that the stage route finishes in three passes with a radix-16/32 first stage measured faster there: 640, 768)
    // (strided axes need T >= 8 adjacent lines per workgroup for coalesced accesses: N <= 512; longer ones keep the stage route —
    // measured 27 GPoints/s for the 4096-point axis of a 4096x4096 array with T = 1)
    // dense lines of a length with a compile-time-plan instance (kern_mixed_ct.hpp)
    if (opt.mixed_lines && opt.mixed_ct && !opt.force_generic && S == 1) {
      const MixedCtMeta* cm = nullptr;
      for (const auto& m : mixedct_registry()) if (m.N == N && (!cm || opt.mixed_ct != 2)) cm = &m;
      if (cm) {
        std::vector<float2h> t;
        Step& st = push(ST_LINES_MIXED);
        int64_t nsp = 1;
        for (int R : cm->radices) {
          const size_t off = t.size();
          t.resize(off + (size_t)(R * nsp));
          for (int q = 0; q < R; ++q) for (int64_t k = 0; k < nsp; ++k) t[off + (size_t)(q * nsp + k)] = root_of_unity(q * k, nsp * R);
          nsp *= R;
        }
        st.variant = cm->id + 1;
        st.p[P_SRC] = src; st.p[P_DST] = dst; st.p[P_TW] = add_table(t);
        st.i[MX_LINES] = lines; st.i[MX_N] = N; st.i[MX_S] = 1; st.i[MX_T] = cm->T; st.i[MX_NST] = (int64_t)cm->radices.size();
        st.i[MX_SWAP] = inverse ? 1 : 0; st.i[MX_THREADS] = cm->threads;
        st.f[F_SCALE] = scale;
        const int64_t tiles = (lines + cm->T - 1) / cm->T;
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((160 * 1024) / (cm->lds_bytes + 1024), 2048 / cm->threads), 8));
        st.grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)opt.compute_units * per_cu));
        ir.route += "mixed-ct[N=" + std::to_string(N) + ",T=" + std::to_string(cm->T) + ",n=" + std::to_string(cm->radices.size()) + "] ";
        return MI355FFT_OK;
      }
    }
    const bool stages_win = ((S == 1 && N < 1024 && radices.size() == 3 && radices[0] >= 16) || (S > 1 && N > 512)) && opt.mixed_lines != 2;
    if (opt.mixed_lines && !opt.force_generic && !stages_win && lds_radices.size() >= 2 && lds_radices.size() <= 12 && N <= 4096) {
      const std::vector<int>& radices = lds_radices;
      ns = (int)radices.size();
      // all stages in one launch, T lines per workgroup in LDS (kern_mixed.hpp)
      std::vector<float2h> t;
      Step& st = push(ST_LINES_MIXED);
      int64_t nsp = 1;
      for (int s = 0; s < ns; ++s) {
        const int R = radices[s];
        st.i[MX_RADIX0 + s] = ((int64_t)R << 32) | (int64_t)t.size();       // radix, table offset (elements)
        const size_t off = t.size();
        t.resize(off + (size_t)(R * nsp));
        for (int q = 0; q < R; ++q) for (int64_t k = 0; k < nsp; ++k) t[off + (size_t)(q * nsp + k)] = root_of_unity(q * k, nsp * R);
        nsp *= R;
      }
      // Tile and workgroup shape from the sweeps in profiles/r01_mixed_radix.log: short lines fill a 64 KB pair of buffers
      // (T lines, 256 threads); from N = 512 on one line per workgroup, threads ~ N/8, and as many workgroups per CU as fit.
      // The stage tables ride in LDS when they are small (<= 16 KB); longer ones are read through the caches.
      int64_t T, threads;
      if (opt.mixed_lds_kb > 0) { T = std::max<int64_t>(1, std::min<int64_t>(opt.mixed_lds_kb * 64 / N, 64)); threads = opt.mixed_threads; }
      else if (N < 512 || S > 1) { T = std::max<int64_t>(1, std::min<int64_t>(4096 / N, 64)); threads = 256; }   // strided axes: lanes walk T lines
      else { T = 1; threads = std::max<int64_t>(64, std::min<int64_t>(256, ((N / 8 + 63) / 64) * 64)); }
      const int64_t lds_bytes = 2 * T * (N + (N >> 5) + 1) * 8;          // kern_mixed.hpp mixed_pitch
      const int64_t tw_lds = (int64_t)t.size() * 8 <= 16 * 1024 ? (int64_t)t.size() : 0;
      st.p[P_SRC] = src; st.p[P_DST] = dst; st.p[P_TW] = add_table(t);
      st.i[MX_LINES] = lines; st.i[MX_N] = N; st.i[MX_S] = S; st.i[MX_T] = T; st.i[MX_NST] = ns;
      st.i[MX_SWAP] = inverse ? 1 : 0; st.i[MX_LDS_BYTES] = lds_bytes; st.i[MX_THREADS] = threads; st.i[MX_TW_TOTAL] = tw_lds;
      st.f[F_SCALE] = scale;
      const int64_t tiles = (lines + T - 1) / T;
      const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((160 * 1024) / (lds_bytes + tw_lds * 8 + 1024), 2048 / threads), 8));
      st.grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)opt.compute_units * per_cu));
      ir.route += "mixed-lines[N=" + std::to_string(N) + ",S=" + std::to_string(S) + ",T=" + std::to_string(T) + ",n=" + std::to_string(ns) + "] ";
      return MI355FFT_OK;
    }
    PtrRef w0, w1;
    if (ns >= 2) w0 = alloc_work((uint64_t)lines * N * 8);
    if (ns >= 3) w1 = alloc_work((uint64_t)lines * N * 8);
    int64_t nsp = 1;
    PtrRef cur = src;
    for (int s = 0; s < ns; ++s) {
      const int R = radices[s];
      const bool last = s == ns - 1;
      PtrRef to = last ? dst : ((s % 2 == 0) ? w0 : w1);
      std::vector<float2h> t;
      if (nsp > 1) {
        t.resize((size_t)(R * nsp));
        for (int q = 0; q < R; ++q) for (int64_t k = 0; k < nsp; ++k) t[(size_t)(q * nsp + k)] = root_of_unity(q * k, nsp * R);
      } else t.push_back(float2h{1, 0});
      Step& st = push(ST_STAGE);
      st.variant = R;
      st.p[P_SRC] = cur; st.p[P_DST] = to; st.p[P_TW] = add_table(t);
      st.i[SG_TOTAL] = lines * (N / R); st.i[SG_N] = N; st.i[SG_S] = S; st.i[SG_NSP] = nsp;
      st.i[SG_SWAP_IN] = (inverse && s == 0) ? 1 : 0; st.i[SG_SWAP_OUT] = (inverse && last) ? 1 : 0;
      st.f[F_SCALE] = last ? scale : 1.0f;
      st.grid = generic_grid(st.i[SG_TOTAL]);
      cur = to;
      nsp *= R;
    }
    ir.route += "stages[N=" + std::to_string(N) + ",S=" + std::to_string(S) + ",n=" + std::to_string(ns) + "] ";
    return MI355FFT_OK;
  }

  // Lengths with a prime factor > 13 (large_policy.js:214-228 picks Bluestein/Rader for those): chirp-z through a
  // power-of-two circular convolution of length M >= 2N-1 on the fast routes.  Axes with stride S > 1 are
  // transposed to contiguous lines first (two extra passes; a completeness route, not a tuned one).
  int emit_bluestein(PtrRef src, PtrRef dst, int64_t N, int64_t S, int64_t outer, bool inverse, float scale, std::string& err) {
    const int64_t lines = S * outer;
    if (N > ((int64_t)1 << 22)) { err = "Unsupported: Bluestein axis length " + std::to_string(N) + " exceeds 2^22"; return MI355FFT_ERR_UNSUPPORTED; }
    int64_t M = 1;
    while (M < 2 * N - 1) M <<= 1;
    // chirp a[n] = e^{-i pi n^2/N} = root(n^2 mod 2N, 2N);  B = FFT_M(b), b[n] = conj(a[n]) wrapped (b[M-n] = b[n])
    std::vector<float2h> chirp((size_t)N);
    std::vector<double> br((size_t)M, 0.0), bi((size_t)M, 0.0);
    for (int64_t n = 0; n < N; ++n) {
      const int64_t m = (int64_t)(((unsigned __int128)n * (unsigned __int128)n) % (unsigned __int128)(2 * N));
      const long double ang = -3.14159265358979323846264338327950288L * (long double)m / (long double)N;
      chirp[(size_t)n] = root_of_unity(m, 2 * N);
      const double cr = (double)cosl(ang), ci = (double)sinl(ang);
      br[(size_t)n] = cr; bi[(size_t)n] = -ci;
      if (n > 0) { br[(size_t)(M - n)] = cr; bi[(size_t)(M - n)] = -ci; }
    }
    host_fft_pow2(br, bi);
    std::vector<float2h> bt((size_t)M);
    for (int64_t m = 0; m < M; ++m) bt[(size_t)m] = float2h{(float)br[(size_t)m], (float)bi[(size_t)m]};
    const PtrRef tchirp = add_table(chirp), tb = add_table(bt);
    PtrRef lin_src = src, lin_dst = dst;
    PtrRef tr;   // dense [outer][S][N] copy of a strided axis
    if (S > 1) {
      tr = alloc_work((uint64_t)lines * N * 8);
      Step& g = push(ST_GATHER);     // transpose [outer][N][S] -> [outer][S][N]
      g.p[P_SRC] = src; g.p[P_DST] = tr;
      g.i[GS_TOTAL] = lines * N; g.i[GS_PER] = S * N; g.i[GS_RANK] = 2; g.i[GS_PHYS_OFFSET] = 0; g.i[GS_PHYS_BATCH_STRIDE] = S * N; g.i[GS_DENSE_OFFSET] = 0; g.i[GS_DENSE_BATCH_STRIDE] = S * N;
      g.shape[0] = N; g.shape[1] = S; g.sa[0] = S; g.sa[1] = 1; g.sb[0] = 1; g.sb[1] = N;
      g.grid = generic_grid(g.i[GS_TOTAL]);
      lin_src = tr; lin_dst = tr;
    }
    const PtrRef y = alloc_work((uint64_t)lines * M * 8);
    // r02: with the convolution length on a line kernel the five launches become two — the chirp and the zero-padded embed ride the
    // first-stage loads of the forward launch, the product with the chirp's spectrum its last-stage store (fft_lines_mul_kernel<C, MAPPED>),
    // and the inverse launch multiplies by the chirp and crops to N points in its store pass (fft_lines_mapped_kernel)
    {
      const LineKernelMeta* mf = nullptr;
      if (opt.fuse_views && opt.conv_lines && !opt.force_generic && S == 1 && M >= 64 && M <= opt.max_line && M * 2 < ((int64_t)1 << 31) &&
          !(opt.xcd_fused == 2 && M == 4096))
        mf = find_line_kernel((int)M, false, false, false, false, 0);
      const LineKernelMeta* mi = mf ? find_line_kernel((int)M, false, false, true, true, 0) : nullptr;
      if (mf && mi && mf->lds_bytes > 0 && mf->R1 > 1) {
        const int64_t one[1] = {M};
        SideMap win = dense_map(one, 1);          // N live points of an M-point line, lines N apart
        win.hi[0] = (int)N; win.batch_stride = N; win.ax = 0;
        const SideMap full = dense_map(one, 1);
        const int64_t flags = LINES_CHIRP | (inverse ? LINES_CHIRP_SWAP : 0);
        Step& f = push_lines(*mf, lin_src, y, lines, {1, M}, {1, M}, 1.0f);
        f.p[LP_MUL_SPECTRUM] = tb; f.p[LP_CHIRP] = tchirp;
        f.i[LS_MUL_CONJ] = 0; f.i[LS_CHIRP_FLAGS] = flags; f.i[LS_MODE] = LM_MUL; f.i[LS_MAPPED] = 1;
        f.imap = win; f.omap = full;
        Step& g = push_lines(*mi, y, lin_dst, lines, {1, M}, {1, M}, (float)((double)scale / (double)M));
        g.p[LP_CHIRP] = tchirp;
        g.i[LS_CHIRP_FLAGS] = flags; g.i[LS_MAPPED] = 1;
        g.imap = full; g.omap = win;
        ir.route += "bluestein-lines[N=" + std::to_string(N) + ",M=" + std::to_string(M) + "] ";
        return MI355FFT_OK;
      }
    }
    Step& pre = push(ST_CHIRP_PRE);
    pre.p[P_SRC] = lin_src; pre.p[P_DST] = y; pre.p[CHP_CHIRP] = tchirp;
    pre.i[CH_N] = N; pre.i[CH_M] = M; pre.i[CH_LINES] = lines; pre.i[CH_SWAP_IN] = inverse ? 1 : 0; pre.i[CH_SWAP_OUT] = 0;
    pre.grid = generic_grid(lines * M);
    int rc = emit_axis(y, y, M, 1, lines, false, 1.0f, err);
    if (rc) return rc;
    Step& pm = push(ST_POINTWISE);
    pm.p[P_SRC] = y; pm.p[P_DST] = y; pm.p[PWP_KERNEL] = tb;
    pm.i[PW_L] = M; pm.i[PW_TOTAL] = lines * M; pm.i[PW_CONJ] = 0; pm.f[F_SCALE] = 1.0f;
    pm.grid = generic_grid(lines * M);
    rc = emit_axis(y, y, M, 1, lines, true, 1.0f, err);
    if (rc) return rc;
    Step& post = push(ST_CHIRP_POST);
    post.p[P_SRC] = y; post.p[P_DST] = lin_dst; post.p[CHP_CHIRP] = tchirp;
    post.i[CH_N] = N; post.i[CH_M] = M; post.i[CH_LINES] = lines; post.i[CH_SWAP_IN] = 0; post.i[CH_SWAP_OUT] = inverse ? 1 : 0;
    post.f[F_SCALE] = (float)((double)scale / (double)M);
    post.grid = generic_grid(lines * N);
    if (S > 1) {
      Step& sc = push(ST_SCATTER);   // back to [outer][N][S]
      sc.p[P_SRC] = tr; sc.p[P_DST] = dst;
      sc.i[GS_TOTAL] = lines * N; sc.i[GS_PER] = S * N; sc.i[GS_RANK] = 2; sc.i[GS_PHYS_OFFSET] = 0; sc.i[GS_PHYS_BATCH_STRIDE] = S * N; sc.i[GS_DENSE_OFFSET] = 0; sc.i[GS_DENSE_BATCH_STRIDE] = S * N;
      sc.shape[0] = N; sc.shape[1] = S; sc.sa[0] = S; sc.sa[1] = 1; sc.sb[0] = 1; sc.sb[1] = N;
      sc.grid = generic_grid(sc.i[GS_TOTAL]);
    }
    ir.route += "bluestein[N=" + std::to_string(N) + ",M=" + std::to_string(M) + "] ";
    return MI355FFT_OK;
  }

  // in-place radix-2 FFT in f64 (plan-time tables only)
  static void host_fft_pow2(std::vector<double>& re, std::vector<double>& im) {
    const size_t n = re.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
      size_t bit = n >> 1;
      for (; j & bit; bit >>= 1) j ^= bit;
      j ^= bit;
      if (i < j) { std::swap(re[i], re[j]); std::swap(im[i], im[j]); }
    }
    for (size_t len = 2; len <= n; len <<= 1) {
      const size_t half = len >> 1;
      for (size_t k = 0; k < half; ++k) {
        const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)len;
        const double wr = (double)cosl(ang), wi = (double)sinl(ang);
        for (size_t i = k; i < n; i += len) {
          const size_t j = i + half;
          const double tr = re[j] * wr - im[j] * wi, ti = re[j] * wi + im[j] * wr;
          re[j] = re[i] - tr; im[j] = im[i] - ti;
          re[i] += tr; im[i] += ti;
        }
      }
    }
  }

  // all axes of a dense [batch][shape] complex array, src -> dst
  // axes_mask: bit a set => axis a is transformed (createFftPlan({axes})); 0 => every axis from first_axis on
  // imap / omap (optional): the FIRST transformed axis reads `src` through imap, the LAST one writes `fin` through omap; the
  // passes between work on the dense array at dst.  The caller has checked axis_mappable() for those axes.
  int emit_nd(PtrRef src, PtrRef dst, const int64_t* shape, int rank, int64_t batch, bool inverse, float scale, std::string& err,
              int first_axis = 0, uint32_t axes_mask = 0, const SideMap* imap = nullptr, const SideMap* omap = nullptr, PtrRef fin = PtrRef()) {
    if (imap || omap) {
      int fa, la;
      nd_first_last(shape, rank, axes_mask, fa, la);
      const int64_t total = prodv(shape, rank);
      PtrRef cur = src;
      int64_t S = 1;
      for (int a = 0; a < rank; ++a) {
        const int64_t N = shape[a];
        if (N > 1 && (axes_mask == 0 || ((axes_mask >> a) & 1u))) {
          const int64_t outer = batch * (total / (S * N));
          const bool use_i = a == fa && imap, use_o = a == la && omap;
          const PtrRef wr = use_o ? fin : dst;
          int rc;
          if (use_i || use_o) rc = emit_axis_mapped(cur, wr, N, S, outer, inverse, a == la ? scale : 1.0f, use_i ? *imap : dense_map(shape, rank), use_o ? *omap : dense_map(shape, rank), a);
          else rc = emit_axis(cur, wr, N, S, outer, inverse, a == la ? scale : 1.0f, err);
          if (rc) { if (err.empty()) err = "no line kernel for a mapped axis"; return rc; }
          cur = wr;
        }
        S *= N;
      }
      return MI355FFT_OK;
    }
    PtrRef cur = src;
    int64_t S = 1;
    for (int a = 0; a < first_axis; ++a) S *= shape[a];
    const int64_t total = prodv(shape, rank);
    bool any = false;
    int last_axis = -1;
    const auto wanted = [&](int a) { return axes_mask == 0 || ((axes_mask >> a) & 1u); };
    for (int a = first_axis; a < rank; ++a) if (shape[a] > 1 && wanted(a)) last_axis = a;
    int start = first_axis;
    // axes 0 and 1 of square power-of-two planes in ONE persistent launch (kern_xcd.hpp TWO_D): columns, barrier, rows
    if (first_axis == 0 && rank >= 2 && wanted(0) && wanted(1) &&
        emit_xcd_2d(cur, dst, shape[0], shape[1], batch * (total / (shape[0] * shape[1])), inverse, last_axis == 1 ? scale : 1.0f)) {
      cur = dst; any = true; S = shape[0] * shape[1]; start = 2;
    }
    for (int a = start; a < rank; ++a) {
      const int64_t N = shape[a];
      if (N > 1 && wanted(a)) {
        const int64_t outer = batch * (total / (S * N));
        const int rc = emit_axis(cur, dst, N, S, outer, inverse, a == last_axis ? scale : 1.0f, err);
        if (rc) return rc;
        cur = dst;
        any = true;
      }
      S *= N;
    }
    if (!any) return emit_axis(cur, dst, 1, 1, batch * total, inverse, scale, err);
    return MI355FFT_OK;
  }

  void emit_strided(bool gather, PtrRef phys, PtrRef dense, const mi355fft_side_layout& lay, const int64_t* shape, int rank, int64_t batch,
                    const int64_t* dense_shape, const int64_t* dense_sub_offset, int64_t dense_batch_stride, int64_t extra_phys_offset,
                    bool real_elements = false) {
    Step& st = push(gather ? ST_GATHER : ST_SCATTER);
    st.i[GS_REAL] = real_elements ? 1 : 0;
    st.p[P_SRC] = gather ? phys : dense;
    st.p[P_DST] = gather ? dense : phys;
    const int64_t per = prodv(shape, rank);
    st.i[GS_TOTAL] = batch * per; st.i[GS_PER] = per; st.i[GS_RANK] = rank;
    int64_t dstride = 1, doff = 0, pstride = 1;
    for (int d = 0; d < rank; ++d) {
      st.shape[d] = shape[d];
      st.sa[d] = lay.strided ? lay.strides[d] : pstride;
      st.sb[d] = dstride;
      doff += (dense_sub_offset ? dense_sub_offset[d] : 0) * dstride;
      dstride *= dense_shape[d];
      pstride *= shape[d];
    }
    st.i[GS_PHYS_OFFSET] = (lay.strided ? lay.offset_elements : 0) + extra_phys_offset;
    st.i[GS_PHYS_BATCH_STRIDE] = (lay.strided && lay.batch_stride_elements > 0) ? lay.batch_stride_elements : per;
    st.i[GS_DENSE_OFFSET] = doff;
    st.i[GS_DENSE_BATCH_STRIDE] = dense_batch_stride;
    st.grid = generic_grid(st.i[GS_TOTAL]);
  }
};

double scale_factor(int normalize, bool inverse, double n_total) {  // runtime/common.js:35-40
  if (normalize == MI355FFT_NORM_NONE) return 1.0;
  if (normalize == MI355FFT_NORM_UNITARY) return 1.0 / std::sqrt(n_total);
  return inverse ? 1.0 / n_total : 1.0;
}

// bytes a strided side must cover: offset + (batch-1)*batchStride + sum (shape_d-1)*stride_d + 1 elements
// (runtime/tensor_descriptor.js:113-121)
uint64_t strided_extent_elems(const mi355fft_side_layout& l, const int64_t* shape, int rank, int64_t batch, int64_t extra) {
  int64_t last = l.offset_elements + extra + (batch - 1) * (l.batch_stride_elements > 0 ? l.batch_stride_elements : prodv(shape, rank));
  for (int d = 0; d < rank; ++d) last += (shape[d] - 1) * l.strides[d];
  return (uint64_t)(last + 1);
}

int validate_common(const mi355fft_plan_desc& d, std::string& err) {
  if (d.struct_size != sizeof(mi355fft_plan_desc)) { err = "mi355fft_plan_desc.struct_size mismatch (ABI)"; return MI355FFT_ERR_INVALID; }
  if (d.rank < 1 || d.rank > MI355FFT_MAX_RANK) { err = "shape must be an array of one or more positive dimensions"; return MI355FFT_ERR_INVALID; }
  for (int i = 0; i < d.rank; ++i)
    if (d.shape[i] <= 0) { err = "shape elements must be positive ints"; return MI355FFT_ERR_INVALID; }
  if (d.batch <= 0) { err = "batch must be positive int; got " + std::to_string(d.batch); return MI355FFT_ERR_INVALID; }
  if (d.normalize < 0 || d.normalize > 2) { err = "normalize must be one of \"none\", \"backward\", \"unitary\""; return MI355FFT_ERR_INVALID; }
  if (prodv(d.shape, d.rank) * d.batch > ((int64_t)1 << 40)) { err = "Unsupported: more than 2^40 points in one plan"; return MI355FFT_ERR_UNSUPPORTED; }
  if (d.precision != MI355FFT_PRECISION_F32 && d.precision != MI355FFT_PRECISION_F16_STORAGE) {
    err = "precision must be one of \"f32\", \"f16-storage\""; return MI355FFT_ERR_INVALID;
  }
  for (const mi355fft_side_layout* l : {&d.input, &d.output})
    if (l->strided)
      for (int i = 0; i < d.rank; ++i)
        if (l->strides[i] <= 0) { err = "layout strides must be positive ints"; return MI355FFT_ERR_INVALID; }
  // mi355fft_side_layout.reserved: fftConv.inputChannels on the input side of the two fftconv types, zero everywhere else
  const bool conv = d.type == MI355FFT_FFTCONV || d.type == MI355FFT_FFTCONV_REAL;
  if (d.output.reserved != 0 || (!conv && d.input.reserved != 0)) {
    err = "mi355fft_side_layout.reserved must be 0 (it carries fftConv.inputChannels on the input side of fftconv plans only)"; return MI355FFT_ERR_INVALID;
  }
  if (conv && d.input.reserved < 0) { err = "fftConv.inputChannels must be a positive integer; got " + std::to_string(d.input.reserved); return MI355FFT_ERR_INVALID; }
  // mi355fft_zero_range.reserved: fftConv.groups in zero_read of the two fftconv types (whether or not the range is enabled), zero everywhere else
  if (d.zero_write.reserved != 0 || (!conv && d.zero_read.reserved != 0)) {
    err = "mi355fft_zero_range.reserved must be 0 (it carries fftConv.groups in zero_read of fftconv plans only)"; return MI355FFT_ERR_INVALID;
  }
  if (conv && d.zero_read.reserved < 0) { err = "fftConv.groups must be a positive integer; got " + std::to_string(d.zero_read.reserved); return MI355FFT_ERR_INVALID; }
  return MI355FFT_OK;
}

// intersection of the view box [off, off+vshape) with the logical domain [0, lshape): region extent, its start in
// logical coordinates and in view coordinates.  false when empty.
bool view_region(const mi355fft_io_view& v, const int64_t* lshape, int rank, int64_t* ext, int64_t* lstart, int64_t* vstart) {
  for (int i = 0; i < rank; ++i) {
    const int64_t s = std::max<int64_t>(0, v.offset[i]), e = std::min<int64_t>(lshape[i], v.offset[i] + v.shape[i]);
    if (e <= s) return false;
    ext[i] = e - s; lstart[i] = s; vstart[i] = s - v.offset[i];
  }
  return true;
}

void emit_zero_outside(Builder& b, PtrRef data, const mi355fft_zero_range& z, const int64_t* shape, int rank, int64_t batch, bool real = false) {
  Step& st = b.push(ST_ZERO_OUTSIDE);
  st.p[P_DATA] = data; st.i[ZO_REAL] = real ? 1 : 0;
  const int64_t per = prodv(shape, rank);
  st.i[ZO_TOTAL] = per * batch; st.i[ZO_PER] = per; st.i[ZO_RANK] = rank;
  for (int i = 0; i < rank; ++i) { st.shape[i] = shape[i]; st.sa[i] = z.start[i]; st.sb[i] = z.end[i]; }
  st.grid = b.generic_grid(st.i[ZO_TOTAL]);
}

int validate_views(const mi355fft_plan_desc& d, std::string& err, const int64_t* read_shape = nullptr, const int64_t* write_shape = nullptr) {
  for (const mi355fft_io_view* v : {&d.io_input, &d.io_output})
    if (v->enabled)
      for (int i = 0; i < d.rank; ++i)
        if (v->shape[i] <= 0) { err = "ioView shape must be an array of positive ints"; return MI355FFT_ERR_INVALID; }
  const char* names[2] = {"zeroPad.read", "zeroPad.write"};
  const int64_t* shapes[2] = {read_shape ? read_shape : d.shape, write_shape ? write_shape : d.shape};   // r2c writes / c2r reads the PACKED domain
  int k = 0;
  for (const mi355fft_zero_range* z : {&d.zero_read, &d.zero_write}) {
    if (z->enabled)
      for (int i = 0; i < d.rank; ++i) {
        if (z->start[i] < 0 || z->end[i] < 0 || z->start[i] > z->end[i] || z->end[i] > shapes[k][i]) {
          err = std::string(names[k]) + ": need 0 <= start[" + std::to_string(i) + "] <= end[" + std::to_string(i) + "] <= shape[" + std::to_string(i) + "]";
          return MI355FFT_ERR_INVALID;
        }
      }
    ++k;
  }
  return MI355FFT_OK;
}

// ---- a side of a plan as an address map over its logical domain (kern_lines.hpp side_line) ----
// Input side: element i of the logical domain `lshape` is read at offset + sum (i_d - viewOffset_d) * stride_d inside the box where
// the ioView.input window, the logical domain and the zeroPad.read range meet, and is zero elsewhere.
SideMap input_side_map(const mi355fft_plan_desc& d, const int64_t* lshape, int rank) {
  const bool vin = d.io_input.enabled != 0;
  const int64_t* ishape = vin ? d.io_input.shape : lshape;
  SideMap m = Builder::dense_map(lshape, rank);
  int64_t dense = 1;
  for (int i = 0; i < rank; ++i) {
    m.stride[i] = d.input.strided ? d.input.strides[i] : dense;
    dense *= ishape[i];
    const int64_t voff = vin ? d.io_input.offset[i] : 0;
    int64_t lo = std::max<int64_t>(0, voff), hi = vin ? std::min<int64_t>(lshape[i], voff + d.io_input.shape[i]) : lshape[i];
    if (d.zero_read.enabled) { lo = std::max(lo, d.zero_read.start[i]); hi = std::min(hi, d.zero_read.end[i]); }
    if (hi < lo) hi = lo;
    m.lo[i] = (int)lo; m.hi[i] = (int)hi;
    m.offset -= voff * m.stride[i];
  }
  m.offset += d.input.strided ? d.input.offset_elements : 0;
  m.batch_stride = d.input.strided && d.input.batch_stride_elements > 0 ? d.input.batch_stride_elements : dense;
  return m;
}
// Output side: element i is written inside the ioView.output window only, as zero outside the zeroPad.write range.
SideMap output_side_map(const mi355fft_plan_desc& d, const int64_t* lshape, int rank) {
  const bool vout = d.io_output.enabled != 0;
  const int64_t* oshape = vout ? d.io_output.shape : lshape;
  SideMap m = Builder::dense_map(lshape, rank);
  int64_t dense = 1;
  for (int i = 0; i < rank; ++i) {
    m.stride[i] = d.output.strided ? d.output.strides[i] : dense;
    dense *= oshape[i];
    const int64_t voff = vout ? d.io_output.offset[i] : 0;
    int64_t lo = std::max<int64_t>(0, voff), hi = vout ? std::min<int64_t>(lshape[i], voff + d.io_output.shape[i]) : lshape[i];
    if (hi < lo) hi = lo;
    m.lo[i] = (int)lo; m.hi[i] = (int)hi;
    if (d.zero_write.enabled) { m.zlo[i] = (int)d.zero_write.start[i]; m.zhi[i] = (int)d.zero_write.end[i]; }
    m.offset -= voff * m.stride[i];
  }
  m.offset += d.output.strided ? d.output.offset_elements : 0;
  m.batch_stride = d.output.strided && d.output.batch_stride_elements > 0 ? d.output.batch_stride_elements : dense;
  return m;
}
uint64_t side_bytes(const mi355fft_side_layout& lay, const mi355fft_io_view& view, const int64_t* lshape, int rank, int64_t batch, int64_t elem) {
  const int64_t* pshape = view.enabled ? view.shape : lshape;
  return lay.strided ? strided_extent_elems(lay, pshape, rank, batch, 0) * elem : (uint64_t)prodv(pshape, rank) * batch * elem;
}

// ---- the two sides of a plan that its launches cannot map (c2c, r2c, c2r and the trig plans; real or complex elements) ----
// Input: strided layout, ioView.input (embed into the zero-filled logical domain) and zeroPad.read produce a dense logical
// array in the workspace; a plain dense input is used where it lies.  In place (c2c only, where nothing but zeroPad.read can be
// asked for) the range is zeroed in the caller's buffer itself.
PtrRef stage_side_input(const mi355fft_plan_desc& d, Builder& b, PtrRef in, const int64_t* lshape, bool real, uint64_t& in_bytes) {
  const int rank = d.rank;
  const int64_t elem = real ? 4 : 8, n = prodv(lshape, rank);
  const bool vin = d.io_input.enabled != 0;
  const int64_t* ishape = vin ? d.io_input.shape : lshape;
  const int64_t in_n = prodv(ishape, rank);
  in_bytes = d.input.strided ? strided_extent_elems(d.input, ishape, rank, d.batch, 0) * elem : (uint64_t)in_n * d.batch * elem;
  if (!(d.input.strided || vin || d.zero_read.enabled)) return in;
  const PtrRef src = d.in_place ? in : b.alloc_work((uint64_t)n * d.batch * elem);
  if (vin) {
    int64_t ext[8], ls[8], vs[8];
    const bool any = view_region(d.io_input, lshape, rank, ext, ls, vs);
    bool covers = any;
    for (int i = 0; any && i < rank; ++i) covers = covers && ext[i] == lshape[i];
    if (!covers) b.zero(src, n * d.batch * (elem / 4));
    if (any) {
      mi355fft_side_layout lay = d.input;
      int64_t vstride = 1, poff = 0;
      for (int i = 0; i < rank; ++i) { poff += vs[i] * (lay.strided ? lay.strides[i] : vstride); vstride *= ishape[i]; }
      if (!lay.strided) { lay.strided = 1; int64_t st = 1; for (int i = 0; i < rank; ++i) { lay.strides[i] = st; st *= ishape[i]; } lay.offset_elements = 0; lay.batch_stride_elements = in_n; }
      else if (lay.batch_stride_elements <= 0) lay.batch_stride_elements = in_n;
      b.emit_strided(true, in, src, lay, ext, rank, d.batch, lshape, ls, n, poff, real);
    }
    b.ir.route += "embed ";
  } else if (d.input.strided) {
    b.emit_strided(true, in, src, d.input, lshape, rank, d.batch, lshape, nullptr, n, 0, real);
    b.ir.route += "gather ";
  } else if (!d.in_place) {
    Step& c = b.push(ST_COPY); c.p[P_SRC] = in; c.p[P_DST] = src; c.i[S_COUNT] = n * d.batch * elem;
  }
  if (d.zero_read.enabled) { emit_zero_outside(b, src, d.zero_read, lshape, rank, d.batch, real); b.ir.route += "zero-read "; }
  return src;
}
// Output: where the transform should write (the caller's buffer, or a dense logical staging array when a strided layout /
// ioView.output follows), and the steps that finish the side afterwards.
PtrRef side_output_target(const mi355fft_plan_desc& d, Builder& b, PtrRef out, const int64_t* lshape, bool real, uint64_t& out_bytes) {
  const int rank = d.rank;
  const int64_t elem = real ? 4 : 8;
  const int64_t* oshape = d.io_output.enabled ? d.io_output.shape : lshape;
  out_bytes = d.output.strided ? strided_extent_elems(d.output, oshape, rank, d.batch, 0) * elem : (uint64_t)prodv(oshape, rank) * d.batch * elem;
  if (d.output.strided || d.io_output.enabled) return b.alloc_work((uint64_t)prodv(lshape, rank) * d.batch * elem);
  return out;
}
int finish_side_output(const mi355fft_plan_desc& d, Builder& b, PtrRef out, PtrRef dst, const int64_t* lshape, bool real, std::string& err) {
  const int rank = d.rank;
  const int64_t elem = real ? 4 : 8, n = prodv(lshape, rank);
  if (d.zero_write.enabled) { emit_zero_outside(b, dst, d.zero_write, lshape, rank, d.batch, real); b.ir.route += "zero-write "; }
  if (d.io_output.enabled) {
    const int64_t* oshape = d.io_output.shape;
    const int64_t out_n = prodv(oshape, rank);
    if (d.io_output.clear_outside) {
      if (d.output.strided) { err = "Unsupported: ioView.output.clearOutside with a strided output layout"; return MI355FFT_ERR_UNSUPPORTED; }
      b.zero(out, out_n * d.batch * (elem / 4));
    }
    int64_t ext[8], ls[8], vs[8];
    if (view_region(d.io_output, lshape, rank, ext, ls, vs)) {
      mi355fft_side_layout lay = d.output;
      int64_t vstride = 1, poff = 0;
      for (int i = 0; i < rank; ++i) { poff += vs[i] * (lay.strided ? lay.strides[i] : vstride); vstride *= oshape[i]; }
      if (!lay.strided) { lay.strided = 1; int64_t st = 1; for (int i = 0; i < rank; ++i) { lay.strides[i] = st; st *= oshape[i]; } lay.offset_elements = 0; lay.batch_stride_elements = out_n; }
      else if (lay.batch_stride_elements <= 0) lay.batch_stride_elements = out_n;
      b.emit_strided(false, out, dst, lay, ext, rank, d.batch, lshape, ls, n, poff, real);
    }
    b.ir.route += "extract ";
  } else if (d.output.strided) {
    b.emit_strided(false, out, dst, d.output, lshape, rank, d.batch, lshape, nullptr, n, 0, real);
    b.ir.route += "scatter ";
  }
  return MI355FFT_OK;
}

int build_c2c(const mi355fft_plan_desc& d, Builder& b, std::string& err) {
  if (d.direction != MI355FFT_FORWARD && d.direction != MI355FFT_INVERSE) { err = "direction must be one of \"forward\", \"inverse\""; return MI355FFT_ERR_INVALID; }
  int rc = validate_views(d, err);
  if (rc) return rc;
  const bool inverse = d.direction == MI355FFT_INVERSE;
  const int rank = d.rank;
  const int64_t n = prodv(d.shape, rank);
  const float scale = (float)scale_factor(d.normalize, inverse, (double)n);
  const bool vin = d.io_input.enabled != 0, vout = d.io_output.enabled != 0;
  if (d.in_place && (vin || vout || d.input.strided || d.output.strided)) { err = "inPlace=true cannot be combined with ioView or strided layouts"; return MI355FFT_ERR_INVALID; }
  const int64_t out_n = prodv(vout ? d.io_output.shape : d.shape, rank);     // physical elements of an output item
  PtrRef in(BUF_INPUT, 0), out(d.in_place ? BUF_INPUT : BUF_OUTPUT, 0);
  b.ir.in_bytes = side_bytes(d.input, d.io_input, d.shape, rank, d.batch, 8);
  b.ir.out_bytes = side_bytes(d.output, d.io_output, d.shape, rank, d.batch, 8);
  if (d.axes_mask >> rank) { err = "Invalid axis in axes for rank " + std::to_string(rank); return MI355FFT_ERR_INVALID; }
  if (vout && d.io_output.clear_outside && d.output.strided) { err = "Unsupported: ioView.output.clearOutside with a strided output layout"; return MI355FFT_ERR_UNSUPPORTED; }

  // ---- rank-1 lane layouts: unit stride along the line on both sides -> one launch, no staging ----
  if (rank == 1 && !vin && !vout && !d.zero_read.enabled && !d.zero_write.enabled && !d.in_place && (d.input.strided || d.output.strided) &&
      (!d.input.strided || d.input.strides[0] == 1) && (!d.output.strided || d.output.strides[0] == 1)) {
    const int64_t ip = d.input.strided && d.input.batch_stride_elements > 0 ? d.input.batch_stride_elements : n;
    const int64_t op = d.output.strided && d.output.batch_stride_elements > 0 ? d.output.batch_stride_elements : n;
    const int64_t ioff = d.input.strided ? d.input.offset_elements : 0, ooff = d.output.strided ? d.output.offset_elements : 0;
    // the line kernels address a tile with 32-bit element offsets: T lines * pitch must stay below 2^31 elements
    if (ip >= n && op >= n && ip < ((int64_t)1 << 24) && op < ((int64_t)1 << 24) &&
        b.emit_lines_pitched(in.plus(ioff * 8), out.plus(ooff * 8), n, d.batch, inverse, scale, ip, op))
      return MI355FFT_OK;
    // four-step sizes (r03): the fused kernels take the two pitches as they are — channel lanes and whdcn layouts of long lines need
    // no gather / scatter either.  Any other route of emit_axis would ignore the pitches: it is rolled back and the staging path taken.
    if (ip >= n && op >= n && n > b.opt.max_line && is_pow2(n) && b.opt.fuse_views && !b.opt.force_generic) {
      const size_t mark = b.ir.steps.size();
      const std::string route_mark = b.ir.route;
      const uint64_t work_mark = b.work_top, work_bytes_mark = b.ir.work_bytes;
      b.lane_in_pitch = ip; b.lane_out_pitch = op; b.lane_used = false;
      const int rcl = b.emit_axis(in.plus(ioff * 8), out.plus(ooff * 8), n, 1, d.batch, inverse, scale, err);
      b.lane_in_pitch = b.lane_out_pitch = 0;
      if (rcl == MI355FFT_OK && b.lane_used) { b.ir.route += "lanes[pitch=" + std::to_string(ip) + "/" + std::to_string(op) + "] "; return MI355FFT_OK; }
      b.ir.steps.resize(mark); b.ir.route = route_mark; b.work_top = work_mark; b.ir.work_bytes = work_bytes_mark; err.clear();
    }
  }

  // ---- rank-1 views of a four-step line with a VIEW instance (r03): ranges as predicates of the fused kernel's loads and stores ----
  if (rank == 1 && !d.in_place && (d.axes_mask == 0 || d.axes_mask == 1) && n > b.opt.max_line && (vin || vout || d.zero_read.enabled || d.zero_write.enabled)) {
    const SideMap im = input_side_map(d, d.shape, 1), om = output_side_map(d, d.shape, 1);
    if (im.stride[0] == 1 && om.stride[0] == 1 && n < ((int64_t)1 << 30)) {
      const size_t mark = b.ir.steps.size();
      if (vout && d.io_output.clear_outside) b.zero(out, out_n * d.batch * 2);
      if (b.emit_xcd_view(in, out, n, d.batch, inverse, scale, im, om)) return MI355FFT_OK;
      b.ir.steps.resize(mark);
    }
  }

  // ---- sides fused into the line kernels: where the first / last transformed axis runs as a line-kernel
  // launch, that side's strided layout, ioView and zero range become the launch's address map (kern_lines.hpp
  // fft_lines_mapped_kernel) — no gather / embed / zero / extract / scatter pass and no staging copy of the array
  int fa = -1, la = -1;
  Builder::nd_first_last(d.shape, rank, d.axes_mask, fa, la);
  const auto stride_below = [&](int a) { int64_t S = 1; for (int i = 0; i < a; ++i) S *= d.shape[i]; return S; };
  const bool need_in = d.input.strided || vin || d.zero_read.enabled;
  const bool need_out = d.output.strided || vout || d.zero_write.enabled;
  const bool small = n < ((int64_t)1 << 31);
  const bool fuse_in = need_in && small && fa >= 0 && b.axis_mappable(d.shape[fa], stride_below(fa), inverse);
  const bool fuse_out = need_out && small && la >= 0 && b.axis_mappable(d.shape[la], stride_below(la), inverse);
  SideMap imap, omap;
  if (fuse_in) imap = input_side_map(d, d.shape, rank);
  if (fuse_out) omap = output_side_map(d, d.shape, rank);

  // ---- input side: dense logical staging when anything but a plain dense read is asked for and the first pass cannot map it ----
  const PtrRef src = fuse_in ? in : stage_side_input(d, b, in, d.shape, false, b.ir.in_bytes);
  const bool stage_in = !src.same(in);

  // ---- transform ----
  // dst: the dense array the passes work on.  A staged or mapped output side needs one that is not the caller's output: the
  // input staging if there is one, else workspace — except when a single pass maps both sides (in -> out directly).
  const bool stage_out = !fuse_out && (d.output.strided || vout);
  PtrRef dst = out;
  if (stage_out || (fuse_out && (d.output.strided || vout) && !(fuse_in && fa == la))) dst = stage_in ? src : b.alloc_work((uint64_t)n * d.batch * 8);
  if (fuse_out && vout && d.io_output.clear_outside) b.zero(out, out_n * d.batch * 2);   // view elements outside the logical domain: zeroed before the store pass
  rc = b.emit_nd(src, dst, d.shape, rank, d.batch, inverse, scale, err, 0, d.axes_mask, fuse_in ? &imap : nullptr, fuse_out ? &omap : nullptr, out);
  if (rc) return rc;
  if (fuse_out) return MI355FFT_OK;
  return finish_side_output(d, b, out, dst, d.shape, false, err);
}

// r2c along axis 0 (packed P = N/2+1 bins), then c2c along the remaining axes of the packed array
int build_r2c(const mi355fft_plan_desc& d, Builder& b, std::string& err) {
  if (d.direction != MI355FFT_FORWARD) { err = "r2c supports direction:\"forward\" only"; return MI355FFT_ERR_INVALID; }
  if (d.in_place) { err = "inPlace=true is supported only on c2c"; return MI355FFT_ERR_INVALID; }
  const int64_t N = d.shape[0], P = N / 2 + 1;
  if (N < 2) { err = "r2c requires shape[0] >= 2"; return MI355FFT_ERR_INVALID; }
  const int64_t n = prodv(d.shape, d.rank), lines = d.batch * (n / N);
  const float scale = (float)scale_factor(d.normalize, false, (double)n);
  int64_t pshape[MI355FFT_MAX_RANK];
  for (int i = 0; i < d.rank; ++i) pshape[i] = d.shape[i];
  pshape[0] = P;
  // ioView.input / zeroPad.read live on the real logical domain, ioView.output / zeroPad.write on the packed one (r2c.js:72-123)
  if (int rv = validate_views(d, err, d.shape, pshape)) return rv;
  const PtrRef user_in(BUF_INPUT, 0), user_out(BUF_OUTPUT, 0);
  const int rank = d.rank;
  // ---- sides fused into the launches: the real side rides the r2c line kernel's first loads, the packed
  // side its store pass (rank 1) or the store pass of the last c2c axis (rank > 1); whatever cannot be mapped is staged as before
  const bool need_in = d.input.strided || d.io_input.enabled || d.zero_read.enabled;
  const bool need_out = d.output.strided || d.io_output.enabled || d.zero_write.enabled;
  const uint32_t upper = rank > 1 ? (((uint32_t)1 << rank) - 1u) & ~1u : 0u;
  int fa = -1, la = -1;
  if (rank > 1) Builder::nd_first_last(pshape, rank, upper, fa, la);
  const bool small = n * 2 < ((int64_t)1 << 31);
  const bool lines0 = small && b.lines_r2c_kernel(N, false, true) != nullptr;     // axis 0 can be the mapped line kernel
  const auto stride_below = [&](int a) { int64_t S = 1; for (int i = 0; i < a; ++i) S *= pshape[i]; return S; };
  const bool fuse_in = need_in && lines0;
  const bool fuse_out = need_out && small && (la >= 1 ? b.axis_mappable(pshape[la], stride_below(la), false) : lines0);
  if (fuse_out && d.io_output.enabled && d.io_output.clear_outside && d.output.strided) { err = "Unsupported: ioView.output.clearOutside with a strided output layout"; return MI355FFT_ERR_UNSUPPORTED; }
  const bool map0 = fuse_in || (fuse_out && la < 1);                              // the axis-0 launch carries at least one map
  b.ir.out_bytes = side_bytes(d.output, d.io_output, pshape, rank, d.batch, 8);
  PtrRef in = user_in;
  if (fuse_in) b.ir.in_bytes = side_bytes(d.input, d.io_input, d.shape, rank, d.batch, 4);
  else in = stage_side_input(d, b, user_in, d.shape, true, b.ir.in_bytes);
  // the dense packed array the passes work on: the caller's output unless a strided layout / ioView follows (staged or mapped)
  PtrRef out = (d.output.strided || d.io_output.enabled) ? b.alloc_work((uint64_t)lines * P * 8) : user_out;
  const SideMap omap = fuse_out ? output_side_map(d, pshape, rank) : SideMap();
  if (fuse_out && d.io_output.enabled && d.io_output.clear_outside) b.zero(user_out, prodv(d.io_output.shape, rank) * d.batch * 2);   // view elements outside the logical domain: zeroed before the store pass
  if (map0) {
    const SideMap im = fuse_in ? input_side_map(d, d.shape, rank) : Builder::dense_map(d.shape, rank);
    const bool store0 = fuse_out && la < 1;
    const SideMap om = store0 ? omap : Builder::dense_map(pshape, rank);
    if (!b.emit_lines_r2c(in, store0 ? user_out : out, N, lines, scale, false, 0, &im, &om)) { err = "no mapped r2c line kernel"; return MI355FFT_ERR_UNSUPPORTED; }
    if (store0) return MI355FFT_OK;
  } else if (N % 2 == 0) {
    const int rc = b.emit_r2c_even(in, out, N, lines, scale, err);
    if (rc) return rc;
  } else {
    PtrRef full = b.alloc_work((uint64_t)lines * N * 8);
    Step& e = b.push(ST_REAL_TO_COMPLEX);
    e.p[P_SRC] = in; e.p[P_DST] = full; e.i[S_COUNT] = lines * N; e.grid = b.generic_grid(lines * N);
    int rc = b.emit_axis(full, full, N, 1, lines, false, 1.0f, err);
    if (rc) return rc;
    Step& p = b.push(ST_PACK_HALF);
    p.p[P_SRC] = full; p.p[P_DST] = out; p.i[PH_N] = N; p.i[PH_P] = P; p.i[PH_BATCH] = lines; p.i[PH_PACKED_STRIDE] = P; p.f[F_SCALE] = scale;
    p.grid = b.generic_grid(lines * P);
    b.ir.route += "r2c-full ";
  }
  if (rank > 1) {
    const bool last_mapped = fuse_out && la >= 1;
    const int rc = last_mapped ? b.emit_nd(out, out, pshape, rank, d.batch, false, 1.0f, err, 1, upper, nullptr, &omap, user_out)
                               : b.emit_nd(out, out, pshape, rank, d.batch, false, 1.0f, err, 1);
    if (rc) return rc;
    if (last_mapped) return MI355FFT_OK;
  }
  return finish_side_output(d, b, user_out, out, pshape, false, err);
}

int build_c2r(const mi355fft_plan_desc& d, Builder& b, std::string& err) {
  if (d.direction != MI355FFT_INVERSE) { err = "c2r supports direction:\"inverse\" only"; return MI355FFT_ERR_INVALID; }
  if (d.in_place) { err = "inPlace=true is supported only on c2c"; return MI355FFT_ERR_INVALID; }
  const int64_t N = d.shape[0], P = N / 2 + 1;
  if (N < 2) { err = "c2r requires shape[0] >= 2"; return MI355FFT_ERR_INVALID; }
  const int64_t n = prodv(d.shape, d.rank), lines = d.batch * (n / N);
  const float scale = (float)scale_factor(d.normalize, true, (double)n);
  int64_t pshape[MI355FFT_MAX_RANK];
  for (int i = 0; i < d.rank; ++i) pshape[i] = d.shape[i];
  pshape[0] = P;
  // ioView.input / zeroPad.read live on the packed domain, ioView.output / zeroPad.write on the real one (c2r.js:168-220)
  if (int rv = validate_views(d, err, pshape, d.shape)) return rv;
  const PtrRef user_in(BUF_INPUT, 0), user_out(BUF_OUTPUT, 0);
  const int rank = d.rank;
  // ---- sides fused into the launches (as build_r2c): the packed side rides the first inverse c2c axis (rank > 1) or the c2r line
  // kernel's pre-split loads (rank 1), the real side the c2r line kernel's store pass
  const bool need_in = d.input.strided || d.io_input.enabled || d.zero_read.enabled;
  const bool need_out = d.output.strided || d.io_output.enabled || d.zero_write.enabled;
  const uint32_t upper = rank > 1 ? (((uint32_t)1 << rank) - 1u) & ~1u : 0u;
  int fa = -1, la = -1;
  if (rank > 1) Builder::nd_first_last(pshape, rank, upper, fa, la);
  const bool small = n * 2 < ((int64_t)1 << 31);
  const bool lines0 = small && b.lines_r2c_kernel(N, true, true) != nullptr;
  const auto stride_below = [&](int a) { int64_t S = 1; for (int i = 0; i < a; ++i) S *= pshape[i]; return S; };
  const bool fuse_in = need_in && small && (fa >= 1 ? b.axis_mappable(pshape[fa], stride_below(fa), true) : lines0);
  const bool fuse_out = need_out && lines0;
  if (fuse_out && d.io_output.enabled && d.io_output.clear_outside && d.output.strided) { err = "Unsupported: ioView.output.clearOutside with a strided output layout"; return MI355FFT_ERR_UNSUPPORTED; }
  const bool map0 = fuse_out || (fuse_in && fa < 1);
  b.ir.out_bytes = side_bytes(d.output, d.io_output, d.shape, rank, d.batch, 4);
  PtrRef in = user_in;
  if (fuse_in) b.ir.in_bytes = side_bytes(d.input, d.io_input, pshape, rank, d.batch, 8);
  else in = stage_side_input(d, b, user_in, pshape, false, b.ir.in_bytes);
  const SideMap imap = fuse_in ? input_side_map(d, pshape, rank) : SideMap();
  PtrRef out = user_out;
  if ((d.output.strided || d.io_output.enabled) && !fuse_out) out = b.alloc_work((uint64_t)n * d.batch * 4);
  PtrRef packed = in;
  bool in_mapped_done = false;
  if (fa >= 1) {
    // inverse c2c over axes 1.. of the packed spectrum, out of place into the workspace: the caller's input is not modified
    packed = b.alloc_work((uint64_t)lines * P * 8);
    const bool first_mapped = fuse_in;
    const int rc = first_mapped ? b.emit_nd(in, packed, pshape, rank, d.batch, true, 1.0f, err, 1, upper, &imap, nullptr)
                                : b.emit_nd(in, packed, pshape, rank, d.batch, true, 1.0f, err, 1);
    if (rc) return rc;
    in_mapped_done = first_mapped;
  }
  if (fuse_out && d.io_output.enabled && d.io_output.clear_outside) b.zero(user_out, prodv(d.io_output.shape, rank) * d.batch);
  if (map0) {
    const SideMap im = (fuse_in && !in_mapped_done) ? imap : Builder::dense_map(pshape, rank);
    const SideMap om = fuse_out ? output_side_map(d, d.shape, rank) : Builder::dense_map(d.shape, rank);
    if (!b.emit_lines_r2c(packed, out, N, lines, scale, true, 0, &im, &om)) { err = "no mapped c2r line kernel"; return MI355FFT_ERR_UNSUPPORTED; }
    if (fuse_out) return MI355FFT_OK;
  } else if (N % 2 == 0) {
    const int rc = b.emit_c2r_even(packed, out, N, lines, scale, err);
    if (rc) return rc;
  } else {
    PtrRef full = b.alloc_work((uint64_t)lines * N * 8);
    Step& u = b.push(ST_UNPACK_HERM);
    u.p[P_SRC] = packed; u.p[P_DST] = full; u.i[PH_N] = N; u.i[PH_P] = P; u.i[PH_BATCH] = lines; u.i[PH_PACKED_STRIDE] = P;
    u.grid = b.generic_grid(lines * N);
    int rc = b.emit_axis(full, full, N, 1, lines, true, 1.0f, err);
    if (rc) return rc;
    Step& r = b.push(ST_COMPLEX_TO_REAL);
    r.p[P_SRC] = full; r.p[P_DST] = out; r.i[S_COUNT] = lines * N; r.f[F_SCALE] = scale;
    r.grid = b.generic_grid(lines * N);
    b.ir.route += "c2r-full ";
  }
  if (int rv = finish_side_output(d, b, user_out, out, d.shape, true, err)) return rv;
  return MI355FFT_OK;
}

// DCT-I..IV / DST-I..IV over real buffers (dct_fft.js): per axis a pre-pass into complex lines of length L, the complex FFT
// of those lines, a post-pass back into the real array (kern_trig.hpp); one scale by normalizeScaleFactor(prod(shape)) folded
// into the last post-pass (dct_fft.js:882).  Layout strides, ioView and zeroPad ride the same side staging as r2c / c2r.
int build_trig(const mi355fft_plan_desc& d, Builder& b, std::string& err) {
  if (d.direction != MI355FFT_FORWARD && d.direction != MI355FFT_INVERSE) { err = "direction must be one of \"forward\", \"inverse\""; return MI355FFT_ERR_INVALID; }
  if (d.in_place) { err = "DCT/DST inPlace is not supported in current implementation"; return MI355FFT_ERR_INVALID; }
  const int rank = d.rank;
  for (int i = 0; i < rank; ++i) if (d.shape[i] < 2) { err = "All DCT/DST dimensions must be >= 2"; return MI355FFT_ERR_INVALID; }
  if (int rv = validate_views(d, err)) return rv;
  const bool fwd = d.direction == MI355FFT_FORWARD;
  int kind;
  switch (d.type) {                                     // dct_fft.js:48-57
    case MI355FFT_DCT1: kind = TK_DCT1; break;
    case MI355FFT_DCT2: kind = fwd ? TK_DCT2_FWD : TK_DCT2_INV; break;
    case MI355FFT_DCT3: kind = fwd ? TK_DCT2_INV : TK_DCT2_FWD; break;
    case MI355FFT_DCT4: kind = TK_DCT4; break;
    case MI355FFT_DST1: kind = TK_DST1; break;
    case MI355FFT_DST2: kind = fwd ? TK_DST2_FWD : TK_DST2_INV; break;
    case MI355FFT_DST3: kind = fwd ? TK_DST2_INV : TK_DST2_FWD; break;
    default: kind = TK_DST4; break;
  }
  const int64_t n = prodv(d.shape, rank);
  const float scale = (float)scale_factor(d.normalize, !fwd, (double)n);
  const PtrRef user_out(BUF_OUTPUT, 0);
  PtrRef cur = stage_side_input(d, b, PtrRef(BUF_INPUT, 0), d.shape, true, b.ir.in_bytes);
  const PtrRef dst = side_output_target(d, b, user_out, d.shape, true, b.ir.out_bytes);
  int64_t S = 1;
  int general_axes = 0;
  for (int a = 0; a < rank; ++a) {
    const int64_t N = d.shape[a], lines = d.batch * (n / N);
    const int64_t L = kind == TK_DCT1 ? 2 * (N - 1) : (kind == TK_DST1 ? 2 * (N + 1) : 2 * N);
    const uint64_t mark = b.work_top;
    if (b.opt.trig_real && !b.opt.force_generic && N >= 4 && (N % 2 == 0 || kind == TK_DCT1 || kind == TK_DST1)) {
      // dense lines: a real FFT of length N behind Makhoul's permutation (dct2/dst2 and their inverses), a complex FFT of
      // length N/2 (dct4/dst4), or the r2c of the real even/odd extension (dct1/dst1) -- kern_trig.hpp kinds TK_REAL..
      const bool tfwd = kind == TK_DCT2_FWD || kind == TK_DST2_FWD, tinv = kind == TK_DCT2_INV || kind == TK_DST2_INV, quarter = kind == TK_DCT4 || kind == TK_DST4;
      const int rkind = tfwd ? (kind == TK_DCT2_FWD ? TK_REAL_DCT2_FWD : TK_REAL_DST2_FWD) : tinv ? (kind == TK_DCT2_INV ? TK_REAL_DCT2_INV : TK_REAL_DST2_INV)
                      : quarter ? (kind == TK_DCT4 ? TK_REAL_DCT4 : TK_REAL_DST4) : (kind == TK_DCT1 ? TK_REAL_DCT1 : TK_REAL_DST1);
      // DCT-II / DST-II of dense lines whose half length is a line-kernel size: permutation, real FFT and phase in ONE launch
      if (tfwd && S == 1 && b.opt.trig_fused && b.emit_lines_r2c(cur, dst, N, lines, a == rank - 1 ? scale : 1.0f, false, kind == TK_DCT2_FWD ? LM_DCT2 : LM_DST2)) {
        cur = dst;
        S *= N;
        continue;
      }
      // DCT-III / DST-III the same way on the c2r line kernel (bins formed from the real line in the pre-split, un-permutation
      // in the store); needs the LDS line buffer: half lengths of 64 and more
      if (tinv && S == 1 && N >= 128 && b.opt.trig_fused && b.emit_lines_r2c(cur, dst, N, lines, a == rank - 1 ? scale : 1.0f, true, kind == TK_DCT2_INV ? LM_DCT3 : LM_DST3)) {
        cur = dst;
        S *= N;
        continue;
      }
      const int64_t M = quarter ? N / 2 : (kind == TK_DCT1 || kind == TK_DST1 ? L : N);     // length of the FFT in the middle
      const int64_t P = quarter ? M : M / 2 + 1;                                  // complex elements per line
      const PtrRef v = quarter ? PtrRef() : b.alloc_work((uint64_t)lines * M * 4), V = b.alloc_work((uint64_t)lines * P * 8);
      const float last = a == rank - 1 ? scale : 1.0f;
      Step& pre = b.push(ST_TRIG_PRE);
      pre.p[TGP_X] = cur; pre.p[TGP_Z] = V; pre.p[TGP_Y] = quarter ? dst : v;
      pre.i[TG_LINES] = lines; pre.i[TG_N] = N; pre.i[TG_REAL_P] = P; pre.i[TG_REAL_M] = M; pre.i[TG_KIND] = rkind; pre.i[TG_STRIDE] = S;
      // S > 1 (axes >= 1): 32 x 32 tiles through LDS, one workgroup per tile
      const auto tiled_grid = [&](int64_t per) { return b.oneshot_grid((lines / S) * ((S + 31) / 32) * ((per + 31) / 32)); };   // one workgroup per tile
      pre.grid = S > 1 ? tiled_grid(tinv || quarter ? P : M) : b.oneshot_grid((lines * (tinv || quarter ? P : M) + 255) / 256);   // streaming pass: one-shot grid (r02)
      b.ir.route += "trig-real[kind=" + std::to_string(kind) + "] ";
      const int rc = quarter ? b.emit_axis(V, V, M, 1, lines, false, 1.0f, err)
                   : tinv ? b.emit_c2r_even(V, v, M, lines, 1.0f, err) : b.emit_r2c_even(v, V, M, lines, 1.0f, err);
      if (rc) return rc;
      Step& post = b.push(ST_TRIG_POST);
      post.p[TGP_X] = quarter ? cur : v; post.p[TGP_Z] = V; post.p[TGP_Y] = dst;
      post.i[TG_LINES] = lines; post.i[TG_N] = N; post.i[TG_REAL_P] = P; post.i[TG_REAL_M] = M; post.i[TG_KIND] = rkind; post.i[TG_STRIDE] = S;
      post.f[F_SCALE] = last;
      post.grid = S > 1 ? tiled_grid(tfwd || quarter ? P : N) : b.oneshot_grid((lines * (tfwd || quarter ? P : N) + 255) / 256);
      b.work_top = mark;
      cur = dst;
      S *= N;
      continue;
    }
    const PtrRef z = b.alloc_work((uint64_t)lines * L * 8);
    ++general_axes;
    Step& pre = b.push(ST_TRIG_PRE);
    pre.p[TGP_X] = cur; pre.p[TGP_Z] = z; pre.p[TGP_Y] = dst;
    pre.i[TG_LINES] = lines; pre.i[TG_N] = N; pre.i[TG_L] = L; pre.i[TG_S] = S; pre.i[TG_KIND] = kind;
    pre.grid = b.generic_grid(lines * L);
    const int rc = b.emit_axis(z, z, L, 1, lines, kind == TK_DCT2_INV || kind == TK_DST2_INV, 1.0f, err);
    if (rc) return rc;
    Step& post = b.push(ST_TRIG_POST);
    post.p[TGP_X] = cur; post.p[TGP_Z] = z; post.p[TGP_Y] = dst;
    post.i[TG_LINES] = lines; post.i[TG_N] = N; post.i[TG_L] = L; post.i[TG_S] = S; post.i[TG_KIND] = kind;
    post.f[F_SCALE] = a == rank - 1 ? scale : 1.0f;
    post.grid = b.generic_grid(lines * N);
    b.work_top = mark;         // the complex lines are a per-axis temporary
    cur = dst;
    S *= N;
  }
  if (general_axes) b.ir.route += "trig[kind=" + std::to_string(kind) + "] ";
  return finish_side_output(d, b, user_out, dst, d.shape, true, err);
}

// ---- fftconv: what both builders share ------------------------------------------------------------------------------------------
// The shapes of an fftconv plan, its output lanes and the index map of a padded axis 0.  A linear result is cropped out of the FFT
// domain, so any domain of at least shape + kernelShape - 1 points gives the same values: a builder may transform axis 0 on a longer
// one (pad_axis0).  Everything the caller states (zeroPad ranges, output shape and offset) stays on the logical domain [0, lfN).
// Padded index k is logical index k below `split` and k - padD from split + padD on; the padD indices in between belong to no logical
// index.  Convolution: split = lfN (the padding is the tail).  Correlation conjugates the kernel spectra, so its kernelShape - 1
// negative lags wrap to the TOP of the domain: split = shape.  pad_lo / pad_hi carry the start / the end of a logical range onto
// the padded domain.
struct ConvGeom {
  int rank;
  int64_t K, B;
  int64_t C = 1;                          // fftConv.inputChannels: B * C data lines and K * C kernels, result (k, b) summed over c
  int64_t G = 1, Cg = 1, Kg = 1;          // fftConv.groups: Cg = C / G channels and Kg = K / G kernels a group; K * Cg kernels, result (k, b) summed over the Cg channels
                                          // of group k / Kg, which start at input line b C + (k / Kg) Cg
  bool linear, corr;
  int64_t ks[8], fs[8], os[8], ooff[8];   // kernel shape, FFT domain (axis 0 as padded), output shape, crop offset on the logical domain
  int64_t inN, kN, oN, lfN;               // elements of a data item, a kernel and an output item; logical axis-0 length of the FFT domain
  int64_t padD = 0, split;
  // output lanes in elements (fftconv.js:868-871): result (k, b) starts at lane0 + k * lane_k + b * lane_b — the caller's strided
  // lanes, kernel-major [K][B][oN] or batch-major [B][K][oN]
  int64_t lane0, lane_k, lane_b;

  void pad_axis0(int64_t F0) { padD = F0 - lfN; fs[0] = F0; }
  int64_t pad_lo(int64_t m) const { return m < split ? m : m + padD; }
  int64_t pad_hi(int64_t e) const { return e <= split ? e : e + padD; }
  // a zeroPad range as ONE padded range (what lies between its two images is never read or extracted)
  mi355fft_zero_range padded(mi355fft_zero_range z) const { z.start[0] = pad_lo(z.start[0]); z.end[0] = pad_hi(z.end[0]); return z; }
  // the crop holds both positive and negative lags of a correlation: two pieces of the padded domain
  bool straddle() const { return padD > 0 && ooff[0] < split && ooff[0] + os[0] > split; }
  int64_t lane_offset(int64_t k) const { return lane0 + k * lane_k; }
  bool depthwise() const { return G > 1 && Cg == 1; }      // every output kernel reads ONE input channel (Kg > 1: a channel multiplier)
  bool one_channel() const { return C == 1 || depthwise(); }   // the single-channel routes apply (depthwise: the overlap-save ones, through push_per_kernel's load map)
};

// Validates the fftconv options and fills the geometry and the plan's extents for elements of `elem` bytes (8: complex, 4: real)
int conv_geometry(const mi355fft_plan_desc& d, int64_t elem, ConvGeom& g, PlanIR& ir, std::string& err) {
  if (d.io_input.enabled || d.io_output.enabled) { err = "ioView is not an fftconv option"; return MI355FFT_ERR_INVALID; }
  if (d.in_place) { err = "fftconv inPlace=true is not supported in current implementation"; return MI355FFT_ERR_INVALID; }
  if (d.conv_mode != MI355FFT_CONVOLUTION && d.conv_mode != MI355FFT_CORRELATION) { err = "fftConv.mode must be one of \"convolution\", \"correlation\""; return MI355FFT_ERR_INVALID; }
  if (d.conv_boundary < 0 || d.conv_boundary > 3) { err = "fftConv.boundary must be one of \"circular\", \"linear-full\", \"linear-same\", \"linear-valid\""; return MI355FFT_ERR_INVALID; }
  if (d.conv_kernel_count <= 0) { err = "fftConv.kernelCount must be a positive integer; got " + std::to_string(d.conv_kernel_count); return MI355FFT_ERR_INVALID; }
  const int rank = g.rank = d.rank;
  const int64_t K = g.K = d.conv_kernel_count, B = g.B = d.batch, C = g.C = std::max<int64_t>(1, d.input.reserved);
  if (C > 1 && prodv(d.shape, rank) * B * C > ((int64_t)1 << 40)) { err = "Unsupported: more than 2^40 points in one plan"; return MI355FFT_ERR_UNSUPPORTED; }
  const int64_t G = g.G = std::max<int64_t>(1, d.zero_read.reserved);
  if (C % G) { err = "fftConv.groups=" + std::to_string(G) + " must divide fftConv.inputChannels=" + std::to_string(C); return MI355FFT_ERR_INVALID; }
  if (K % G) { err = "fftConv.groups=" + std::to_string(G) + " must divide fftConv.kernelCount=" + std::to_string(K); return MI355FFT_ERR_INVALID; }
  const int64_t Cg = g.Cg = C / G;
  g.Kg = K / G;
  g.linear = d.conv_boundary != MI355FFT_CIRCULAR;
  g.corr = d.conv_mode == MI355FFT_CORRELATION;
  bool ks_given = false;
  for (int i = 0; i < rank; ++i) if (d.conv_kernel_shape[i] != 0) ks_given = true;
  for (int i = 0; i < rank; ++i) {
    int64_t &ks = g.ks[i], &fs = g.fs[i], &os = g.os[i], &ooff = g.ooff[i];
    ks = ks_given ? d.conv_kernel_shape[i] : d.shape[i];
    if (ks <= 0) { err = "fftConv.kernelShape must be an array of " + std::to_string(rank) + " positive ints"; return MI355FFT_ERR_INVALID; }
    if (!g.linear) {
      if (ks > d.shape[i]) { err = "fftConv.kernelShape[" + std::to_string(i) + "] must be <= shape[" + std::to_string(i) + "] when fftConv.boundary=\"circular\""; return MI355FFT_ERR_INVALID; }
      fs = d.shape[i]; os = d.shape[i]; ooff = 0;
    } else {
      fs = d.shape[i] + ks - 1;
      if (d.conv_boundary == MI355FFT_LINEAR_FULL) { os = fs; ooff = 0; }
      else if (d.conv_boundary == MI355FFT_LINEAR_SAME) { os = d.shape[i]; ooff = (ks - 1) / 2; }
      else {
        os = d.shape[i] - ks + 1; ooff = ks - 1;
        if (os <= 0) { err = "fftConv.boundary=\"linear-valid\" requires kernelShape[" + std::to_string(i) + "] <= shape[" + std::to_string(i) + "]"; return MI355FFT_ERR_INVALID; }
      }
    }
  }
  // zeroPad ranges live on the FFT domain: read = the embedded data before the forward transform, write = the inverse
  // transform before the crop (fftconv.js:386,542,565)
  if (int rv = validate_views(d, err, g.fs, g.fs)) return rv;
  g.lfN = g.fs[0];
  g.split = g.corr ? d.shape[0] : g.lfN;
  const int64_t inN = g.inN = prodv(d.shape, rank), kN = g.kN = prodv(g.ks, rank), oN = g.oN = prodv(g.os, rank);
  const int64_t kstride = d.conv_output_kernel_stride_elements;
  if (d.output.strided && K > 1 && kstride <= 0) { err = "multi-kernel strided output requires fftConv.channelPolicy.output or fftConv.outputKernelStrideElements"; return MI355FFT_ERR_INVALID; }
  ir.kernel_bytes = (uint64_t)K * Cg * kN * elem;
  ir.in_bytes = d.input.strided ? strided_extent_elems(d.input, d.shape, rank, B * C, 0) * elem : (uint64_t)inN * B * C * elem;
  ir.out_bytes = d.output.strided ? strided_extent_elems(d.output, g.os, rank, B, (K - 1) * kstride) * elem : (uint64_t)K * B * oN * elem;
  const bool kmajor = d.conv_output_layout == MI355FFT_KERNEL_MAJOR;
  g.lane0 = d.output.strided ? d.output.offset_elements : 0;
  g.lane_k = d.output.strided ? kstride : kmajor ? B * oN : oN;
  g.lane_b = d.output.strided ? (d.output.batch_stride_elements > 0 ? d.output.batch_stride_elements : oN) : kmajor ? oN : K * oN;
  return MI355FFT_OK;
}

// ---- the sides of an fftconv launch as address maps over the domain `dom` (the FFT domain, or the axis-0 line a route is dense over) ----
// Data: element i is read at offset + sum i_d * stride_d where zeroPad.read meets [0, shape), and is zero elsewhere (the embed)
SideMap conv_load_map(const mi355fft_plan_desc& d, const ConvGeom& g, const int64_t* dom, int rank) {
  SideMap m = Builder::dense_map(dom, rank);
  int64_t st = 1;
  for (int i = 0; i < rank; ++i) {
    m.stride[i] = d.input.strided ? d.input.strides[i] : st;
    st *= d.shape[i];
    int64_t lo = 0, hi = d.shape[i];
    if (d.zero_read.enabled) { lo = std::max(lo, d.zero_read.start[i]); hi = std::min(hi, d.zero_read.end[i]); }
    if (hi < lo) hi = lo;
    m.lo[i] = (int)lo; m.hi[i] = (int)hi;
  }
  m.offset = d.input.strided ? d.input.offset_elements : 0;
  m.batch_stride = d.input.strided && d.input.batch_stride_elements > 0 ? d.input.batch_stride_elements : g.inN;
  return m;
}
// Kernels: kernelShape zero-padded into the domain
SideMap conv_kernel_map(const ConvGeom& g, const int64_t* dom, int rank) {
  SideMap m = Builder::dense_map(dom, rank);
  int64_t st = 1;
  for (int i = 0; i < rank; ++i) { m.stride[i] = st; st *= g.ks[i]; m.hi[i] = (int)g.ks[i]; }
  m.batch_stride = g.kN;
  return m;
}
// Result of kernel k: element i - ooff of its lane is stored for i inside the crop [ooff, ooff + os), as zero outside the
// zeroPad.write range; both ranges are logical (the VIEW and rconv kernels carry them onto a padded axis themselves)
SideMap conv_store_map(const mi355fft_plan_desc& d, const ConvGeom& g, const int64_t* dom, int rank, int64_t k) {
  SideMap m = Builder::dense_map(dom, rank);
  m.offset = g.lane_offset(k);
  m.batch_stride = g.lane_b;
  int64_t st = 1;
  for (int i = 0; i < rank; ++i) {
    m.stride[i] = d.output.strided ? d.output.strides[i] : st;
    st *= g.os[i];
    m.lo[i] = (int)g.ooff[i]; m.hi[i] = (int)(g.ooff[i] + g.os[i]);
    m.zlo[i] = d.zero_write.enabled ? (int)d.zero_write.start[i] : 0;
    m.zhi[i] = d.zero_write.enabled ? (int)d.zero_write.end[i] : (int)(i == 0 ? g.lfN : g.fs[i]);
    m.offset -= g.ooff[i] * m.stride[i];
  }
  return m;
}
// The crop as a pass of its own: kernel k's inverse transform `y`, dense over the FFT domain, into its lane of the output
void conv_staged_crop(Builder& b, const mi355fft_plan_desc& d, const ConvGeom& g, PtrRef out, PtrRef y, int64_t k, bool real_elements) {
  const int rank = g.rank;
  const int64_t fN = prodv(g.fs, rank);
  mi355fft_side_layout lay = d.output;
  if (!lay.strided) { lay.strided = 1; int64_t st = 1; for (int i = 0; i < rank; ++i) { lay.strides[i] = st; st *= g.os[i]; } }
  lay.offset_elements = g.lane_offset(k);
  lay.batch_stride_elements = g.lane_b;
  int64_t poff[8], s1[8], s2[8], o2[8];
  for (int i = 0; i < rank; ++i) { poff[i] = o2[i] = g.ooff[i]; s1[i] = s2[i] = g.os[i]; }
  poff[0] = g.pad_lo(g.ooff[0]);
  if (!g.straddle()) { b.emit_strided(false, out, y, lay, g.os, rank, g.B, g.fs, poff, fN, 0, real_elements); return; }
  s1[0] = g.split - g.ooff[0]; s2[0] = g.os[0] - s1[0]; o2[0] = g.split + g.padD;
  b.emit_strided(false, out, y, lay, s1, rank, g.B, g.fs, poff, fN, 0, real_elements);
  b.emit_strided(false, out, y, lay, s2, rank, g.B, g.fs, o2, fN, s1[0] * lay.strides[0], real_elements);
}

// ---- re-basing a finished plan onto workspace staging (f16-storage, rconv-widened) ----
Step convert_step(StepKind kind, PtrRef src, PtrRef dst, int64_t count, unsigned grid) {
  Step c;
  c.kind = kind; c.p[P_SRC] = src; c.p[P_DST] = dst; c.i[S_COUNT] = count; c.grid = grid;
  return c;
}
// Every reference to the caller's input / output / kernel buffer moves to the workspace offset given for it; the converter steps
// `front` go in front of the plan's steps and `back` behind
void restage(PlanIR& ir, uint64_t in_stage, uint64_t out_stage, uint64_t kernel_stage, std::vector<Step> front, const std::vector<Step>& back) {
  for (Step& s : ir.steps)
    for (PtrRef& p : s.p) {
      if (p.buf == BUF_INPUT) p = PtrRef(BUF_WORK, (int64_t)in_stage + p.off);
      else if (p.buf == BUF_OUTPUT) p = PtrRef(BUF_WORK, (int64_t)out_stage + p.off);
      else if (p.buf == BUF_KERNEL) p = PtrRef(BUF_WORK, (int64_t)kernel_stage + p.off);
    }
  front.insert(front.end(), ir.steps.begin(), ir.steps.end());
  front.insert(front.end(), back.begin(), back.end());
  ir.steps.swap(front);
}

// The block length the default rule (PlannerOptions::conv_ols == 1) gives to overlap-save on a complex line of lfN = shape + M - 1 logical points
// and a kernel of M points; 0: the request keeps its earlier route.  Left alone: requests of at most 16384 points and kernels beyond 513 points (where a
// 4096-point block returns less than 7/8 of its positions; not measured).  Measured (profiles/fftconv_cols_ab.log: 128 x 2^20 (*) {31, 255, 513}, K = 1 and 4,
// 1024 x 100000 (*) 129, 128 x 700000 (*) 255 and two lines above 2^22, P = 512 .. 4096): every block length is 4.1-9.9x ahead of pad[..] fftconv[K] and
// 2.4-3.2x ahead of fftconv-pipeline-view; the fastest P is the smallest power of two >= 8 (M - 1) from 2048 on (M = 31: 512, 1024 and 2048 within the
// 3 % spread; M = 129: 2048 is 5 % ahead of 1024; M = 255: 2048; M = 513: 2048 and 4096 within 2 %)
constexpr int64_t CONV_OLS_MIN_FN = 16384, CONV_OLS_MAX_KERNEL = 513;
int64_t conv_ols_block(int64_t lfN, int64_t M) {
  if (lfN <= CONV_OLS_MIN_FN || M > CONV_OLS_MAX_KERNEL) return 0;
  return 8 * (M - 1) <= 2048 ? 2048 : 4096;
}

// The tile edge the default rule (PlannerOptions::conv_ols2d == 1) gives to overlap-save on a rank-2 image of fN0 x fN1 = shape + M - 1 logical points and a
// kernel of M0 x M1 points; 0: the request keeps its earlier route.  Left alone: domains of at most 16384 points and axes below 64 points (the small requests
// whose routes the tests pin; a tile would be mostly padding) and kernels beyond 33 points on an axis (a 128-point tile returns less than 3/4 of its
// positions per axis; not measured).
// Measured (profiles/fftconv_tiles_ab.log: 8 x 1024^2 (*) 9x9, 4 x 512^2 (*) 5x5, 3 x 1920x1080 (*) 17x17, 4096^2 (*) 33x33 valid, 16 x 256^2 (*) 3x3 and
// 8 x 1016^2 (*) 9x9 full, K = 1 and 4, both tiles; spread between repeated samples <= 3.2 %): both tiles are 9-44x ahead of the Bluestein / mixed-radix
// plans and 2.0-3.4x ahead of the power-of-two domain 1024^2 of the linear-full request (lines-mapped + columns: 0.206 ms against 0.061), so no class is
// excluded.  P = 64 is 29-68 % ahead of P = 128 up to 17 points (9x9: 138 against 107 G points/s; 17x17: 109 against 81; 3x3 and 5x5: 52 against 31);
// at 33 points P = 128 is 47-51 % ahead (95-102 against 65-68).  Kernels of 18 .. 32 points were not measured: they take the larger tile
constexpr int64_t CONV_TILES_MIN_POINTS = 16384, CONV_TILES_MIN_AXIS = 64, CONV_TILES_MAX_KERNEL = 33, CONV_TILES_P64_MAX_KERNEL = 17;
int64_t conv_tiles_block(int64_t fN0, int64_t fN1, int64_t M0, int64_t M1) {
  const int64_t M = std::max(M0, M1);
  if (fN0 * fN1 <= CONV_TILES_MIN_POINTS || fN0 < CONV_TILES_MIN_AXIS || fN1 < CONV_TILES_MIN_AXIS || M > CONV_TILES_MAX_KERNEL) return 0;
  return M <= CONV_TILES_P64_MAX_KERNEL ? 64 : 128;
}

// The tile edge the default rule (PlannerOptions::rconv_ols2d == 1) gives to overlap-save on a real rank-2 image: conv_tiles_block's bounds (they also keep the
// small real rank-2 requests on rconv[K], whose routes the tests pin) and, as measured, its tile edges.
// Measured (profiles/fftconv_rtiles_ab.log: conv_tiles_block's six requests as real data, K = 1 and 4, both tiles; spread between repeated samples <= 3.9 %):
// both tiles are 2.5-38x ahead of rconv[K] on the exact-length domain on every request (the nearest: 3.8-5.3x at P = 64 on 8 x 1016^2 (*) 9x9 linear-full,
// whose domain 1024^2 keeps rconv[K] off the Bluestein lines), so no class is excluded.  P = 64 is 48-86 % ahead of P = 128 up to 17 points (9x9: 210-246
// against 137-165 G real points/s; 17x17: 163-191 against 104-123; 3x3 and 5x5: 52-72 against 28-38); at 33 points P = 128 is 41-48 % ahead (160-175 against
// 113-118): the complex route's boundary.  Kernels of 18 .. 32 points were not measured: they take the larger tile, as there
int64_t rconv_tiles_block(int64_t fN0, int64_t fN1, int64_t M0, int64_t M1) { return conv_tiles_block(fN0, fN1, M0, M1); }

// The tile edge the default rule (PlannerOptions::sum_ols2d == 1) gives to the sum form of the tile routes (fftConv.inputChannels > 1, complex and real): conv_tiles_block's
// bounds on the domain, and the one sum instance there is, P = 64, for the kernels conv_tiles_block gives that tile (up to 17 points an axis).  Kernels of 18 .. 33
// points take the composed routes fftconv-sum / rconv-sum: a P = 128 sum instance does not exist (MI355_TILE_SUM_KERNEL_LIST)
// Measured (profiles/fftconv_sum_ab.log: 8 x 1024^2 (*) 9x9, 4 x 512^2 (*) 5x5 and 3 x 1920x1080 (*) 17x17 linear-same, complex and real, C = 3 / 16 / 64, K = 1 / 4, the three
// forms timed alternately in one process; spread between a form's two medians <= 1.4 %): the tile-sum route is 10.0-38.7x (complex) and 5.9-36.0x (real) ahead of the composed
// sum route (MI355FFT_SUM_OLS2D=0: Bluestein / mixed-radix transforms of batch * C whole images) on every request, so no class inside the instance's bounds is
// excluded; against C single-channel tile plans run back to back WITHOUT their sum it is 1.50-1.85x at C = 3, 1.85-3.18x at C = 16 and 1.90-3.37x at C = 64 ahead
// (98-297 / 100-534 G complex / real input points/s)
int64_t sum_tiles_block(int64_t fN0, int64_t fN1, int64_t M0, int64_t M1) { return conv_tiles_block(fN0, fN1, M0, M1) == 64 ? 64 : 0; }

// The tile edge the default rule (PlannerOptions::group_ols2d == 1) gives to the grouped tile kernel (fftConv.groups > 1, every output kernel in one launch): sum_tiles_block's
// bounds (conv_tiles_block's on the domain, kernels up to 17 points an axis: the one grouped tile there is, P = 64), for all four classes of request (depthwise, Cg = 1 /
// grouped sums, Cg > 1; complex / real).  A class is in the rule only where the kernel was ahead of BOTH alternatives on every measured request of the class by more than
// the spread between a form's two medians; all four were.  Measured (profiles/fftconv_group_ab.log, tools/fftconv_group_ab.py: linear-same, 8 x 256^2 (*) 3x3 and 5x5 with
// C = K = G = 64, 4 x 512^2 (*) 9x9 with C = K = G = 32, 8 x 256^2 (*) 3x3 with C = K = 64, G = 4 and with C = 16, K = 32, G = 16, 3 x 1920x1080 (*) 17x17 with
// C = K = G = 3; the three forms timed alternately in one process, spread <= 1.5 %): against MI355FFT_GROUP_OLS2D=0 (depthwise: the single-channel tile route through the
// per-kernel load map, 1 + K launches; Cg > 1: the composed route) the one launch is 2.4-3.6x (complex) and 3.3-5.5x (real) ahead on the depthwise requests of 32 and 64
// channels, 1.12x / 1.10x at C = 3 on 1920x1080 (3 launches saved, every launch already full) and 10.4x / 10.1x on G = 4; against G plans with inputChannels = Cg and
// kernelCount = Kg on data already sliced per group, the slicing not counted, 3.3-5.2x / 4.8-8.2x, 1.22x / 1.26x and 2.6x / 4.5x
int64_t group_tiles_block(int64_t fN0, int64_t fN1, int64_t M0, int64_t M1) { return sum_tiles_block(fN0, fN1, M0, M1); }

// The brick edge the default rule (PlannerOptions::conv_ols3d == 1) gives to overlap-save on a rank-3 volume of fN0 x fN1 x fN2 = shape + M - 1 logical points
// and a kernel of M0 x M1 x M2 points; 0: the request keeps its earlier route.  Left alone: domains of at most 32768 points and axes below 32 points (the
// small requests whose routes the tests pin; a brick would be mostly padding) and kernels beyond 9 points on an axis (a brick returns less than 1/8 of its
// points; not measured: 10 .. 15 points stay on the switch alone).
// Measured (profiles/fftconv_bricks_ab.log: 256^3 (*) {3^3, 5^3, 7^3, 9^3}, 8 x 128^3 (*) 5^3, 64 x 64^3 (*) 3^3, 500x300x200 (*) 5x5x3 and, for the domain 256^3
// of the power-of-two lines and columns, {252^3 (*) 5^3, 250^3 (*) 7^3, 248^3 (*) 9^3} linear-full, K = 1 and 4; spread between repeated samples <= 1.4 % for
// the brick and <= 0.4 % for the old plans): the brick is ahead on every request in every class: 3^3 66-85x and 7^3 31-41x the Bluestein plans of 256^3
// (133-140 and 63 G points/s per kernel), 3^3 7.0-11.3x, 5^3 6.1-12.9x and 9^3 3.9-5.2x the mixed-radix plans (132-134, 101-107 and 39-40), 500x300x200
// 37-49x, and against the power-of-two domain 256^3 2.95-3.37x at 5^3, 1.93-2.22x at 7^3 and 1.19-1.39x at 9^3 (the nearest).  So kernel edges up to 9 enter
// the rule; the even edges between the measured odd ones take their neighbours' verdict
constexpr int64_t CONV_BRICKS_MIN_POINTS = 32768, CONV_BRICKS_MIN_AXIS = 32, CONV_BRICKS_MAX_KERNEL = 9, RCONV_BRICKS_MAX_KERNEL = 9;
int64_t bricks_block(const int64_t* fs, const int64_t* ks, int64_t max_kernel) {
  const int64_t M = std::max(ks[0], std::max(ks[1], ks[2]));
  if (std::min(fs[0], std::min(fs[1], fs[2])) < CONV_BRICKS_MIN_AXIS || M > max_kernel) return 0;
  // fN0 fN1 fN2 <= MIN_POINTS, without forming a product that could leave 64 bits (an axis may hold 2^31 points): every axis is >= 32 here, so the domain
  // is small only if each axis is at most MIN_POINTS / 32^2, and then the product fits
  const int64_t cap = CONV_BRICKS_MIN_POINTS / (CONV_BRICKS_MIN_AXIS * CONV_BRICKS_MIN_AXIS);
  if (fs[0] <= cap && fs[1] <= cap && fs[2] <= cap && fs[0] * fs[1] * fs[2] <= CONV_BRICKS_MIN_POINTS) return 0;
  return 16;
}
int64_t conv_bricks_block(const int64_t* fs, const int64_t* ks) { return bricks_block(fs, ks, CONV_BRICKS_MAX_KERNEL); }
// The same for real volumes (PlannerOptions::rconv_ols3d == 1): conv_bricks_block's bounds (they also keep the small real rank-3 requests on rconv[K], whose
// routes the tests pin) and, as measured, its largest kernel edge.
// Measured (profiles/fftconv_rbricks_ab.log: conv_bricks_block's requests as real data; spread <= 2.8 % for the brick, <= 0.2 % for the old plans): ahead of
// rconv[K] on every request in every class: 3^3 48-59x (64 x 64^3: 6.7-10.6x), 7^3 25-33x, 5^3 5.8-12.1x, 9^3 3.9-5.2x, 500x300x200 29-38x, and against
// the domain 256^3 3.5-4.7x at 5^3, 2.5-3.4x at 7^3 and 1.65-2.26x at 9^3: the complex route's boundary.  66-205 G real points/s per kernel
int64_t rconv_bricks_block(const int64_t* fs, const int64_t* ks) { return bricks_block(fs, ks, RCONV_BRICKS_MAX_KERNEL); }

// ---- overlap-save: what its six routes share --------------------------------------------------------------------------------------------
// Linear modes, and circular boundaries in the WRAP form described above ols_circular_take.  A line (rank 1), an image (rank 2) or a volume (rank 3) is cut into blocks of P points per axis, and each block runs forward transform, product with a kernel
// spectrum on P points and inverse transform inside one workgroup: no padded or exact-length domain, no transform of a whole line, no Bluestein or column
// launch.  One launch writes the K kernel spectra into the workspace, then one launch per kernel follows: 1 + K launches for any length.  Strided lanes,
// channel-policy lanes, zeroPad and the crop ride the two address maps (the real routes stand in front of build_fftconv_real's rejection of strided sides
// for that reason).  The kernels' indices are 32-bit: every route bounds its axes and its block count by 2^31 less a margin.
//
// A route's switch (PlannerOptions::conv_ols, rconv_ols, conv_ols2d, rconv_ols2d, conv_ols3d, rconv_ols3d; `sw` nonzero here): 0 keeps the earlier routes for every request (the
// caller's gate); 1 is the route's measured rule, `rule`; any other value forces that block on every request it fits (L >= 2 per axis) where it is a legal
// block of the route (`legal`: complex lines a power of two 128 .. 4096, real lines 128 .. 8192, tiles 64 or 128, bricks 16), and gives none where it is not
int64_t ols_switch(int64_t sw, bool legal, int64_t rule) { return sw > 1 ? (legal ? sw : 0) : rule; }

// The geometry of one axis of fN = shape + M - 1 logical points under a kernel of M points and blocks of P.  Block j holds signal indices [s0, s0 + P),
// s0 = j L - pre, pre = M - 1, and gives L = P - pre results.  A real line is transformed as P / 2 complex points, so pre and L stay even there:
// pre = M - 1 + e, e = (M - 1) & 1, L = (P - pre) & ~1.  The result window of a block starts at w0 = pre convolving and at e correlating (the conjugated
// spectrum puts the wrap-around at the top of the block); signal indices stay below plim.  nb = 0: the block does not fit (P = 0 included)
//
// `wrap` (circular boundary: fN = shape = N, the output has N points and no crop offset): L is the linear form's, nb = ceil(N / L), fN = plim = N, and
// block j holds signal indices j L - pre .. j L - pre + P - 1 TAKEN MODULO N.  Convolving, pre = w0 = M - 1 (+ e): block j stores the results of signal
// positions [j L, j L + L) below N.  Correlating, y[m] = sum_t conj(h[t]) x[(m + t) mod N] looks forward only, so the blocks need no head: pre = w0 = 0
// (no head of M - 1 points with a wrapping store), block j starts at j L, only its tail wraps, and its wrap-free window is again [j L, j L + L) below N.  In both
// modes the windows of the nb blocks partition [0, N): every output element is stored by exactly one block, and the store rule is the linear one
// (q = s0 + i is never negative inside a window, so m = q)
OlsAxis ols_axis(int64_t fN, int64_t shape, int64_t M, int64_t P, bool corr, bool real_line, bool wrap = false) {
  OlsAxis a;
  a.pre = real_line ? M - 1 + ((M - 1) & 1) : M - 1;
  a.L = real_line ? (P - a.pre) & ~(int64_t)1 : P - a.pre;
  a.nb = a.L >= 2 ? (fN + a.L - 1) / a.L : 0;
  a.fN = fN; a.plim = corr ? shape : fN; a.w0 = corr ? a.pre - (M - 1) : a.pre;
  if (wrap) { a.plim = fN; if (corr) a.pre = 0; a.w0 = a.pre; }
  return a;
}

// Circular boundaries on the six routes (PlannerOptions::ols_circular; `P` is the block the route's own rule names for the domain `shape`, 0: none).  The
// route is taken only where shape[a] >= 2 P on every axis: any index a block (or the absent partner of a real pair) forms then wraps at most once.  2: every
// such request; 1: those with an axis that is no power of two (their earlier plans hold Bluestein, mixed-radix or per-radix stage launches) and lines above
// 2^22 points; power-of-two domains keep the routes the tests pin them to
bool ols_circular_take(const PlannerOptions& opt, const int64_t* shape, int rank, int64_t P) {
  if (!opt.ols_circular || P <= 0) return false;
  bool pow2 = true;
  for (int a = 0; a < rank; ++a) { if (shape[a] < 2 * P) return false; pow2 = pow2 && is_pow2(shape[a]); }
  return opt.ols_circular >= 2 || !pow2 || (rank == 1 && shape[0] > ((int64_t)1 << 22));
}

// One launch per kernel: K copies of the prepared step `proto`, launch k with kernel k's spectrum (`spectra` + k * `bytes`) in p[slot] and kernel k's
// lane of the output behind its store map.  (The overlap-save routes and lines-rconv[N=P]; the caller has written the mode's own slots)
// Depthwise requests (fftConv.groups with Cg = 1, ConvGeom::depthwise) run the single-channel kernels through the load map alone: launch k reads one channel of
// every item, input line b C + k / Kg, so the map steps C lines from item to item and starts k / Kg lines in
void push_per_kernel(Builder& b, const mi355fft_plan_desc& d, const ConvGeom& g, const Step& proto, LinesPtr slot, PtrRef spectra, int64_t bytes) {
  for (int64_t k = 0; k < g.K; ++k) {
    Step& st = b.push(ST_LINES);
    st = proto;
    st.p[slot] = spectra.plus(k * bytes);
    st.omap = conv_store_map(d, g, g.fs, g.rank, k);
    if (g.depthwise()) {
      st.imap.offset += (k / g.Kg) * proto.imap.batch_stride;
      st.imap.batch_stride = proto.imap.batch_stride * g.C;
    }
  }
}
// the route tag's last field of such a request
std::string depthwise_field(const ConvGeom& g) { return g.depthwise() ? ",G=" + std::to_string(g.G) : std::string(); }

// That step for the line routes: `lines` lines (or blocks) of P points on the line kernel `m`, `outer` LDS elements a line, read through the data map.
// The real modes carry the split roots `proots` (LO and HI in one table) as well
Step conv_line_proto(const Builder& b, const mi355fft_plan_desc& d, const ConvGeom& g, const LineKernelMeta& m, LineMode mode, int64_t lines, int64_t outer, int64_t P,
                     PtrRef tables, PtrRef proots = PtrRef()) {
  Step st;
  st.kind = ST_LINES;
  st.variant = m.id;
  st.p[LP_IN] = PtrRef(BUF_INPUT, 0); st.p[LP_OUT] = PtrRef(BUF_OUTPUT, 0); st.p[LP_TW] = tables;
  const int64_t tiles = (lines + m.T - 1) / m.T;
  st.i[LS_TILES] = tiles; st.i[LS_LINES] = lines; st.i[LS_IN_S] = 1; st.i[LS_IN_OUTER] = outer; st.i[LS_OUT_S] = 1; st.i[LS_OUT_OUTER] = outer;
  if (mode != LM_CONV_OLS) { st.p[LP_TW_LO] = proots; st.i[LS_FS_SHIFT] = 10; st.i[LS_FS_LO_MASK] = 1023; }
  st.i[LS_MODE] = mode; st.i[LS_MAPPED] = 1; st.i[LS_CONJ] = g.corr ? 1 : 0;
  st.f[F_SCALE] = (float)(1.0 / (double)P);
  st.imap = conv_load_map(d, g, g.fs, 1);
  st.grid = b.lines_grid(m, tiles);
  return st;
}

// Overlap-save in two dimensions: images, small kernels, one launch per kernel on P x P tiles (kern_tiles.hpp has the index map).  Tile (j0, j1) holds signal
// indices [s0_a, s0_a + P) on axis a and gives L0 x L1 results (ols_axis per axis); K P^2 8 bytes of workspace for any image.  The first launch is the tile
// kernel's forward half on the kernels, zero-padded into a tile by conv_kernel_map: the K spectra in the order the product reads them, one tile a kernel, no
// overlap.  `real`: f32 data (the maps and the geometry count f32 elements); a work item is a PAIR of tiles that are neighbours on axis 1, one in the real and
// one in the imaginary parts of the complex tile: B nb_0 ceil(nb_1 / 2) work items a launch.  In the spectrum launch a work item is one real kernel (nb_1 = 1
// and L_1 = P put its partner beyond the kernel map: zero imaginary parts): K complex spectra on P x P points.  False: the request keeps its earlier route
bool emit_tiles_ols(Builder& b, const mi355fft_plan_desc& d, const ConvGeom& g, bool real) {
  const int64_t *ks = g.ks, *fs = g.fs, lim = ((int64_t)1 << 31) - 16384;   // (the kernel's indices are 32-bit)
  if (fs[0] >= lim || fs[1] >= lim) return false;
  const int64_t sw = real ? b.opt.rconv_ols2d : b.opt.conv_ols2d, rule = real ? rconv_tiles_block(fs[0], fs[1], ks[0], ks[1]) : conv_tiles_block(fs[0], fs[1], ks[0], ks[1]);
  const bool wrap = !g.linear;                                              // (circular: the rule's tile alone, a forced tile moves linear requests only)
  // fftConv.inputChannels C > 1: the kernel's sum form.  A work item loops over c: channel c's tile from input line sb C + c (the load map's batch stride is the
  // line stride), forward, accumulate times spectrum (k, c); one inverse and one store a tile.  K C spectra in the workspace, launch k reads those from k C on.
  // Linear boundaries only; its own switch (PlannerOptions::sum_ols2d, rule sum_tiles_block) behind the route's
  // fftConv.groups G > 1, three ways:
  //   the grouped kernel (PlannerOptions::group_ols2d, rule group_tiles_block; linear boundaries): ONE launch of B K per_image work items, item (sb, k, tile) summing the
  //     Cg channels of group k / Kg into kernel k's lane; K Cg spectra in the workspace
  //   depthwise (Cg = 1) without it: the single-channel instances under their own switch and rule, circular ones included, launch k reading channel k / Kg
  //     through its load map (push_per_kernel)
  //   Cg > 1 without it: not here (the composed routes)
  const int64_t C = g.C, Cg = g.Cg, ssw = b.opt.sum_ols2d, gsw = b.opt.group_ols2d;
  const int64_t PG = g.G > 1 && !wrap ? (gsw == 64 ? 64 : gsw == 1 ? group_tiles_block(fs[0], fs[1], ks[0], ks[1]) : 0) : 0;
  const OlsAxis gax[2] = {ols_axis(fs[0], d.shape[0], ks[0], PG, g.corr, false, false), ols_axis(fs[1], d.shape[1], ks[1], PG, g.corr, false, false)};
  const TileKernelMeta* gm = PG && gax[0].L >= 2 && gax[1].L >= 2 ? find_tile_kernel((int)PG, real, Cg > 1, Cg > 1 ? 1 : 2) : nullptr;
  const bool grouped = gm != nullptr;
  if (g.G > 1 && !grouped && Cg > 1) return false;
  const bool sum = !grouped && g.G == 1 && C > 1;
  if (sum && (wrap || ssw == 0)) return false;
  const int64_t P = grouped ? PG
                  : sum ? ols_switch(ssw, ssw == 64 || ssw == 128, sum_tiles_block(fs[0], fs[1], ks[0], ks[1]))
                        : wrap ? (ols_circular_take(b.opt, d.shape, 2, rule) ? rule : 0) : ols_switch(sw, sw == 64 || sw == 128, rule);
  const TileKernelMeta* tm = grouped ? gm : P ? find_tile_kernel((int)P, real, sum) : nullptr;
  const TileKernelMeta* sm = (sum || grouped) && tm ? find_tile_kernel((int)P, real) : tm;    // the spectrum launch stays on the single-channel instance
  const OlsAxis ax[2] = {ols_axis(fs[0], d.shape[0], ks[0], P, g.corr, false, wrap), ols_axis(fs[1], d.shape[1], ks[1], P, g.corr, false, wrap)};
  const int64_t per_image = ax[0].nb * (real ? (ax[1].nb + 1) / 2 : ax[1].nb);
  const int64_t items = g.B * (grouped ? g.K : 1) * per_image;
  if (!tm || !sm || ax[0].L < 2 || ax[1].L < 2 || ax[0].nb * ax[1].nb >= lim || g.B * per_image >= lim || items >= lim || g.B * C >= lim || g.K * Cg >= lim) return false;
  const int64_t pd[2] = {P, P};
  const PtrRef G = b.alloc_work((uint64_t)g.K * Cg * P * P * 8);
  std::vector<float2h> roots;
  for (int q = 1; q < tm->R1; ++q) for (int k = 0; k < tm->R0; ++k) roots.push_back(root_of_unity((int64_t)q * k, P));
  const PtrRef tables = b.add_table(roots);
  int64_t per_cu = std::min<int64_t>((160 * 1024) / tm->lds_bytes, 2048 / tm->threads);
  per_cu = std::max<int64_t>(per_cu, 1);
  const auto launch = [&](const TileKernelMeta* km, LineMode mode, PtrRef src, PtrRef dst, int64_t count) {
    Step st;
    st.kind = ST_LINES;
    st.variant = km->id;
    st.p[LP_IN] = src; st.p[LP_OUT] = dst; st.p[LP_TW] = tables;
    st.i[LS_TILES] = count; st.i[LS_LINES] = count; st.i[LS_IN_S] = 1; st.i[LS_IN_OUTER] = P; st.i[LS_OUT_S] = 1; st.i[LS_OUT_OUTER] = P;
    st.i[LS_MODE] = mode; st.i[LS_MAPPED] = 1;
    st.grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(count, per_cu * b.opt.compute_units));
    return st;
  };
  const std::string tile = "[N=" + std::to_string(P) + "x" + std::to_string(P);
  Step sp = launch(sm, real ? LM_TILES_RSPECTRUM : LM_TILES_SPECTRUM, PtrRef(BUF_KERNEL, 0), G, g.K * Cg);
  OlsAxis whole;
  whole.fN = whole.plim = whole.L = P; whole.nb = 1;
  ols_store(sp.i, whole, whole);
  sp.imap = conv_kernel_map(g, pd, 2); sp.omap = Builder::dense_map(pd, 2);
  b.ir.steps.push_back(sp);
  b.ir.route += (real ? "tiles-rspectrum" : "tiles-spectrum") + tile + "] ";
  Step proto = launch(tm, real ? LM_TILES_RCONV_OLS : LM_TILES_CONV_OLS, PtrRef(BUF_INPUT, 0), PtrRef(BUF_OUTPUT, 0), items);
  proto.i[LS_CONJ] = g.corr ? 1 : 0; proto.i[LS_OLS_WRAP] = wrap ? 1 : 0; proto.i[LS_TILES_CHANNELS] = sum ? C : 0;
  ols_store(proto.i, ax[0], ax[1]);
  proto.f[F_SCALE] = (float)(1.0 / (double)(P * P));
  proto.imap = conv_load_map(d, g, fs, 2);
  const std::string tiles = ",L=" + std::to_string(ax[0].L) + "x" + std::to_string(ax[1].L);
  if (grouped) {      // one launch: the kernel forms each item's lane from kernel 0's store map and ConvGeom::lane_k, uniform for every output layout, explicit kernel stride and channel policy
    const auto both = [](int64_t lo, int64_t hi) { return (int64_t)((uint64_t)lo | ((uint64_t)hi << 32)); };
    proto.i[LS_TILES_CHANNELS] = both(Cg, C); proto.i[LS_TILES_KERNELS] = both(g.K, g.Kg); proto.i[LS_TILES_LANE_K] = g.lane_k;
    proto.p[LP_MUL_SPECTRUM] = G;
    proto.omap = conv_store_map(d, g, g.fs, g.rank, 0);
    b.ir.steps.push_back(proto);
    b.ir.route += std::string(real ? "tiles-rconv-ols-group" : "tiles-conv-ols-group") + tile + tiles + ",C=" + std::to_string(C) + ",G=" + std::to_string(g.G) + ",K=" + std::to_string(g.K) + "] ";
    return true;
  }
  push_per_kernel(b, d, g, proto, LP_MUL_SPECTRUM, G, Cg * P * P * 8);
  b.ir.route += std::string(real ? "tiles-rconv-ols" : "tiles-conv-ols") + (sum ? "-sum" : "") + tile + tiles +
                (sum ? ",C=" + std::to_string(C) : std::string()) + depthwise_field(g) + (wrap ? ",wrap] " : "] ");
  return true;
}

// Overlap-save in three dimensions: volumes, small kernels, one launch per kernel on 16^3 bricks (kern_bricks.hpp has the index map): emit_tiles_ols with a
// third axis.  Brick (j0, j1, j2) holds signal indices [s0_a, s0_a + 16) on axis a and gives L0 x L1 x L2 results; K 16^3 8 bytes of workspace for any volume.
// The first launch is the brick kernel's forward half on the kernels, zero-padded into a brick by conv_kernel_map.  `real`: f32 data; a work item is a PAIR
// of bricks that are neighbours on axis 2: B nb_0 nb_1 ceil(nb_2 / 2) work items a launch, and in the spectrum launch one real kernel (nb_2 = 1 and L_2 = 16
// put its partner beyond the kernel map).  False: the request keeps its earlier route
bool emit_bricks_ols(Builder& b, const mi355fft_plan_desc& d, const ConvGeom& g, bool real) {
  const int64_t *ks = g.ks, *fs = g.fs, lim = ((int64_t)1 << 31) - 16384;   // (the kernel's indices are 32-bit)
  if (fs[0] >= lim || fs[1] >= lim || fs[2] >= lim) return false;
  const int64_t sw = real ? b.opt.rconv_ols3d : b.opt.conv_ols3d, rule = real ? rconv_bricks_block(fs, ks) : conv_bricks_block(fs, ks);
  const bool wrap = !g.linear;                                              // (circular: as in emit_tiles_ols)
  const int64_t P = wrap ? (ols_circular_take(b.opt, d.shape, 3, rule) ? rule : 0) : ols_switch(sw, sw == 16, rule);
  const BrickKernelMeta* bm = P ? find_brick_kernel((int)P, real) : nullptr;
  OlsAxis ax[3];
  for (int a = 0; a < 3; ++a) ax[a] = ols_axis(fs[a], d.shape[a], ks[a], P, g.corr, false, wrap);
  if (!bm || ax[0].L < 2 || ax[1].L < 2 || ax[2].L < 2) return false;
  const int64_t n01 = ax[0].nb * ax[1].nb;                                  // (each nb < 2^31: the products below stay inside 64 bits step by step)
  if (n01 >= lim || n01 * ax[2].nb >= lim) return false;
  const int64_t items = g.B * n01 * (real ? (ax[2].nb + 1) / 2 : ax[2].nb);
  if (g.B >= lim || items >= lim) return false;
  const int64_t pd[3] = {P, P, P}, V = P * P * P;
  const PtrRef G = b.alloc_work((uint64_t)g.K * V * 8);
  int64_t per_cu = std::min<int64_t>((160 * 1024) / bm->lds_bytes, 2048 / bm->threads);
  per_cu = std::max<int64_t>(per_cu, 1);
  const auto launch = [&](LineMode mode, PtrRef src, PtrRef dst, int64_t count) {
    Step st;
    st.kind = ST_LINES;
    st.variant = bm->id;
    st.p[LP_IN] = src; st.p[LP_OUT] = dst;
    st.i[LS_TILES] = count; st.i[LS_LINES] = count; st.i[LS_IN_S] = 1; st.i[LS_IN_OUTER] = P; st.i[LS_OUT_S] = 1; st.i[LS_OUT_OUTER] = P;
    st.i[LS_MODE] = mode; st.i[LS_MAPPED] = 1;
    st.grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(count, per_cu * b.opt.compute_units));
    return st;
  };
  const std::string brick = "[N=" + std::to_string(P) + "x" + std::to_string(P) + "x" + std::to_string(P);
  Step sp = launch(real ? LM_BRICKS_RSPECTRUM : LM_BRICKS_SPECTRUM, PtrRef(BUF_KERNEL, 0), G, g.K);
  OlsAxis whole;
  whole.fN = whole.plim = whole.L = P; whole.nb = 1;
  ols_store(sp.i, whole, whole, &whole);
  sp.imap = conv_kernel_map(g, pd, 3); sp.omap = Builder::dense_map(pd, 3);
  b.ir.steps.push_back(sp);
  b.ir.route += (real ? "bricks-rspectrum" : "bricks-spectrum") + brick + "] ";
  Step proto = launch(real ? LM_BRICKS_RCONV_OLS : LM_BRICKS_CONV_OLS, PtrRef(BUF_INPUT, 0), PtrRef(BUF_OUTPUT, 0), items);
  proto.i[LS_CONJ] = g.corr ? 1 : 0; proto.i[LS_OLS_WRAP] = wrap ? 1 : 0;
  ols_store(proto.i, ax[0], ax[1], &ax[2]);
  proto.f[F_SCALE] = (float)(1.0 / (double)V);
  proto.imap = conv_load_map(d, g, fs, 3);
  push_per_kernel(b, d, g, proto, LP_MUL_SPECTRUM, G, V * 8);
  b.ir.route += (real ? "bricks-rconv-ols" : "bricks-conv-ols") + brick + ",L=" + std::to_string(ax[0].L) + "x" + std::to_string(ax[1].L) + "x" + std::to_string(ax[2].L) + depthwise_field(g) + (wrap ? ",wrap] " : "] ");
  return true;
}

// y_k = IFFT( FFT(x) .* (conj?)FFT(h_k) ) / Nfft, cropped per boundary, written per output layout / lanes
// (runtime/plans/fftconv.js:308-709, exec :1415-1712; reference semantics: src/utils/math.js:469-603)
int build_fftconv(const mi355fft_plan_desc& d, Builder& b, std::string& err) {
  ConvGeom g;
  if (int rv = conv_geometry(d, 8, g, b.ir, err)) return rv;
  const int rank = g.rank;
  const int64_t K = g.K, B = g.B, inN = g.inN;
  // fftConv.inputChannels C > 1: B * C data lines and K * C kernels, result (k, b) = sum_c x[b C + c] (*) h[k C + c].  The single-channel routes below are
  // not considered; the request takes emit_tiles_ols's sum form (rank 2, linear) or the composed route with the sum in its pointwise pass (fftconv-sum)
  const int64_t C = g.C, BC = B * C, KC = K * g.Cg;      // (fftConv.groups: K Cg kernels, each output kernel summing its group's Cg channels)
  const int64_t *ks = g.ks, *fs = g.fs, zero[8] = {0};
  const bool zpad = d.zero_read.enabled || d.zero_write.enabled;
  // ---- overlap-save: long complex lines, short kernels, one launch per kernel on blocks of P points (kern_lines.hpp fft_lines_conv_ols_kernel has the
  // index map); K P 8 bytes of workspace for any length.  The switch's rule is conv_ols_block
  // Circular requests (PlannerOptions::ols_circular, ols_circular_take) run the kernel's WRAP instances on the rule's block alone
  if (rank == 1 && g.one_channel() && b.opt.conv_ols != 0 && b.opt.conv_lines && !b.opt.force_generic && g.lfN < ((int64_t)1 << 31) - 16384) {
    const int64_t sw = b.opt.conv_ols, rule = conv_ols_block(g.lfN, ks[0]);
    const bool wrap = !g.linear;
    const int64_t P = wrap ? (ols_circular_take(b.opt, d.shape, 1, rule) ? rule : 0) : ols_switch(sw, is_pow2(sw) && sw >= 128 && sw <= 4096, rule);
    const OlsAxis ax = ols_axis(g.lfN, d.shape[0], ks[0], P, g.corr, false, wrap);
    const int64_t lines = B * ax.nb;
    const LineKernelMeta* om = (P && ax.L >= 2 && lines < ((int64_t)1 << 31) - 64 && b.axis_mappable(P, 1, false)) ? find_line_kernel((int)P, false, false, false, false, 0) : nullptr;
    if (om && om->lds_bytes > 0 && om->R1 > 1) {
      const int64_t pd[1] = {P};
      const PtrRef G = b.alloc_work((uint64_t)K * P * 8);
      if (int rv = b.emit_axis_mapped(PtrRef(BUF_KERNEL, 0), G, P, 1, K, false, 1.0f, conv_kernel_map(g, pd, 1), Builder::dense_map(pd, 1), 0)) return rv;
      Step proto = conv_line_proto(b, d, g, *om, LM_CONV_OLS, lines, P, P, b.line_tables(*om));
      ols_store(proto.i, ax);
      proto.i[LS_OLS_WRAP] = wrap ? 1 : 0;
      push_per_kernel(b, d, g, proto, LP_MUL_SPECTRUM, G, P * 8);
      b.ir.route += "lines-conv-ols[N=" + std::to_string(P) + ",L=" + std::to_string(ax.L) + depthwise_field(g) + (wrap ? ",wrap] " : "] ");
      return MI355FFT_OK;
    }
  }
  // ---- overlap-save in two dimensions (emit_tiles_ols); the switch's rule is conv_tiles_block
  if (rank == 2 && b.opt.conv_ols2d != 0 && b.opt.conv_lines && !b.opt.force_generic && b.opt.fuse_views && emit_tiles_ols(b, d, g, false)) return MI355FFT_OK;
  // ---- overlap-save in three dimensions (emit_bricks_ols); the switch's rule is conv_bricks_block
  if (rank == 3 && g.one_channel() && b.opt.conv_ols3d != 0 && b.opt.conv_lines && !b.opt.force_generic && b.opt.fuse_views && emit_bricks_ols(b, d, g, false)) return MI355FFT_OK;
  // Long rank-1 linear modes: the next power of two keeps the transforms off the Bluestein / mixed-radix routes (ConvGeom)
  if (b.opt.conv_pad && rank == 1 && g.linear && g.lfN > 16384 && g.lfN <= ((int64_t)1 << 22) && !is_pow2(g.lfN)) {
    int64_t P = 32768;
    while (P < g.lfN) P <<= 1;
    g.pad_axis0(P);
    b.ir.route += "pad[" + std::to_string(g.lfN) + "->" + std::to_string(P) + "] ";
  }
  const int64_t fN = prodv(fs, rank);
  PtrRef in(BUF_INPUT, 0), out(BUF_OUTPUT, 0), kern(BUF_KERNEL, 0);

  // small 1-D circular problems: one launch, one workgroup per batch entry (kern_fftconv.hpp)
  // (throughput-sized problems do better on the line kernels below: measured 49 vs 150 GPoints/s at N=1024, batch 65536)
  const bool lines_mul_ok = b.opt.conv_lines && is_pow2(fN) && fN >= 64 && fN <= b.opt.max_line;
  if (!b.opt.force_generic && !zpad && rank == 1 && C == 1 && !g.linear && K <= 15 &&
      !(lines_mul_ok && B * fN * K > b.opt.conv_fused_max_points)) {
    const ConvKernelMeta* cm = nullptr;
    for (const auto& m : conv_kernel_registry())
      if (m.N == fN && m.TL >= K + 1 && (!cm || m.TL < cm->TL)) cm = &m;
    if (cm) {
      std::vector<float2h> tw;
      for (int q = 1; q < cm->R1; ++q) for (int k = 0; k < cm->R0; ++k) tw.push_back(root_of_unity((int64_t)q * k, fN));
      Step& st = b.push(ST_FFTCONV_FUSED);
      st.variant = cm->id;
      st.p[FCP_IN] = in; st.p[FCP_KERN] = kern; st.p[FCP_OUT] = out; st.p[FCP_TW] = b.add_table(tw);
      st.i[FC_BATCH] = B; st.i[FC_K] = K; st.i[FC_KERN_LEN] = ks[0]; st.i[FC_CONJ] = g.corr ? 1 : 0;
      st.i[FC_IN_OFFSET] = d.input.strided ? d.input.offset_elements : 0;
      st.i[FC_IN_BATCH_STRIDE] = (d.input.strided && d.input.batch_stride_elements > 0) ? d.input.batch_stride_elements : inN;
      st.i[FC_IN_STRIDE] = d.input.strided ? d.input.strides[0] : 1;
      st.i[FC_OUT_OFFSET] = g.lane0; st.i[FC_OUT_KERNEL_STRIDE] = g.lane_k; st.i[FC_OUT_BATCH_STRIDE] = g.lane_b; st.i[FC_OUT_STRIDE] = d.output.strided ? d.output.strides[0] : 1;
      st.f[F_SCALE] = (float)(1.0 / (double)fN);
      st.grid = (unsigned)std::min<int64_t>(B, (int64_t)b.opt.compute_units * 4);
      b.ir.route += "fftconv-fused[N=" + std::to_string(fN) + ",K=" + std::to_string(K) + ",TL=" + std::to_string(cm->TL) + "] ";
      return MI355FFT_OK;
    }
  }
  const bool embed = g.linear;
  mi355fft_side_layout dense{};  // strided == 0
  // ---- sides fused into the launches (fftconv.js:353-373): the zero-padded embed of kernels and data, the
  // strided lanes and zeroPad.read ride the first forward axis' loads; zeroPad.write, the crop of the linear modes and the output
  // lanes ride the last inverse axis' store pass — where those axes are line-kernel launches
  int fa = -1, la = -1;
  Builder::nd_first_last(fs, rank, 0, fa, la);
  const auto stride_below = [&](int a) { int64_t S = 1; for (int i = 0; i < a; ++i) S *= fs[i]; return S; };
  const bool small = fN < ((int64_t)1 << 31);
  const bool map_fwd = small && fa >= 0 && b.axis_mappable(fs[fa], stride_below(fa), false);
  const bool map_inv = small && la >= 0 && b.axis_mappable(fs[la], stride_below(la), true);
  // 1. kernels: zero-padded into the FFT domain, transformed once per exec
  PtrRef kf = b.alloc_work((uint64_t)KC * fN * 8);
  bool kernel_embed = false;
  for (int i = 0; i < rank; ++i) if (ks[i] != fs[i]) kernel_embed = true;
  int rc;
  if (kernel_embed && map_fwd) {
    const SideMap km = conv_kernel_map(g, fs, rank);
    rc = b.emit_nd(kern, kf, fs, rank, KC, false, 1.0f, err, 0, 0, &km, nullptr);
  } else {
    if (kernel_embed) {
      b.zero(kf, KC * fN * 2);
      b.emit_strided(true, kern, kf, dense, ks, rank, KC, fs, zero, fN, 0);
    }
    rc = b.emit_nd(kernel_embed ? kf : kern, kf, fs, rank, KC, false, 1.0f, err);
  }
  if (rc) return rc;
  // 1b. 2^20-point circular lines, dense on both sides: forward transform, K products and K inverse transforms in ONE persistent launch
  // whose spectrum tiles never leave the registers (kern_regtile.hpp fft_xcd_conv1m_kernel): 56 + 40 (K - 1) B/point instead of 88 + 56 (K - 1)
  // The linear modes (a padded or exact 2^20-point domain) and zeroPad take the kernel's VIEW form: the embed of the data is a predicate of its
  // first loads, crop and zeroPad.write are predicates of its last stores (A reads 8 shape, C writes 8 os bytes per line and kernel)
  if (b.opt.conv_pipeline && !b.opt.force_generic && b.opt.xcd_fused == 1 && b.opt.xcd_shared && !b.opt.only_pass && rank == 1 && C == 1 && fN == ((int64_t)1 << 20) &&
      !d.input.strided && !d.output.strided) {
    const bool view = g.linear || zpad;
    const XcdKernelMeta* xm = nullptr;
    for (const auto& m : xcd_kernel_registry()) if (m.kind == (view ? XK_CONV_VIEW : XK_CONV)) xm = &m;
    if (xm) {
      Builder::XcdLaunch x = b.xcd_launch(*xm, false, 2 * fN, B);   // two slots per data line in a round (W and W2): Builder::xcd_groups
      x.ta = x.tb = b.line_tables(make_meta(0, 1024, 32, 32, 1, 32, true, true, false, false, 0));
      b.xcd_roots(x, fN);
      Step& st = b.push_xcd(ST_XCD_FUSED, xm->id, x, in, view ? out.plus(-g.ooff[0] * 8) : out, B, fN);
      st.i[XS_OUT_PITCH] = g.lane_b;                    // between data lines
      st.i[XS_OUT_KERNEL_PITCH] = g.lane_k;                    // between the kernels of one data line
      st.i[XS_MUL_OFF] = kf.off - x.wslots.off; st.i[XS_CONV_K] = K; st.i[XS_CONV_CONJ] = g.corr ? 1 : 0;
      st.f[F_SCALE] = (float)(1.0 / (double)fN);
      if (view) {
        st.i[XS_IN_PITCH] = inN;                        // the data lines keep their own length: nothing is embedded
        // the launch addresses both sides itself (the pitches above, `out - ooff` as its pointer): its maps carry the ranges
        // only and stay dense over the domain
        st.imap = conv_load_map(d, g, fs, rank);
        st.omap = conv_store_map(d, g, fs, rank, 0);
        st.omap.offset = 0;
        st.imap.batch_stride = st.omap.batch_stride = fN;
        st.i[XS_V_SPLIT] = g.split; st.i[XS_V_SHIFT] = g.padD;
        b.ir.route += "fftconv-pipeline-view[N=1024x1024,K=" + std::to_string(K) + "] ";
      } else b.ir.route += "fftconv-pipeline[N=1024x1024,K=" + std::to_string(K) + "] ";
      return MI355FFT_OK;
    }
  }
  // 2. data: gather (strided lanes) / embed (linear modes) into the dense FFT domain, forward transform once
  PtrRef xf = b.alloc_work((uint64_t)BC * fN * 8);
  const bool side_in = embed || d.input.strided || d.zero_read.enabled;
  const bool fuse_in = side_in && map_fwd;
  const SideMap xmap = fuse_in ? conv_load_map(d, g, fs, rank) : SideMap();
  if (!fuse_in) {
    if (embed) b.zero(xf, BC * fN * 2);
    if (embed || d.input.strided) b.emit_strided(true, in, xf, d.input, d.shape, rank, BC, fs, zero, fN, 0);
    else if (d.zero_read.enabled) { Step& c = b.push(ST_COPY); c.p[P_SRC] = in; c.p[P_DST] = xf; c.i[S_COUNT] = BC * fN * 8; }
    if (d.zero_read.enabled) { emit_zero_outside(b, xf, d.zero_read, fs, rank, BC); b.ir.route += "zero-read "; }
  }
  const bool staged = side_in && !fuse_in;
  // 1-D, power-of-two FFT length with an LDS-resident line kernel: the product with kernel k's spectrum rides the forward FFT's
  // last stage (kern_lines.hpp fft_lines_mul_kernel), one launch per kernel instead of forward FFT + K pointwise passes
  const LineKernelMeta* mul_m = nullptr;
  if (b.opt.conv_lines && !b.opt.force_generic && rank == 1 && C == 1 && is_pow2(fN) && fN <= b.opt.max_line && !(b.opt.xcd_fused == 2 && fN == 4096)) {
    mul_m = find_line_kernel((int)fN, false, false, false, false, 0);
    if (mul_m && (mul_m->lds_bytes == 0 || mul_m->R1 <= 1)) mul_m = nullptr;
  }
  if (!mul_m) {
    rc = fuse_in ? b.emit_nd(in, xf, fs, rank, BC, false, 1.0f, err, 0, 0, &xmap, nullptr)
                 : b.emit_nd(staged ? xf : in, xf, fs, rank, BC, false, 1.0f, err);
    if (rc) return rc;
  }
  const PtrRef mul_tables = mul_m ? b.line_tables(*mul_m) : PtrRef();
  // 3. per kernel: product, inverse transform scaled by 1/Nfft, crop + place
  PtrRef y = b.alloc_work((uint64_t)B * fN * 8);
  const float inv_n = (float)(1.0 / (double)fN);
  const bool direct_out = !embed && !d.output.strided && d.conv_output_layout == MI355FFT_KERNEL_MAJOR;   // the inverse FFT can land in the output itself
  const bool side_out = embed || d.output.strided || d.zero_write.enabled || d.conv_output_layout != MI355FFT_KERNEL_MAJOR;
  const bool fuse_out = side_out && map_inv && g.padD == 0;
  for (int64_t k = 0; k < K; ++k) {
    if (mul_m) {
      Step& st = b.push(ST_LINES);
      st.variant = mul_m->id;
      st.p[LP_IN] = staged ? xf : in; st.p[LP_OUT] = y; st.p[LP_TW] = mul_tables; st.p[LP_MUL_SPECTRUM] = kf.plus(k * fN * 8);
      const int64_t tiles = (B + mul_m->T - 1) / mul_m->T;
      st.i[LS_TILES] = tiles; st.i[LS_LINES] = B; st.i[LS_IN_S] = 1; st.i[LS_IN_OUTER] = fN; st.i[LS_OUT_S] = 1; st.i[LS_OUT_OUTER] = fN;
      st.i[LS_MUL_CONJ] = g.corr ? 1 : 0; st.i[LS_MODE] = LM_MUL;
      st.f[F_SCALE] = 1.0f;
      st.grid = b.lines_grid(*mul_m, tiles);
      if (fuse_in) { st.i[LS_MAPPED] = 1; st.imap = xmap; st.imap.ax = 0; st.omap = Builder::dense_map(fs, rank); }
      if (k == 0) b.ir.route += std::string(fuse_in ? "lines-mul-mapped[N=" : "lines-mul[N=") + std::to_string(fN) + "] ";
    } else {
      Step& pm = b.push(ST_POINTWISE);
      pm.p[P_SRC] = xf.plus((k / g.Kg) * g.Cg * fN * 8); pm.p[P_DST] = y; pm.p[PWP_KERNEL] = kf.plus(k * g.Cg * fN * 8);     // (the group's first channel: a shift of the data pointer)
      pm.i[PW_L] = fN; pm.i[PW_TOTAL] = B * fN; pm.i[PW_CONJ] = g.corr ? 1 : 0; pm.i[PW_CHANNELS] = C > 1 ? g.Cg : 0; pm.i[PW_ITEM_LINES] = g.G > 1 ? C : 0; pm.f[F_SCALE] = 1.0f;
      pm.grid = b.generic_grid(B * fN);
    }
    if (fuse_out) {
      const SideMap om = conv_store_map(d, g, fs, rank, k);
      rc = b.emit_nd(y, y, fs, rank, B, true, inv_n, err, 0, 0, nullptr, &om, out);
      if (rc) return rc;
      continue;
    }
    if (direct_out) {
      const PtrRef lane = out.plus(g.lane_offset(k) * 8);
      rc = b.emit_nd(y, lane, fs, rank, B, true, inv_n, err);
      if (rc) return rc;
      if (d.zero_write.enabled) emit_zero_outside(b, lane, d.zero_write, fs, rank, B);
      continue;
    }
    rc = b.emit_nd(y, y, fs, rank, B, true, inv_n, err);
    if (rc) return rc;
    if (d.zero_write.enabled) emit_zero_outside(b, y, g.padded(d.zero_write), fs, rank, B);
    conv_staged_crop(b, d, g, out, y, k, false);
  }
  if (d.zero_write.enabled && !fuse_out) b.ir.route += "zero-write ";
  b.ir.route += C > 1 ? "fftconv-sum[K=" + std::to_string(K) + ",C=" + std::to_string(C) + (g.G > 1 ? ",G=" + std::to_string(g.G) : std::string()) + "] " : "fftconv[K=" + std::to_string(K) + "] ";
  return MI355FFT_OK;
}

// ---- fftconv over real data (type MI355FFT_FFTCONV_REAL) ------------------------------------------------------------------------
// Signals, kernels and results are f32 reals; the values are the real parts of what build_fftconv's plan returns for the same data
// with zero imaginary parts.  Every option keeps its meaning; side layouts and the kernel stride count f32 elements.  Six routes:
//   bricks-rconv-ols[N=16x16x16,L=L0xL1xL2]  rank 3, linear modes, volumes with small kernels by default (rconv_bricks_block; MI355FFT_RCONV_OLS3D): overlap-save
//                     on pairs of 16^3 bricks (emit_bricks_ols)
//   tiles-rconv-ols[N=PxP,L=L0xL1]  rank 2, linear modes, images with small kernels by default (rconv_tiles_block; MI355FFT_RCONV_OLS2D): overlap-save on
//                     pairs of P x P tiles (emit_tiles_ols)
//   lines-rconv-ols[N=P,L=L]  rank 1, linear modes, shape + kernelShape - 1 > 8192 and kernelShape <= 4096 by default (MI355FFT_RCONV_OLS): overlap-save
//                     on blocks of P points (what the overlap-save routes share is said once, above ols_switch)
//   lines-rconv[N=P]  rank 1, FFT length P a power of two, 128 <= P <= 8192 by default (16384 and 32768 with strided sides or MI355FFT_RCONV_FUSED=2) (circular: P = shape; linear modes: the next power of two
//                     >= max(shape + kernelShape - 1, 128) — a linear result is cropped, so any P >= that length is legal): one
//                     lines-r2c-mapped launch writes the K packed kernel spectra, then ONE launch per kernel does r2c, product and c2r
//                     of a data line inside LDS (kern_lines.hpp fft_lines_rconv_kernel).  Strided lanes, the embed, zeroPad and the
//                     crop ride its two address maps: 4 B read + 4 B written per real point and kernel, 1 + K launches
//   rconv[K]          everything else whose axis-0 FFT length can be made even (all linear requests: axis 0 is rounded up — rank 1 to
//                     the next power of two up to 2^22; circular requests with even shape[0]); any rank; dense sides: the real
//                     emitters on kernels and data, then per kernel a pointwise pass over the packed bins, the inverse, zeroPad.write
//                     and the real crop
//   rconv-widened     circular with odd shape[0] (no even domain is allowed): the complex plan between widening / narrowing passes
// The three overlap-save routes also take circular requests inside their bounds (tags ending in ",wrap]": ols_circular_take), odd lines and strided sides
// of rank 2 and 3 among them, which then have a direct plan
// Validation, shapes, lanes and the padded-domain index map are ConvGeom's, shared with build_fftconv; each route hands it the
// axis-0 length it transforms on.
constexpr int64_t OLS_MAX_KERNEL = 4096;   // the longest kernel the default rule gives to overlap-save: the longest one measured (3.8x / 2.5x ahead at K = 1 / 4)
int build_fftconv_real(const mi355fft_plan_desc& d, Builder& b, std::string& err) {
  ConvGeom g;
  if (int rv = conv_geometry(d, 4, g, b.ir, err)) return rv;
  const int rank = g.rank;
  const int64_t K = g.K, B = g.B, inN = g.inN, kN = g.kN, oN = g.oN, lfN = g.lfN;
  const int64_t C = g.C;      // fftConv.inputChannels > 1 (build_fftconv): emit_tiles_ols's sum form or rconv-sum, the composed route summing over c in its pointwise pass
  const bool linear = g.linear, corr = g.corr;
  const int64_t *ks = g.ks, *fs = g.fs, zero[8] = {0};
  const bool strided = d.input.strided || d.output.strided;
  const PtrRef in(BUF_INPUT, 0), out(BUF_OUTPUT, 0), kern(BUF_KERNEL, 0);

  // ---- overlap-save: long real lines, short kernels, one launch per kernel on blocks of P points, each running the pipeline of lines-rconv
  // (kern_lines.hpp fft_lines_rconv_ols_kernel has the index map).  The switch's rule, whatever the line's length when a block is forced:
  // Circular requests (PlannerOptions::ols_circular, ols_circular_take) run the kernel's WRAP instances on the rule's block alone
  if (rank == 1 && g.one_channel() && b.opt.rconv_fused == 1 && b.opt.rconv_ols != 0 && !(b.opt.force_generic && !linear) && lfN < ((int64_t)1 << 31) - 16384) {
    const int64_t M = ks[0], sw = b.opt.rconv_ols;
    const bool wrap = !linear;
    // measured (profiles/fftconv_ols_ab.log, 256 x 2^20 (*) {31, 255, 1024, 4096}, K = 1 and 4, and three longer / shorter lines): every block length
    // 1024 .. 8192 is 2.5-8x ahead of pad[..] rconv[K] and 46-66x ahead of the Bluestein plans above 2^22; the fastest P is the smallest power of two
    // >= 8 (M - 1) from 1024 on (M = 31: 1024, 255: 2048, 1024 and 4096: 8192), except that P = 4096 is behind 8192 on every request (its instance
    // holds 190 VGPRs: two workgroups per CU where the LDS would take three) and is never chosen
    int64_t rule = 0;
    if (lfN > 8192 && M <= OLS_MAX_KERNEL) { rule = 1024; while (rule < 8 * (M - 1) && rule < 8192) rule <<= 1; if (rule == 4096) rule = 8192; }
    const int64_t P = wrap ? (ols_circular_take(b.opt, d.shape, 1, rule) ? rule : 0) : ols_switch(sw, is_pow2(sw) && sw >= 128 && sw <= 8192, rule);
    const OlsAxis ax = ols_axis(lfN, d.shape[0], M, P, corr, true, wrap);
    const int64_t lines = B * ax.nb;
    const LineKernelMeta* om = (P && ax.L >= 2 && lines < ((int64_t)1 << 31) - 64) ? b.lines_r2c_kernel(P, false, true) : nullptr;
    if (om) {
      const int64_t H = P / 2;
      const int64_t pd[1] = {P}, pp[1] = {H + 1};
      const PtrRef G = b.alloc_work((uint64_t)K * (H + 1) * 8);
      const SideMap km = conv_kernel_map(g, pd, 1);
      const SideMap gm = Builder::dense_map(pp, 1);
      if (!b.emit_lines_r2c(kern, G, P, K, 1.0f, false, 0, &km, &gm)) { err = "no mapped r2c line kernel"; return MI355FFT_ERR_UNSUPPORTED; }
      const PtrRef tables = b.line_tables(*om), proots = b.rconv_roots(P);
      Step proto = conv_line_proto(b, d, g, *om, LM_RCONV_OLS, lines, H, P, tables, proots);
      ols_store(proto.i, ax);
      proto.i[LS_OLS_WRAP] = wrap ? 1 : 0;
      push_per_kernel(b, d, g, proto, LP_RCONV_SPECTRUM, G, (H + 1) * 8);
      b.ir.route += "lines-rconv-ols[N=" + std::to_string(P) + ",L=" + std::to_string(ax.L) + depthwise_field(g) + (wrap ? ",wrap] " : "] ");
      return MI355FFT_OK;
    }
  }
  // ---- overlap-save in two dimensions on real tile pairs (emit_tiles_ols); the switch's rule is rconv_tiles_block
  if (rank == 2 && (linear || b.opt.fuse_views) && b.opt.rconv_ols2d != 0 && b.opt.rconv_fused != 0 && !b.opt.force_generic && emit_tiles_ols(b, d, g, true)) return MI355FFT_OK;
  // ---- overlap-save in three dimensions on real brick pairs (emit_bricks_ols); the switch's rule is rconv_bricks_block
  if (rank == 3 && g.one_channel() && (linear || b.opt.fuse_views) && b.opt.rconv_ols3d != 0 && b.opt.rconv_fused != 0 && !b.opt.force_generic && emit_bricks_ols(b, d, g, true)) return MI355FFT_OK;

  // ---- route 1: one launch per kernel on the line kernels --------------------------------------------------------------------
  int64_t P1 = 0;
  if (rank == 1 && !linear) { if (is_pow2(lfN) && lfN >= 128 && lfN <= 32768) P1 = lfN; }
  else if (rank == 1 && lfN <= 32768) { P1 = 128; while (P1 < lfN) P1 <<= 1; }
  // measured (profiles/fftconv_real_ab.log): the one-launch route is ahead of rconv[K] up to P = 8192 (1.3-1.9x at K = 1, 1.0-1.5x at K = 4); at
  // P = 16384 and 32768 it ties at K = 1 and loses at K = 4 (0.75x: 40 registers spilt, one or two workgroups per CU running the stages twice
  // behind barriers), so those lengths take rconv[K] unless a side is strided (only the line route's address maps carry lanes) or the
  // switch is 2 (every length: tests and measurement)
  const bool route1 = b.opt.rconv_fused == 2 || (b.opt.rconv_fused == 1 && (P1 <= 8192 || strided));
  const LineKernelMeta* rm = (P1 && route1 && C == 1) ? b.lines_r2c_kernel(P1, false, true) : nullptr;
  if (rm) {
    const int64_t P = P1, H = P / 2;
    g.pad_axis0(P);
    if (g.padD) b.ir.route += "pad[" + std::to_string(lfN) + "->" + std::to_string(P) + "] ";
    const int64_t pp[1] = {H + 1};
    // the K kernels, zero-embedded kN -> P by the load predicate, as packed spectra in the workspace
    const PtrRef G = b.alloc_work((uint64_t)K * (H + 1) * 8);
    const SideMap km = conv_kernel_map(g, fs, 1), gm = Builder::dense_map(pp, 1);
    if (!b.emit_lines_r2c(kern, G, P, K, 1.0f, false, 0, &km, &gm)) { err = "no mapped r2c line kernel"; return MI355FFT_ERR_UNSUPPORTED; }
    const PtrRef tables = b.line_tables(*rm), proots = b.rconv_roots(P);
    Step proto = conv_line_proto(b, d, g, *rm, LM_RCONV, B, H, P, tables, proots);
    proto.i[LS_RCONV_SPLIT] = g.split; proto.i[LS_RCONV_PADD] = g.padD;
    push_per_kernel(b, d, g, proto, LP_RCONV_SPECTRUM, G, (H + 1) * 8);
    b.ir.route += "lines-rconv[N=" + std::to_string(P) + "] ";
    return MI355FFT_OK;
  }
  if (strided) { err = "Unsupported: strided layouts on real fftconv outside the one-launch line route"; return MI355FFT_ERR_UNSUPPORTED; }

  // ---- route 3: circular, odd shape[0]: the complex plan between a widening and a narrowing pass ----------------------------------
  if (!linear && (lfN & 1)) {
    if (C > 1) { err = "Unsupported: fftConv.inputChannels > 1 on real circular fftconv with odd shape[0] (no even FFT domain; use complex data)"; return MI355FFT_ERR_UNSUPPORTED; }
    mi355fft_plan_desc dc = d;
    dc.type = MI355FFT_FFTCONV;
    if (int rc = build_fftconv(dc, b, err)) return rc;
    PlanIR& ir = b.ir;
    const uint64_t in_c = (uint64_t)B * inN * 8, k_c = (uint64_t)K * kN * 8, out_c = (uint64_t)K * B * oN * 8;
    const uint64_t in_stage = align_up(ir.work_bytes, 256), k_stage = align_up(in_stage + in_c, 256), out_stage = align_up(k_stage + k_c, 256);
    ir.work_bytes = align_up(out_stage + out_c, 256);
    const auto convert = [&](StepKind kind, PtrRef src, PtrRef dst, int64_t count) { return convert_step(kind, src, dst, count, b.generic_grid(count)); };
    restage(ir, in_stage, out_stage, k_stage,
            {convert(ST_REAL_TO_COMPLEX, in, PtrRef(BUF_WORK, (int64_t)in_stage), B * inN), convert(ST_REAL_TO_COMPLEX, kern, PtrRef(BUF_WORK, (int64_t)k_stage), K * kN)},
            {convert(ST_COMPLEX_TO_REAL, PtrRef(BUF_WORK, (int64_t)out_stage), out, K * B * oN)});
    ir.in_bytes = in_c / 2; ir.kernel_bytes = k_c / 2; ir.out_bytes = out_c / 2;
    ir.route = "rconv-widened " + ir.route;
    return MI355FFT_OK;
  }

  // ---- route 2: composed from the real emitters --------------------------------------------------------------------------------
  // rank-1 linear requests take the next power of two (any domain >= lfN gives the same cropped values, and the half-length transforms
  // stay off the mixed-radix / Bluestein routes); other linear requests round axis 0 up to an even length
  if (linear) {
    int64_t P = lfN + (lfN & 1);
    if (rank == 1 && b.opt.conv_pad && lfN <= ((int64_t)1 << 22)) { P = 2; while (P < lfN) P <<= 1; }
    g.pad_axis0(P);
  }
  if (g.padD) b.ir.route += "pad[" + std::to_string(lfN) + "->" + std::to_string(fs[0]) + "] ";
  int64_t ps[8];
  for (int i = 0; i < rank; ++i) ps[i] = fs[i];
  ps[0] = fs[0] / 2 + 1;
  const int64_t fN = prodv(fs, rank), pN = prodv(ps, rank), F0 = fs[0];
  const bool mapped0 = rank == 1 && fN < ((int64_t)1 << 31) && b.lines_r2c_kernel(F0, false, true) != nullptr;
  mi355fft_side_layout dense{};
  int rc;
  // real lines [count][shape] -> packed spectra [count][ps]: embedded into the FFT domain (zeros elsewhere), restricted to `zr`;
  // `im`: the same as the address map of a line launch
  const auto forward = [&](PtrRef src, PtrRef dst, const int64_t* shp, int64_t count, const mi355fft_zero_range* zr, const SideMap& im) -> int {
    bool emb = false;
    for (int i = 0; i < rank; ++i) if (shp[i] != fs[i]) emb = true;
    if ((emb || zr) && mapped0) {
      const SideMap om = Builder::dense_map(ps, 1);
      if (!b.emit_lines_r2c(src, dst, F0, count, 1.0f, false, 0, &im, &om)) { err = "no mapped r2c line kernel"; return MI355FFT_ERR_UNSUPPORTED; }
      return MI355FFT_OK;
    }
    PtrRef cur = src;
    if (emb || zr) {
      const PtrRef xr = b.alloc_work((uint64_t)count * fN * 4);
      if (emb) {
        b.zero(xr, count * fN);
        b.emit_strided(true, src, xr, dense, shp, rank, count, fs, zero, fN, 0, true);
      } else { Step& c = b.push(ST_COPY); c.p[P_SRC] = src; c.p[P_DST] = xr; c.i[S_COUNT] = count * fN * 4; }
      if (zr) {
        emit_zero_outside(b, xr, g.padded(*zr), fs, rank, count, true);
        b.ir.route += "zero-read ";
      }
      cur = xr;
    }
    if (int r = b.emit_r2c_even(cur, dst, F0, count * (fN / F0), 1.0f, err)) return r;
    if (rank > 1) return b.emit_nd(dst, dst, ps, rank, count, false, 1.0f, err, 1);
    return MI355FFT_OK;
  };
  const PtrRef kf = b.alloc_work((uint64_t)K * g.Cg * pN * 8);
  if ((rc = forward(kern, kf, ks, K * g.Cg, nullptr, conv_kernel_map(g, fs, 1)))) return rc;
  const PtrRef xf = b.alloc_work((uint64_t)B * C * pN * 8);
  if ((rc = forward(in, xf, d.shape, B * C, d.zero_read.enabled ? &d.zero_read : nullptr, conv_load_map(d, g, fs, 1)))) return rc;
  const PtrRef y = b.alloc_work((uint64_t)B * pN * 8);
  const bool direct_out = !linear && d.conv_output_layout == MI355FFT_KERNEL_MAJOR;     // the real inverse can land in the output itself
  const PtrRef yr = direct_out ? PtrRef() : b.alloc_work((uint64_t)B * fN * 4);
  const float inv_n = (float)(1.0 / (double)fN);
  for (int64_t k = 0; k < K; ++k) {
    Step& pm = b.push(ST_POINTWISE);
    pm.p[P_SRC] = xf.plus((k / g.Kg) * g.Cg * pN * 8); pm.p[P_DST] = y; pm.p[PWP_KERNEL] = kf.plus(k * g.Cg * pN * 8);
    pm.i[PW_L] = pN; pm.i[PW_TOTAL] = B * pN; pm.i[PW_CONJ] = corr ? 1 : 0; pm.i[PW_CHANNELS] = C > 1 ? g.Cg : 0; pm.i[PW_ITEM_LINES] = g.G > 1 ? C : 0; pm.f[F_SCALE] = 1.0f;
    pm.grid = b.generic_grid(B * pN);
    if (rank > 1 && (rc = b.emit_nd(y, y, ps, rank, B, true, 1.0f, err, 1))) return rc;
    const PtrRef dst = direct_out ? out.plus(g.lane_offset(k) * 4) : yr;
    if ((rc = b.emit_c2r_even(y, dst, F0, B * (fN / F0), inv_n, err))) return rc;
    if (d.zero_write.enabled) emit_zero_outside(b, dst, g.padded(d.zero_write), fs, rank, B, true);
    if (!direct_out) conv_staged_crop(b, d, g, out, yr, k, true);
  }
  if (d.zero_write.enabled) b.ir.route += "zero-write ";
  b.ir.route += C > 1 ? "rconv-sum[K=" + std::to_string(K) + ",C=" + std::to_string(C) + (g.G > 1 ? ",G=" + std::to_string(g.G) : std::string()) + "] " : "rconv[K=" + std::to_string(K) + "] ";
  return MI355FFT_OK;
}

// ---- precision "f16-storage" (reference src/kernels/f16_storage.js; runtime/plans/c2c.js:1036-1050, 3840-3861, 4163-4180) ----
// The checks the reference makes before planning: custom strides (layout.strides, whdcn) and fftconv take f32 only.
int validate_f16_storage(const mi355fft_plan_desc& d, std::string& err) {
  if (d.type == MI355FFT_FFTCONV || d.type == MI355FFT_FFTCONV_REAL) { err = "fftconv supports precision:\"f32\" only in current implementation"; return MI355FFT_ERR_INVALID; }
  if (d.input.strided || d.output.strided) {
    if (d.type >= MI355FFT_DCT1) err = "custom strides for dct/dst currently support precision:\"f32\" only";
    else err = std::string("custom strides currently support precision:\"f32\" only") + (d.type == MI355FFT_R2C ? " for r2c" : d.type == MI355FFT_C2R ? " for c2r" : "");
    return MI355FFT_ERR_INVALID;
  }
  return MI355FFT_OK;
}

// The f32 plan is built as usual and then given binary16 sides.  Where that plan is one dense ROW line launch (c2c lines[N], r2c
// lines-r2c[N], c2r lines-c2r[N]) the launch itself reads and writes binary16 (the H16 instances of kern_lines.hpp): 8 B per complex
// point instead of 16, no staging.  Every other route runs unchanged on f32 staging regions behind the f32 plan's workspace:
// binary16 -> f32 of the input in front, f32 -> binary16 of the output behind (and of the caller's output in front as well when
// ioView.output keeps untouched elements, clearOutside: false).  Extents halve; real sides round up to 4 bytes.
bool fuse_f16_storage(PlanIR& ir) {
  if (ir.steps.size() != 1) return false;
  Step& s = ir.steps[0];
  if (s.kind != ST_LINES || s.i[LS_MAPPED] != 0 || s.i[LS_MODE] < LM_C2C || s.i[LS_MODE] > LM_C2R) return false;
  if (!s.p[LP_IN].same(PtrRef(BUF_INPUT, 0)) || !s.p[LP_OUT].same(PtrRef(BUF_OUTPUT, 0))) return false;
  const LineKernelMeta& m = line_kernel_registry()[(size_t)s.variant];
  if (m.in_col || m.out_col || m.twid != 0 || m.swap_in != m.swap_out) return false;
  if (s.i[LS_MODE] == LM_C2C && (s.i[LS_IN_S] != 1 || s.i[LS_OUT_S] != 1 || s.i[LS_IN_OUTER] != m.N || s.i[LS_OUT_OUTER] != m.N)) return false;   // c2c: dense lines, no pitches
  s.i[LS_H16] = 1;
  ir.route += "f16 ";
  return true;
}

void wrap_f16_storage(const mi355fft_plan_desc& d, PlanIR& ir) {
  const uint64_t in32 = ir.in_bytes, out32 = ir.out_bytes;
  ir.in_bytes = align_up(in32 / 2, 4);
  ir.out_bytes = align_up(out32 / 2, 4);
  if (fuse_f16_storage(ir)) return;
  const auto grid = [](int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(((n + 7) / 8 + 255) / 256, Builder::MAX_BLOCKS)); };   // 8 scalars a lane
  const uint64_t in_stage = align_up(ir.work_bytes, 256);
  const uint64_t out_stage = d.in_place ? in_stage : align_up(in_stage + in32, 256);
  ir.work_bytes = d.in_place ? align_up(in_stage + in32, 256) : align_up(out_stage + out32, 256);
  const auto convert = [&](StepKind kind, PtrRef src, PtrRef dst, uint64_t scalars) { return convert_step(kind, src, dst, (int64_t)scalars, grid((int64_t)scalars)); };
  const bool keep_out = d.io_output.enabled && !d.io_output.clear_outside;
  std::vector<Step> front{convert(ST_F16_TO_F32, PtrRef(BUF_INPUT, 0), PtrRef(BUF_WORK, (int64_t)in_stage), in32 / 4)};
  if (keep_out) front.push_back(convert(ST_F16_TO_F32, PtrRef(BUF_OUTPUT, 0), PtrRef(BUF_WORK, (int64_t)out_stage), out32 / 4));
  restage(ir, in_stage, out_stage, 0, front,
          {convert(ST_F32_TO_F16, PtrRef(BUF_WORK, (int64_t)out_stage), PtrRef(d.in_place ? BUF_INPUT : BUF_OUTPUT, 0), out32 / 4)});
  ir.route = std::string(keep_out ? "f16-in+out " : "f16-in ") + ir.route + "f16-out ";
}

}  // namespace

int build_plan_f32(const mi355fft_plan_desc& desc, const PlannerOptions& opt, PlanIR& out, std::string& err);

AliasVariant alias_variant(const PlanIR& ir, uint64_t in_off, uint64_t out_off, std::string& err) {
  const mi355fft_plan_desc& d = ir.desc;
  if (d.in_place || d.type != MI355FFT_C2C) return ALIAS_AS_IS;
  if (!(in_off < out_off + ir.out_bytes && out_off < in_off + ir.in_bytes)) return ALIAS_AS_IS;
  if (d.input.strided || d.output.strided) return ALIAS_AS_IS;
  if (d.io_input.enabled || d.io_output.enabled) return ALIAS_STAGED;
  if (in_off == out_off) return ALIAS_AS_IS;
  err = "output range overlaps the input range at another offset: run the plan on one range (same buffer and offset) or on two disjoint ones";
  return ALIAS_REFUSED;
}

int build_plan(const mi355fft_plan_desc& desc, const PlannerOptions& opt, PlanIR& out, std::string& err) {
  out = PlanIR();
  out.desc = desc;
  int rc = validate_common(desc, err);
  if (rc) return rc;
  const bool f16 = desc.precision == MI355FFT_PRECISION_F16_STORAGE;
  if (f16 && (rc = validate_f16_storage(desc, err))) return rc;
  // c2c N = 8192 under f16: the LDS ROW instance (LINE_ROW(8192, ...)) takes binary16 sides; line-reg has no such instance
  if (f16 && desc.type == MI355FFT_C2C && opt.line32k >= 1) {
    PlannerOptions o = opt;
    o.line32k = 0;
    PlanIR probe;
    std::string e2;
    if (build_plan_f32(desc, o, probe, e2) == MI355FFT_OK && probe.steps.size() == 1 && probe.steps[0].kind == ST_LINES) {
      wrap_f16_storage(desc, probe);
      if (probe.steps.size() == 1) { out = probe; return MI355FFT_OK; }
    }
  }
  rc = build_plan_f32(desc, opt, out, err);
  if (rc) return rc;
  if (f16) wrap_f16_storage(desc, out);
  return MI355FFT_OK;
}

int build_plan_f32(const mi355fft_plan_desc& desc, const PlannerOptions& opt, PlanIR& out, std::string& err) {
  out = PlanIR();
  out.desc = desc;
  int rc;
  Builder b(out, opt);
  switch (desc.type) {
    case MI355FFT_C2C: rc = build_c2c(desc, b, err); break;
    case MI355FFT_R2C: rc = build_r2c(desc, b, err); break;
    case MI355FFT_C2R: rc = build_c2r(desc, b, err); break;
    case MI355FFT_DCT1: case MI355FFT_DCT2: case MI355FFT_DCT3: case MI355FFT_DCT4:
    case MI355FFT_DST1: case MI355FFT_DST2: case MI355FFT_DST3: case MI355FFT_DST4: rc = build_trig(desc, b, err); break;
    case MI355FFT_FFTCONV: rc = build_fftconv(desc, b, err); break;
    case MI355FFT_FFTCONV_REAL: rc = build_fftconv_real(desc, b, err); break;
    default: err = "type must be one of \"c2c\", \"r2c\", \"c2r\", \"fftconv\" (other createPlan types are outside the MI355X hot path)"; rc = MI355FFT_ERR_UNSUPPORTED;
  }
  if (rc) return rc;
  if (out.table.empty()) out.table.push_back(float2h{1, 0});
  return MI355FFT_OK;
}

}  // namespace mi355
