// emu.cpp — host emulation of the HIP kernels for the GPU-less CPU test tier (tests/test_emu_*.py).
//
// TEST INFRASTRUCTURE ONLY.  Compiles webgpu-fft_amd/csrc/kern_*.hpp with -DMI355_HOST_EMU (see
// csrc/platform.hpp) and runs a planned transform on host memory: one std::thread per GPU thread, a
// pthread barrier for __syncthreads().  It exists so kernel index math / LDS layouts / barrier placement
// and the planner can be checked against the oracle (and under ASan/UBSan) where there is no GPU.
// Nothing here is linked into libmi355fft.so; the product has no CPU fallback.
#include <pthread.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "dispatch.hpp"

namespace emu {
thread_local dim3_t t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local char* t_smem = nullptr;
unsigned g_xcds = 2;
static thread_local pthread_barrier_t* t_barrier = nullptr;
static thread_local pthread_barrier_t* t_wave_barrier = nullptr;
void sync_threads() { pthread_barrier_wait(t_barrier); }
void sync_wave() { pthread_barrier_wait(t_wave_barrier); }
}  // namespace emu

namespace {

struct EmuLauncher {
  // every kernel is a grid-stride loop: a few blocks exercise the stride path (MI355_EMU_MAX_GRID overrides,
  // e.g. to make grid*T a multiple of the four-step group so the hoisted-roots path runs)
  unsigned max_grid = std::getenv("MI355_EMU_MAX_GRID") ? (unsigned)std::atoi(std::getenv("MI355_EMU_MAX_GRID")) : 3;
  template <class... P, class... A>
  void launch(void (*kernel)(P...), unsigned grid, unsigned block, unsigned smem, A&&... args) {
    const unsigned g = std::min(grid, max_grid);
    std::vector<char> shared(std::max<size_t>(smem, 64 * 1024) + 64);
    char* smem_base = shared.data() + (64 - (reinterpret_cast<uintptr_t>(shared.data()) & 63)) % 64;
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, block);
    const unsigned waves = (block + 63) / 64;
    std::vector<pthread_barrier_t> wbar(waves);
    for (unsigned w = 0; w < waves; ++w) pthread_barrier_init(&wbar[w], nullptr, std::min(64u, block - 64 * w));
    std::vector<std::thread> th;
    th.reserve(block);
    auto body = [&](unsigned tid) {
      emu::t_barrier = &bar;
      emu::t_wave_barrier = &wbar[tid / 64];
      emu::t_smem = smem_base;
      emu::t_blockDim.x = block;
      emu::t_gridDim.x = g;
      emu::t_threadIdx.x = tid;
      for (unsigned b = 0; b < g; ++b) {
        emu::t_blockIdx.x = b;
        kernel(args...);
        pthread_barrier_wait(&bar);  // next block reuses the shared memory
      }
    };
    for (unsigned t = 0; t < block; ++t) th.emplace_back(body, t);
    for (auto& t : th) t.join();
    pthread_barrier_destroy(&bar);
    for (auto& w : wbar) pthread_barrier_destroy(&w);
  }
  void copy(void* dst, const void* src, size_t bytes) { std::memmove(dst, src, bytes); }

  unsigned sticky = 0;
  unsigned* sticky_error_word() { return &sticky; }
  // kernels whose workgroups synchronise with each other (kern_xcd.hpp): every block gets its own threads,
  // barrier and shared memory, and all blocks run at the same time
  template <class... P, class... A>
  void launch_concurrent(void (*kernel)(P...), unsigned grid, unsigned block, unsigned smem, A&&... args) {
    const size_t bytes = std::max<size_t>(smem, 64 * 1024) + 64;
    std::vector<std::vector<char>> shared(grid, std::vector<char>(bytes));
    std::vector<pthread_barrier_t> bars(grid);
    for (auto& b : bars) pthread_barrier_init(&b, nullptr, block);
    const unsigned waves = (block + 63) / 64;
    std::vector<pthread_barrier_t> wbars((size_t)grid * waves);
    for (unsigned b = 0; b < grid; ++b)
      for (unsigned w = 0; w < waves; ++w) pthread_barrier_init(&wbars[(size_t)b * waves + w], nullptr, std::min(64u, block - 64 * w));
    std::vector<std::thread> th;
    th.reserve((size_t)grid * block);
    for (unsigned b = 0; b < grid; ++b)
      for (unsigned t = 0; t < block; ++t)
        th.emplace_back([&, b, t] {
          emu::t_barrier = &bars[b];
          emu::t_wave_barrier = &wbars[(size_t)b * waves + t / 64];
          emu::t_smem = shared[b].data() + (64 - (reinterpret_cast<uintptr_t>(shared[b].data()) & 63)) % 64;
          emu::t_blockDim.x = block; emu::t_gridDim.x = grid; emu::t_threadIdx.x = t; emu::t_blockIdx.x = b;
          kernel(args...);
        });
    for (auto& t : th) t.join();
    for (auto& b : bars) pthread_barrier_destroy(&b);
    for (auto& w : wbars) pthread_barrier_destroy(&w);
  }
};

// records the launch shape of a fused-kernel dispatch case instead of launching (emu_check_xcd_registry)
struct ShapeProbe {
  unsigned block = 0, smem = 0;
  template <class... P, class... A>
  void launch_concurrent(void (*)(P...), unsigned, unsigned b, unsigned s, A&&...) { block = b; smem = s; }
};

}  // namespace

extern "C" {

// registry metadata must agree with the LineCfg constants the kernels were compiled with
int emu_check_registry(char* msg, size_t msg_bytes) {
  using namespace mi355;
  int cur = 0, bad = 0;
  const auto& reg = line_kernel_registry();
#define CHECK(N_, R0_, R1_, R2_, T_, IC, OC, SI, SO, TW)                                                     \
  {                                                                                                          \
    using C = LineCfg<N_, R0_, R1_, R2_, T_, IC, OC, SI, SO, TW>;                                            \
    const LineKernelMeta& m = reg[(size_t)cur];                                                              \
    if (m.threads != C::THREADS || m.lds_bytes != C::LDS_BYTES || m.tw_elems != C::TW_ELEMS || m.N != N_) {  \
      std::snprintf(msg, msg_bytes, "registry mismatch at id %d (N=%d)", cur, N_);                           \
      ++bad;                                                                                                 \
    }                                                                                                        \
    ++cur;                                                                                                   \
  }
#define LINE_ROW(N, R0, R1, R2, T) CHECK(N, R0, R1, R2, T, false, false, false, false, 0) CHECK(N, R0, R1, R2, T, false, false, true, true, 0)
#define LINE_ROW_TRIG(N, R0, R1, R2, T) CHECK(N, R0, R1, R2, T, false, false, false, false, 4)
#define LINE_PASS_A(N, R0, R1, R2, T) CHECK(N, R0, R1, R2, T, true, true, false, false, 0) CHECK(N, R0, R1, R2, T, true, true, true, false, 0) CHECK(N, R0, R1, R2, T, true, true, true, true, 0)
#define LINE_PASS_B(N, R0, R1, R2, T) CHECK(N, R0, R1, R2, T, false, true, false, false, 2) CHECK(N, R0, R1, R2, T, false, true, false, true, 2)
#define LINE_COL_RAGGED(N, R0, R1, R2, T) CHECK(N, R0, R1, R2, T, true, true, false, false, 3) CHECK(N, R0, R1, R2, T, true, true, true, true, 3)
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
#undef CHECK
  if (cur != (int)reg.size()) { std::snprintf(msg, msg_bytes, "registry size %d != %zu", cur, reg.size()); ++bad; }
  return bad;
}

// the fused registry's threads and LDS bytes (they decide co-residency: plan.cpp xcd_launch) must be what each instance's
// dispatch case launches with
int emu_check_xcd_registry(char* msg, size_t msg_bytes) {
  using namespace mi355;
  int bad = 0;
  for (const XcdKernelMeta& m : xcd_kernel_registry()) {
    ShapeProbe p;
    if (!launch_xcd_fused(m.id, XcdFusedArgs{}, 1u, p) || (int)p.block != m.threads || (int)p.smem != m.lds_bytes) {
      std::snprintf(msg, msg_bytes, "fused registry mismatch at id %d (%dx%d): launched %u threads, %u B of LDS; registry %d, %d", m.id, m.N1, m.N2,
                    p.block, p.smem, m.threads, m.lds_bytes);
      ++bad;
    }
  }
  return bad;
}

// Plans `desc` and runs it on host buffers.  input/output/kernel are host pointers of at least the byte
// extents the plan reports (checked).  output == NULL for in-place plans.  Returns the planner status or
// 100+ for harness errors; err receives the message; route (optional) the plan's route string.
// input == NULL plans only.  work_fill: the byte the workspace (and its 256 spare bytes) is filled with before the first launch; tail_modified (optional) is set
// when a launch changed one of the spare bytes behind the workspace.
int emu_run_plan_ex(const mi355fft_plan_desc* desc, void* input, uint64_t input_bytes, void* output, uint64_t output_bytes, void* kernel,
                    uint64_t kernel_bytes, int force_generic, uint64_t chunk_bytes, int work_fill, int* tail_modified, char* err, size_t err_bytes,
                    char* route, size_t route_bytes, int* launches) {
  using namespace mi355;
  PlannerOptions opt;
  opt.force_generic = force_generic;
  if (chunk_bytes) opt.chunk_bytes = chunk_bytes;
  opt.compute_units = std::getenv("MI355_EMU_CUS") ? std::atoi(std::getenv("MI355_EMU_CUS")) : 2;
  if (const char* e = std::getenv("MI355_EMU_XCD_FUSED")) opt.xcd_fused = std::atoi(e); else opt.xcd_fused = 0;
  if (const char* e = std::getenv("MI355_EMU_XCD_SPLIT")) opt.xcd_split = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_FUSE_VIEWS")) opt.fuse_views = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_RES")) opt.xcd_res = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_RES_DEPTH")) opt.xcd_res_depth = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_SLOTS")) opt.xcd_slots = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_MIXED_LINES")) opt.mixed_lines = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_MIXED_CT")) opt.mixed_ct = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_MAX_LINE")) opt.max_line = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_2D")) opt.xcd_2d = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_RT")) opt.xcd_rt = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_XCD_HX")) opt.xcd_hx = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_CONV_PIPELINE")) opt.conv_pipeline = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_LINES_R2C")) opt.lines_r2c = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_LINES_C2R")) opt.lines_c2r = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_TRIG_REAL")) opt.trig_real = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_TRIG_FUSED")) opt.trig_fused = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_TRIG_ALT")) opt.trig_alt = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_LINE32K")) opt.line32k = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_SOLO_MAX_KB")) opt.solo_max_kb = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_CONV_LINES")) opt.conv_lines = std::atoi(e);
  if (const char* e = std::getenv("MI355_EMU_CONV_FUSED_MAX_POINTS")) opt.conv_fused_max_points = std::atoll(e);
  emu::g_xcds = std::getenv("MI355_EMU_XCDS") ? (unsigned)std::atoi(std::getenv("MI355_EMU_XCDS")) : 2u;
  PlanIR ir;
  std::string e;
  int rc = build_plan(*desc, opt, ir, e);
  // output and input of an out-of-place c2c plan in one allocation: what mi355fft_plan_exec does then (plan.hpp alias_variant), the two
  // pointers standing for the offsets
  if (!rc && input && output) {
    const AliasVariant v = alias_variant(ir, (uint64_t)(uintptr_t)input, (uint64_t)(uintptr_t)output, e);
    if (v == ALIAS_REFUSED) { std::snprintf(err, err_bytes, "%s", e.c_str()); return MI355FFT_ERR_INVALID; }
    if (v == ALIAS_STAGED) { opt.fuse_views = 0; rc = build_plan(*desc, opt, ir, e); }
  }
  if (rc) { std::snprintf(err, err_bytes, "%s", e.c_str()); return rc; }
  if (route) std::snprintf(route, route_bytes, "%s", ir.route.c_str());
  if (launches) *launches = (int)ir.steps.size();
  if (!input) return 0;   // route and launches only, under the emulator's own planner switches
  if (input_bytes < ir.in_bytes) { std::snprintf(err, err_bytes, "input too small: need %llu", (unsigned long long)ir.in_bytes); return 100; }
  if (!desc->in_place && output_bytes < ir.out_bytes) { std::snprintf(err, err_bytes, "output too small: need %llu", (unsigned long long)ir.out_bytes); return 101; }
  if (kernel_bytes < ir.kernel_bytes) { std::snprintf(err, err_bytes, "kernel too small: need %llu", (unsigned long long)ir.kernel_bytes); return 102; }
  std::vector<char> work(ir.work_bytes + 256, (char)work_fill);
  void* base[5] = {input, desc->in_place ? input : output, work.data(), kernel, ir.table.data()};
  EmuLauncher l;
  auto lines_fn = [&](int family, int id, const LineArgs& a, unsigned grid) -> bool {
    switch (family) {
      case FAM_ROW_SMALL: return launch_lines_family<FAM_ROW_SMALL>(id, a, grid, l);
      case FAM_ROW_1K: return launch_lines_family<FAM_ROW_1K>(id, a, grid, l);
      case FAM_ROW_BIG: return launch_lines_family<FAM_ROW_BIG>(id, a, grid, l);
      case FAM_PASS_A: return launch_lines_family<FAM_PASS_A>(id, a, grid, l);
      case FAM_PASS_B: return launch_lines_family<FAM_PASS_B>(id, a, grid, l);
    }
    return false;
  };
  for (const Step& s : ir.steps) {
    void* ptr[5];
    for (int i = 0; i < 5; ++i) ptr[i] = s.p[i].buf == BUF_NONE ? nullptr : (char*)base[s.p[i].buf] + s.p[i].off;
    auto xcd_fn = [&](int id, const XcdFusedArgs& a, unsigned grid) { return launch_xcd_fused(id, a, grid, l); };
    if (!dispatch_step(s, ptr, l, lines_fn, xcd_fn)) { std::snprintf(err, err_bytes, "no kernel for step kind %d variant %d", (int)s.kind, s.variant); return 103; }
  }
  if (tail_modified) {
    *tail_modified = 0;
    for (size_t i = ir.work_bytes; i < work.size(); ++i) if (work[i] != (char)work_fill) *tail_modified = 1;
  }
  if (l.sticky) { std::snprintf(err, err_bytes, "XCD-fused kernel gave up waiting (sticky=%u)", l.sticky); return 104; }
  return 0;
}

// the same on a zero-filled workspace (what the test_emu_* modules run)
int emu_run_plan(const mi355fft_plan_desc* desc, void* input, uint64_t input_bytes, void* output, uint64_t output_bytes, void* kernel,
                 uint64_t kernel_bytes, int force_generic, uint64_t chunk_bytes, char* err, size_t err_bytes, char* route, size_t route_bytes,
                 int* launches) {
  return emu_run_plan_ex(desc, input, input_bytes, output, output_bytes, kernel, kernel_bytes, force_generic, chunk_bytes, 0, nullptr, err, err_bytes,
                         route, route_bytes, launches);
}

// Planner only (host logic tests: routes, guards, workspace sizes) — nothing is run, so shapes far beyond host memory are fine.
int emu_plan_only(const mi355fft_plan_desc* desc, int compute_units, char* err, size_t err_bytes, char* route, size_t route_bytes, int* launches,
                  uint64_t* work_bytes) {
  using namespace mi355;
  PlannerOptions opt = planner_options_from_env();
  opt.compute_units = compute_units > 0 ? compute_units : 256;
  PlanIR ir;
  std::string e;
  const int rc = build_plan(*desc, opt, ir, e);
  if (rc) { std::snprintf(err, err_bytes, "%s", e.c_str()); return rc; }
  if (route) std::snprintf(route, route_bytes, "%s", ir.route.c_str());
  if (launches) *launches = (int)ir.steps.size();
  if (work_bytes) *work_bytes = ir.work_bytes;
  return 0;
}

// Planner only, the whole PlanIR as text: two plans are the same plan when their dumps are equal (tools/plan_snapshot.py compares
// the planner of two builds this way).  Returns the planner status; `out` receives the error text or the dump, cut at out_bytes;
// `needed` the bytes the full text takes (with its terminator).  Floats are printed as their bit patterns, the table as its length
// and the FNV-1a hash of its bytes.
int emu_plan_dump(const mi355fft_plan_desc* desc, int compute_units, char* out, size_t out_bytes, size_t* needed) {
  using namespace mi355;
  PlannerOptions opt = planner_options_from_env();
  opt.compute_units = compute_units > 0 ? compute_units : 256;
  PlanIR ir;
  std::string t;
  const int rc = build_plan(*desc, opt, ir, t);
  if (!rc) {
    const auto num = [&](const char* name, long long v) { t += name; t += std::to_string(v); };
    const auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return (long long)u; };
    const auto ints = [&](const char* name, const auto* v, int n) { t += name; for (int i = 0; i < n; ++i) { t += i ? "," : ""; t += std::to_string((long long)v[i]); } };
    const auto side = [&](const char* name, const SideMap& m) {
      t += name; num(" rank=", m.rank); num(" ax=", m.ax); ints(" dims=", m.dims, 8); ints(" lo=", m.lo, 8); ints(" hi=", m.hi, 8);
      ints(" zlo=", m.zlo, 8); ints(" zhi=", m.zhi, 8); ints(" stride=", m.stride, 8); num(" offset=", m.offset); num(" batch_stride=", m.batch_stride);
      t += "\n";
    };
    uint64_t h = 1469598103934665603ull;
    const unsigned char* tb = (const unsigned char*)ir.table.data();
    for (size_t i = 0; i < ir.table.size() * sizeof(float2h); ++i) h = (h ^ tb[i]) * 1099511628211ull;
    t = "route=" + ir.route + "\n";
    num("work_bytes=", (long long)ir.work_bytes); num(" in_bytes=", (long long)ir.in_bytes); num(" out_bytes=", (long long)ir.out_bytes);
    num(" kernel_bytes=", (long long)ir.kernel_bytes); num(" table_len=", (long long)ir.table.size());
    char hex[32];
    std::snprintf(hex, sizeof hex, " table_hash=%016llx\n", (unsigned long long)h);
    t += hex;
    num("steps=", (long long)ir.steps.size()); t += "\n";
    for (size_t n = 0; n < ir.steps.size(); ++n) {
      const Step& s = ir.steps[n];
      num("step ", (long long)n); num(" kind=", s.kind); num(" variant=", s.variant); num(" grid=", s.grid);
      t += " p=";
      for (int i = 0; i < 5; ++i) { t += i ? "," : ""; t += std::to_string(s.p[i].buf) + ":" + std::to_string((long long)s.p[i].off); }
      ints(" i=", s.i, 20); num(" f=", bits(s.f[0])); num(",", bits(s.f[1]));
      ints(" shape=", s.shape, 8); ints(" sa=", s.sa, 8); ints(" sb=", s.sb, 8);
      t += "\n";
      side("  imap", s.imap);
      side("  omap", s.omap);
    }
  }
  if (needed) *needed = t.size() + 1;
  if (out && out_bytes) std::snprintf(out, out_bytes, "%s", t.c_str());
  return rc;
}

// support kernels: PRNG twin + reductions
int emu_fill_random(float* out, uint64_t row_floats, uint64_t rows, uint32_t seed0, uint64_t first_transform) {
  EmuLauncher l;
  l.launch(mi355::fill_random_kernel, 2u, 256u, 0u, out, (unsigned long long)row_floats, (unsigned long long)rows, (unsigned)seed0,
           (unsigned long long)first_transform);
  return 0;
}
int emu_diff_sumsq(const float* a, const float* b, double alpha, uint64_t count, double* out) {
  EmuLauncher l;
  double partial[2] = {0, 0};
  l.launch(mi355::diff_sumsq_kernel, 2u, 256u, 0u, a, b, alpha, (unsigned long long)count, (double*)partial);
  *out = partial[0] + partial[1];
  return 0;
}

}  // extern "C"
