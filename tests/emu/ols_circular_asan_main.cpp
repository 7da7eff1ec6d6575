// Stand-alone program for the bounds of the circular (WRAP) forms of two overlap-save kernels under AddressSanitizer + UBSan on the host: the rank-2 tile
// kernel on real tile pairs (kern_tiles.hpp fft_tiles_conv_ols_kernel on a WRTileCfg) and the real line kernel (kern_lines.hpp fft_lines_rconv_ols_kernel on
// OlsWrap<C>).  The planner (plan.cpp) plans real 150 x 130 (*) 9 x 5 circular, batch 3 (64-point tiles, nb = 3 x 3: every edge tile wraps, the last pair of a
// row has no partner) and real 8193 (*) 31 circular, batch 2 (1024-point blocks on an odd line: sample pairs across the seam, the parity flip behind it), each
// as convolution and as correlation.  The launches run here on the kernels' own source (MI355_HOST_EMU: one std::thread per GPU thread, a pthread barrier
// for __syncthreads()).  Input, kernel, output and workspace are heap blocks of exactly the plan's extents, so a wrapped index that leaves [0, shape), or an
// absent partner's load, is a heap-buffer-overflow report.  Every output is compared with a direct circular sum in double precision.
// Only these kernels' instances are compiled: the tile route's spectrum launch is the tile kernel's linear instance (dispatch.hpp launch_tiles_rconv_ols);
// the line route's spectrum launch (lines-r2c-mapped, not under test here) is replaced by the same packed spectra computed on the host.
// Built by ols_circular_asan.mk and run by tests/test_emu_fftconv_circular_asan.py:
//   ASAN_OPTIONS=detect_leaks=0 ./ols_circular_asan      (exit status 0, four rel_l2 lines and "ok", no sanitizer report)
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "dispatch.hpp"

namespace emu {
thread_local dim3_t t_threadIdx, t_blockIdx, t_blockDim, t_gridDim;
thread_local char* t_smem = nullptr;
unsigned g_xcds = 1;
static thread_local pthread_barrier_t* t_barrier = nullptr;
void sync_threads() { pthread_barrier_wait(t_barrier); }
void sync_wave() { pthread_barrier_wait(t_barrier); }
}  // namespace emu

namespace {
using namespace mi355;

// blocks one after the other, `block` host threads each, LDS of exactly `smem` bytes on the heap
struct Launcher {
  template <class... P, class... A>
  void launch(void (*kernel)(P...), unsigned grid, unsigned block, unsigned smem, A&&... args) {
    pthread_barrier_t bar;
    pthread_barrier_init(&bar, nullptr, block);
    for (unsigned b = 0; b < grid; ++b) {
      char* lds = (char*)std::malloc(smem ? smem : 1);
      std::vector<std::thread> th;
      for (unsigned t = 0; t < block; ++t)
        th.emplace_back([&, t] {
          emu::t_threadIdx.x = t; emu::t_blockIdx.x = b; emu::t_blockDim.x = block; emu::t_gridDim.x = grid;
          emu::t_smem = lds; emu::t_barrier = &bar;
          kernel(args...);
        });
      for (auto& x : th) x.join();
      std::free(lds);
    }
    pthread_barrier_destroy(&bar);
  }
};

int run(int rank, bool corr) {
  const int n0 = rank == 2 ? 150 : 8193, n1 = rank == 2 ? 130 : 1, m0 = rank == 2 ? 9 : 31, m1 = rank == 2 ? 5 : 1, batch = rank == 2 ? 3 : 2, K = 1;
  const int P = rank == 2 ? 64 : 1024;
  mi355fft_plan_desc d;
  std::memset(&d, 0, sizeof d);
  d.struct_size = (uint32_t)sizeof d;
  d.type = MI355FFT_FFTCONV_REAL; d.rank = rank; d.shape[0] = n0; d.shape[1] = n1; d.batch = batch;
  d.conv_mode = corr ? MI355FFT_CORRELATION : MI355FFT_CONVOLUTION; d.conv_boundary = MI355FFT_CIRCULAR; d.conv_kernel_count = K; d.conv_output_layout = MI355FFT_KERNEL_MAJOR;
  d.conv_kernel_shape[0] = m0; d.conv_kernel_shape[1] = m1;
  PlannerOptions opt;
  opt.compute_units = 2;        // few workgroups: each walks several work items
  opt.ols_circular = 1;
  PlanIR ir;
  std::string err;
  if (int rc = build_plan(d, opt, ir, err)) { std::fprintf(stderr, "build_plan failed (%d): %s\n", rc, err.c_str()); return 1; }
  const char* tag = rank == 2 ? "tiles-rspectrum[N=64x64] tiles-rconv-ols[N=64x64,L=56x60,wrap]" : "lines-r2c-mapped[N=1024] lines-rconv-ols[N=1024,L=994,wrap]";
  if (ir.route.find(tag) == std::string::npos || (int)ir.steps.size() != 1 + K) { std::fprintf(stderr, "route %s, %zu launches\n", ir.route.c_str(), ir.steps.size()); return 1; }
  // heap blocks of exactly the plan's extents
  float* in = (float*)std::malloc(ir.in_bytes);
  float* out = (float*)std::malloc(ir.out_bytes);
  float* kern = (float*)std::malloc(ir.kernel_bytes);
  char* work = (char*)std::malloc(ir.work_bytes);
  if (ir.in_bytes != (uint64_t)4 * n0 * n1 * batch || ir.out_bytes != (uint64_t)4 * n0 * n1 * batch * K) { std::fprintf(stderr, "extents\n"); return 1; }
  uint64_t s = 0x9E3779B97F4A7C15ull + (uint64_t)rank + (corr ? 16 : 0);
  const auto rnd = [&] { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (float)((double)((s * 0x2545F4914F6CDD1Dull) >> 40) / (double)(1 << 24) - 0.5); };
  for (size_t i = 0; i < ir.in_bytes / 4; ++i) in[i] = rnd();
  for (size_t i = 0; i < ir.kernel_bytes / 4; ++i) kern[i] = rnd();
  for (size_t i = 0; i < ir.out_bytes / 4; ++i) out[i] = 777.0f;
  std::memset(work, 0xFF, ir.work_bytes);
  Launcher l;
  for (const Step& st : ir.steps) {
    if (st.kind != ST_LINES) { std::fprintf(stderr, "not a line-mode launch\n"); return 1; }
    void* ptr[STEP_PTRS];
    for (int i = 0; i < STEP_PTRS; ++i) {
      char* base = nullptr;
      switch (st.p[i].buf) {
        case BUF_INPUT: base = (char*)in; break;
        case BUF_OUTPUT: base = (char*)out; break;
        case BUF_WORK: base = work; break;
        case BUF_KERNEL: base = (char*)kern; break;
        case BUF_TABLE: base = (char*)ir.table.data(); break;
        default: break;
      }
      ptr[i] = base ? base + st.p[i].off : nullptr;
    }
    const int mode = (int)st.i[LS_MODE];
    bool launched = false;
    if (mode == LM_TILES_RSPECTRUM && !st.i[LS_OLS_WRAP]) launched = launch_tiles_rconv_ols(st.variant, tiles_args_of(st, ptr), st.grid, l);
    else if (mode == LM_TILES_RCONV_OLS && st.i[LS_OLS_WRAP]) launched = launch_tiles_rconv_ols_wrap(st.variant, tiles_args_of(st, ptr), st.grid, l);
    else if (mode == LM_R2C && st.i[LS_MAPPED]) {
      // the K packed kernel spectra the line kernel multiplies in: bins 0 .. P / 2 of the kernel zero-padded to P points
      cf* G = (cf*)ptr[LP_OUT];
      for (int k = 0; k < K; ++k)
        for (int b = 0; b <= P / 2; ++b) {
          double re = 0, im = 0;
          for (int r = 0; r < m0; ++r) { const double ph = -2.0 * M_PI * (double)((long long)b * r % P) / P; re += kern[k * m0 + r] * std::cos(ph); im += kern[k * m0 + r] * std::sin(ph); }
          G[k * (P / 2 + 1) + b] = cf{(float)re, (float)im};
        }
      launched = true;
    } else if (mode == LM_RCONV_OLS && st.i[LS_OLS_WRAP]) {
      // the argument block as dispatch.hpp dispatch_step fills it for this mode
      RconvOlsArgs oa{};
      LineArgs& a = oa.a;
      a.in = (const cf*)ptr[LP_IN]; a.out = (cf*)ptr[LP_OUT]; a.tw = (const cf*)ptr[LP_TW]; a.tw_lo = (const cf*)ptr[LP_TW_LO]; a.tw_hi = (const cf*)ptr[LP_TW_HI];
      a.num_tiles = st.i[LS_TILES]; a.num_lines = st.i[LS_LINES];
      a.in_S = st.i[LS_IN_S]; a.in_outer_stride = st.i[LS_IN_OUTER]; a.out_S = st.i[LS_OUT_S]; a.out_outer_stride = st.i[LS_OUT_OUTER];
      a.fs_shift = (int)st.i[LS_FS_SHIFT]; a.fs_lo_mask = (unsigned)st.i[LS_FS_LO_MASK]; a.fs_group = 1; a.real_mode = mode;
      a.mapped = 1; a.imap = st.imap; a.omap = st.omap; a.scale = st.f[F_SCALE]; a.conj = (int)st.i[LS_CONJ];
      const OlsAxis g = ols_axis_of(st.i, 0);
      oa.o.fN = (int)g.fN; oa.o.plim = (int)g.plim; oa.o.nb = (int)g.nb; oa.o.L = (int)g.L; oa.o.w0 = (int)g.w0; oa.o.pre = (int)g.pre;
      launched = launch_lines_rconv_ols_wrap(st.variant, oa, st.grid, l);
    }
    if (!launched) { std::fprintf(stderr, "no instance for mode %d, variant %d\n", mode, st.variant); return 1; }
  }
  // direct circular sums: convolution y[o] = sum_r h[r] x[(o - r) mod n], correlation y[o] = sum_r h[r] x[(o + r) mod n]
  double num = 0, den = 0;
  int bad = 0;
  for (int k = 0; k < K; ++k) for (int b = 0; b < batch; ++b) for (int o1 = 0; o1 < n1; ++o1) for (int o0 = 0; o0 < n0; ++o0) {
    double want = 0;
    for (int r1 = 0; r1 < m1; ++r1) {
      const int p1 = ((corr ? o1 + r1 : o1 - r1) % n1 + n1) % n1;
      for (int r0 = 0; r0 < m0; ++r0) {
        const int p0 = ((corr ? o0 + r0 : o0 - r0) % n0 + n0) % n0;
        want += (double)kern[(k * m1 + r1) * m0 + r0] * (double)in[((size_t)b * n1 + p1) * n0 + p0];
      }
    }
    const double got = out[(((size_t)k * batch + b) * n1 + o1) * n0 + o0];
    num += (got - want) * (got - want); den += want * want;
  }
  const double rel = std::sqrt(num / den);
  std::printf("%s %s: %d work items a launch on %u workgroups, rel_l2 %.3e\n", corr ? "correlation" : "convolution", ir.route.c_str(), (int)ir.steps.back().i[LS_TILES], ir.steps.back().grid, rel);
  if (!(rel <= 1e-5)) { std::fprintf(stderr, "differs from the direct sum: rel_l2 %.3e\n", rel); bad = 1; }
  std::free(in); std::free(out); std::free(kern); std::free(work);
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (int rank : {2, 1}) { bad |= run(rank, false); bad |= run(rank, true); }
  if (!bad) std::printf("ok\n");
  return bad;
}
