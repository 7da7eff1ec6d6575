// Stand-alone program for the bounds of the rank-2 overlap-save tile kernel on real tile pairs (kern_tiles.hpp fft_tiles_conv_ols_kernel on an RTileCfg)
// under AddressSanitizer + UBSan on the host: the planner (plan.cpp) plans 150 x 130 (*) 9 x 5 linear-same on real data, batch 3, dense, and the same with
// batch 2, K = 2 and rank-2 strides, offsets and batch strides on both sides (odd, in f32 elements), each on the 64- and on the 128-point tile.  On the
// 64-point tile nb_1 = 3: the second pair row has no partner; on the 128-point tile nb_1 = 2.  The two launches of the route run here on the kernel's own
// source (MI355_HOST_EMU: one std::thread per GPU thread, a pthread barrier for __syncthreads()).  Input, kernel, output and workspace are heap blocks of
// exactly the plan's extents, so a load or store outside a tile's predicates (an absent partner's among them) is a heap-buffer-overflow report.  Every
// output is compared with a direct sum in double precision, and every output element outside the lanes must keep its sentinel.
// Only the tile kernel's instances are compiled (dispatch.hpp launch_tiles_rconv_ols).  Built with the flags of the Makefile's libmi355emu_asan.so rule
// without -shared:
//   clang++ $(CXXFLAGS) -fsanitize=address,undefined -fno-omit-frame-pointer -ftls-model=initial-exec tiles_rconv_ols_asan_main.cpp $(CSRC)/plan.cpp -o tiles_rconv_ols_asan
//   ASAN_OPTIONS=detect_leaks=0 ./tiles_rconv_ols_asan      (exit status 0, four rel_l2 lines and "ok", no sanitizer report)
// No test builds it; profiles/fftconv_rtiles_resource_usage.log has the run taken.
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

int run(int P, bool strided) {
  const int n0 = 150, n1 = 130, m0 = 9, m1 = 5, batch = strided ? 2 : 3, K = strided ? 2 : 1;
  const int64_t si[2] = {strided ? 3 : 1, strided ? 455 : n0}, so[2] = {strided ? 5 : 1, strided ? 761 : n0};
  const int64_t ioff = strided ? 5 : 0, ooff = strided ? 7 : 0, kst = strided ? 1 : (int64_t)batch * n0 * n1;
  const int64_t ibs = strided ? n1 * si[1] + 11 : (int64_t)n0 * n1, obs = strided ? n1 * so[1] + 7 : (int64_t)n0 * n1;
  mi355fft_plan_desc d;
  std::memset(&d, 0, sizeof d);
  d.struct_size = (uint32_t)sizeof d;
  d.type = MI355FFT_FFTCONV_REAL; d.rank = 2; d.shape[0] = n0; d.shape[1] = n1; d.batch = batch;
  d.conv_mode = MI355FFT_CONVOLUTION; d.conv_boundary = MI355FFT_LINEAR_SAME; d.conv_kernel_count = K; d.conv_output_layout = MI355FFT_KERNEL_MAJOR;
  d.conv_kernel_shape[0] = m0; d.conv_kernel_shape[1] = m1;
  if (strided) {
    d.input.strided = d.output.strided = 1;
    for (int a = 0; a < 2; ++a) { d.input.strides[a] = si[a]; d.output.strides[a] = so[a]; }
    d.input.offset_elements = ioff; d.output.offset_elements = ooff; d.input.batch_stride_elements = ibs; d.output.batch_stride_elements = obs;
    d.conv_output_kernel_stride_elements = kst;
  }
  PlannerOptions opt;
  opt.compute_units = 2;        // few workgroups: each walks several tiles
  opt.rconv_ols2d = P;
  PlanIR ir;
  std::string err;
  if (int rc = build_plan(d, opt, ir, err)) { std::fprintf(stderr, "build_plan failed (%d): %s\n", rc, err.c_str()); return 1; }
  char tag[96];
  std::snprintf(tag, sizeof tag, "tiles-rspectrum[N=%dx%d] tiles-rconv-ols[N=%dx%d,L=%dx%d]", P, P, P, P, P - m0 + 1, P - m1 + 1);
  if (ir.route.find(tag) == std::string::npos || (int)ir.steps.size() != 1 + K) { std::fprintf(stderr, "route %s, %zu launches\n", ir.route.c_str(), ir.steps.size()); return 1; }
  // heap blocks of exactly the plan's extents
  float* in = (float*)std::malloc(ir.in_bytes);
  float* out = (float*)std::malloc(ir.out_bytes);
  float* kern = (float*)std::malloc(ir.kernel_bytes);
  char* work = (char*)std::malloc(ir.work_bytes);
  uint64_t s = 0x9E3779B97F4A7C15ull + (uint64_t)P + (strided ? 1 : 0);
  const auto rnd = [&] { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return (float)((double)((s * 0x2545F4914F6CDD1Dull) >> 40) / (double)(1 << 24) - 0.5); };
  for (size_t i = 0; i < ir.in_bytes / 4; ++i) in[i] = rnd();
  for (size_t i = 0; i < ir.kernel_bytes / 4; ++i) kern[i] = rnd();
  for (size_t i = 0; i < ir.out_bytes / 4; ++i) out[i] = 777.0f;
  std::memset(work, 0xFF, ir.work_bytes);
  Launcher l;
  for (const Step& st : ir.steps) {
    if (st.kind != ST_LINES || (st.i[LS_MODE] != LM_TILES_RCONV_OLS && st.i[LS_MODE] != LM_TILES_RSPECTRUM)) { std::fprintf(stderr, "not a tile launch\n"); return 1; }
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
    if (!launch_tiles_rconv_ols(st.variant, tiles_args_of(st, ptr), st.grid, l)) { std::fprintf(stderr, "no instance %d\n", st.variant); return 1; }
  }
  // direct sums: y[o] = sum_r h[r] x[o + c - r], c = (M - 1) / 2
  std::vector<char> touched(ir.out_bytes / 4, 0);
  const int c0 = (m0 - 1) / 2, c1 = (m1 - 1) / 2;
  double num = 0, den = 0;
  int bad = 0;
  for (int k = 0; k < K; ++k) for (int b = 0; b < batch; ++b) for (int o1 = 0; o1 < n1; ++o1) for (int o0 = 0; o0 < n0; ++o0) {
    double want = 0;
    for (int r1 = 0; r1 < m1; ++r1) {
      const int p1 = o1 + c1 - r1;
      if (p1 < 0 || p1 >= n1) continue;
      for (int r0 = 0; r0 < m0; ++r0) {
        const int p0 = o0 + c0 - r0;
        if (p0 < 0 || p0 >= n0) continue;
        want += (double)kern[(k * m1 + r1) * m0 + r0] * (double)in[ioff + b * ibs + p1 * si[1] + p0 * si[0]];
      }
    }
    const int64_t at = ooff + k * kst + b * obs + o1 * so[1] + o0 * so[0];
    touched[(size_t)at] = 1;
    const double got = out[at];
    num += (got - want) * (got - want); den += want * want;
  }
  for (size_t i = 0; i < touched.size(); ++i)
    if (!touched[i] && out[i] != 777.0f) { if (!bad) std::fprintf(stderr, "store outside the lanes at element %zu\n", i); bad = 1; }
  const double rel = std::sqrt(num / den);
  std::printf("%s %s: %d work items a launch on %u workgroups, rel_l2 %.3e\n", strided ? "strided" : "dense", ir.route.c_str(), (int)ir.steps.back().i[LS_TILES], ir.steps.back().grid, rel);
  if (!(rel <= 1e-5)) { std::fprintf(stderr, "differs from the direct sum: rel_l2 %.3e\n", rel); bad = 1; }
  std::free(in); std::free(out); std::free(kern); std::free(work);
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  for (int P : {64, 128}) { bad |= run(P, false); bad |= run(P, true); }
  if (!bad) std::printf("ok\n");
  return bad;
}
