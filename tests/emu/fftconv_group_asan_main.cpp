// Stand-alone program for the bounds of grouped and depthwise convolution (fftConv.groups) under AddressSanitizer + UBSan on the host: both forms of the grouped
// rank-2 tile kernel (kern_tiles.hpp fft_tiles_conv_ols_group_kernel: the sum form on a GTileCfg, complex tiles, and the depthwise form on a DRTileCfg, real
// tile pairs) and the grouped pointwise multiply-accumulate pass of the composed routes (kern_generic.hpp pointwise_group_sum_kernel).  The planner (plan.cpp)
// plans complex 150 x 100 (*) 9 x 5 linear-same convolution with C = 4, K = 4, G = 2 and real 150 x 130 (*) 9 x 5 linear-same correlation, depthwise C = K = G = 3
// (nb_1 = 3: the last pair of a row has no partner), batch 2, on the 64-point tile: 1 + 1 launches each.  The launches run here on the kernels' own source
// (MI355_HOST_EMU: one std::thread per GPU thread, a pthread barrier for __syncthreads()).  Input, kernel, output and workspace are heap blocks of exactly the
// plan's in_bytes, kernel_bytes, out_bytes and work_bytes, so a load from a line beyond batch * C, a spectrum read beyond K Cg P^2 or a store beyond the last
// output lane is a heap-buffer-overflow report.  Every output is compared with a direct sum over the group's channels in double precision.  The launcher also
// holds every tile launch to the threads and LDS bytes of the planner's registry (find_tile_kernel), and check_registry holds both grouped lists, entry by entry
// and in their length, to it.
// Built by fftconv_group_asan.mk and run by tests/test_emu_fftconv_group_asan.py:
//   ASAN_OPTIONS=detect_leaks=0 ./fftconv_group_asan      (exit status 0, a registry line, three rel_l2 lines and "ok", no sanitizer report)
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
  unsigned block = 0, smem = 0;     // of the last launch
  template <class... P, class... A>
  void launch(void (*kernel)(P...), unsigned grid, unsigned block_, unsigned smem_, A&&... args) {
    block = block_; smem = smem_;
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

uint64_t g_seed = 0x9E3779B97F4A7C15ull;
float rnd() {
  uint64_t& s = g_seed;
  s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
  return (float)((double)((s * 0x2545F4914F6CDD1Dull) >> 40) / (double)(1 << 24) - 0.5);
}

// the grouped tile route: `real` data depthwise as correlation, complex data with Cg = Kg = 2 as convolution
int run_tiles(bool real) {
  const int n0 = 150, n1 = real ? 130 : 100, m0 = 9, m1 = 5, batch = 2, C = real ? 3 : 4, K = C, G = real ? 3 : 2, Cg = C / G, Kg = K / G, P = 64, w = real ? 1 : 2;
  const bool corr = real;
  mi355fft_plan_desc d;
  std::memset(&d, 0, sizeof d);
  d.struct_size = (uint32_t)sizeof d;
  d.type = real ? MI355FFT_FFTCONV_REAL : MI355FFT_FFTCONV; d.rank = 2; d.shape[0] = n0; d.shape[1] = n1; d.batch = batch;
  d.conv_mode = corr ? MI355FFT_CORRELATION : MI355FFT_CONVOLUTION; d.conv_boundary = MI355FFT_LINEAR_SAME; d.conv_kernel_count = K; d.conv_output_layout = MI355FFT_KERNEL_MAJOR;
  d.conv_kernel_shape[0] = m0; d.conv_kernel_shape[1] = m1;
  d.input.reserved = C;
  d.zero_read.reserved = G;
  PlannerOptions opt;
  opt.compute_units = 2;        // few workgroups: each walks several work items
  opt.group_ols2d = P;
  PlanIR ir;
  std::string err;
  if (int rc = build_plan(d, opt, ir, err)) { std::fprintf(stderr, "build_plan failed (%d): %s\n", rc, err.c_str()); return 1; }
  const char* tag = real ? "tiles-rspectrum[N=64x64] tiles-rconv-ols-group[N=64x64,L=56x60,C=3,G=3,K=3]" : "tiles-spectrum[N=64x64] tiles-conv-ols-group[N=64x64,L=56x60,C=4,G=2,K=4]";
  if (ir.route.find(tag) == std::string::npos || (int)ir.steps.size() != 2) { std::fprintf(stderr, "route %s, %zu launches\n", ir.route.c_str(), ir.steps.size()); return 1; }
  const uint64_t esz = 4 * w;
  if (ir.in_bytes != esz * n0 * n1 * batch * C || ir.kernel_bytes != esz * m0 * m1 * K * Cg || ir.out_bytes != esz * n0 * n1 * batch * K || ir.work_bytes < (uint64_t)K * Cg * P * P * 8) {
    std::fprintf(stderr, "extents: in %llu kernel %llu out %llu work %llu\n", (unsigned long long)ir.in_bytes, (unsigned long long)ir.kernel_bytes, (unsigned long long)ir.out_bytes,
                 (unsigned long long)ir.work_bytes);
    return 1;
  }
  // heap blocks of exactly the plan's extents
  float* in = (float*)std::malloc(ir.in_bytes);
  float* out = (float*)std::malloc(ir.out_bytes);
  float* kern = (float*)std::malloc(ir.kernel_bytes);
  char* work = (char*)std::malloc(ir.work_bytes);
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
    const bool grouped = st.i[LS_TILES_KERNELS] != 0;
    bool launched = false;
    if (mode == LM_TILES_SPECTRUM && !grouped) launched = launch_tiles_conv_ols(st.variant, tiles_args_of(st, ptr), st.grid, l);
    else if (mode == LM_TILES_RSPECTRUM && !grouped) launched = launch_tiles_rconv_ols(st.variant, tiles_args_of(st, ptr), st.grid, l);
    else if (mode == LM_TILES_CONV_OLS && grouped) launched = launch_tiles_conv_ols_group(st.variant, tiles_group_args_of(st, ptr), st.grid, l);
    else if (mode == LM_TILES_RCONV_OLS && grouped) launched = launch_tiles_rconv_ols_group(st.variant, tiles_group_args_of(st, ptr), st.grid, l);
    if (!launched) { std::fprintf(stderr, "no instance for mode %d, variant %d\n", mode, st.variant); return 1; }
    if (grouped) {
      const TilesGroupArgs ga = tiles_group_args_of(st, ptr);
      if (ga.channels != Cg || ga.item_lines != C || ga.kernels != K || ga.kernels_per_group != Kg || ga.out_kernel_stride != (long long)batch * n0 * n1) {
        std::fprintf(stderr, "group slots: Cg %d C %d K %d Kg %d lane_k %lld\n", ga.channels, ga.item_lines, ga.kernels, ga.kernels_per_group, ga.out_kernel_stride);
        return 1;
      }
    }
    // the planner's registry entry of the instance against what the dispatch launched with
    const TileKernelMeta* tm = grouped ? find_tile_kernel(P, real, Cg > 1, Cg > 1 ? 1 : 2) : find_tile_kernel(P, real);
    if (!tm || tm->id != st.variant || (unsigned)tm->threads != l.block || (unsigned)tm->lds_bytes != l.smem) {
      std::fprintf(stderr, "tile registry (grouped %d): launched %u threads, %u B of LDS\n", (int)grouped, l.block, l.smem);
      return 1;
    }
  }
  // direct sums over the group's channels; linear-same: output o is index m = o + c of the logical domain, c = (M - 1) / 2.  Convolution y[m] = sum_r h[r] x[m - r];
  // correlation y = sum_r conj(h[r]) x[lag + r], the lag m below n and m - (n + M - 1) from there on
  const int c0 = (m0 - 1) / 2, c1 = (m1 - 1) / 2;
  const auto lag = [](int m, int n, int M) { return m < n ? m : m - (n + M - 1); };
  double num = 0, den = 0;
  for (int k = 0; k < K; ++k) for (int b = 0; b < batch; ++b) for (int o1 = 0; o1 < n1; ++o1) for (int o0 = 0; o0 < n0; ++o0) {
    double re = 0, im = 0;
    const int first = (k / Kg) * Cg;
    for (int c = 0; c < Cg; ++c)
      for (int r1 = 0; r1 < m1; ++r1) {
        const int p1 = corr ? lag(o1 + c1, n1, m1) + r1 : o1 + c1 - r1;
        if (p1 < 0 || p1 >= n1) continue;
        for (int r0 = 0; r0 < m0; ++r0) {
          const int p0 = corr ? lag(o0 + c0, n0, m0) + r0 : o0 + c0 - r0;
          if (p0 < 0 || p0 >= n0) continue;
          const size_t xa = (((size_t)(b * C + first + c) * n1 + p1) * n0 + p0) * w, ha = (((size_t)(k * Cg + c) * m1 + r1) * m0 + r0) * w;
          if (real) re += (double)kern[ha] * in[xa];
          else {
            const double xr = in[xa], xi = in[xa + 1], hr = kern[ha], hi = corr ? -kern[ha + 1] : kern[ha + 1];
            re += xr * hr - xi * hi; im += xr * hi + xi * hr;
          }
        }
      }
    const size_t at = ((((size_t)k * batch + b) * n1 + o1) * n0 + o0) * w;
    const double dr = out[at] - re, di = real ? 0.0 : out[at + 1] - im;
    num += dr * dr + di * di; den += re * re + im * im;
  }
  const double rel = std::sqrt(num / den);
  std::printf("%s %s: %d work items in the launch on %u workgroups, rel_l2 %.3e\n", corr ? "correlation" : "convolution", ir.route.c_str(), (int)ir.steps.back().i[LS_TILES], ir.steps.back().grid, rel);
  int bad = 0;
  if (!(rel <= 1e-5)) { std::fprintf(stderr, "differs from the direct sum: rel_l2 %.3e\n", rel); bad = 1; }
  std::free(in); std::free(out); std::free(kern); std::free(work);
  return bad;
}

// The two lists of grouped instances (MI355_TILE_GROUP_KERNEL_LIST on complex tiles and on real tile pairs) against the planner's registry: the list has two
// entries, id 0 the sum form and id 1 the depthwise form, both P = 64 on 256 threads; every id dispatches, with the registry's threads and LDS bytes, and the id
// behind the list's end does not; no 128-point grouped entry exists.  Nothing runs: the launcher only records the launch shape
struct Recorder {
  unsigned block = 0, smem = 0;
  template <class... P, class... A> void launch(void (*)(P...), unsigned, unsigned block_, unsigned smem_, A&&...) { block = block_; smem = smem_; }
};
int check_registry() {
  int entries = 0;
#define X(P, R0, R1, TH, DW) ++entries;
  MI355_TILE_GROUP_KERNEL_LIST(X)
#undef X
  if (entries != 2) { std::fprintf(stderr, "MI355_TILE_GROUP_KERNEL_LIST has %d entries\n", entries); return 1; }
  const TilesGroupArgs none{};
  for (int real = 0; real < 2; ++real) {
    for (int id = 0; id <= entries; ++id) {
      Recorder rec;
      const bool ok = real ? launch_tiles_rconv_ols_group(id, none, 1u, rec) : launch_tiles_conv_ols_group(id, none, 1u, rec);
      if (id == entries) {
        if (ok) { std::fprintf(stderr, "grouped list (real %d): id %d dispatches beyond the list\n", real, id); return 1; }
        continue;
      }
      const bool sum = id == 0;                        // id 0: Cg > 1, id 1: Cg = 1
      const TileKernelMeta* tm = find_tile_kernel(64, real != 0, sum, sum ? 1 : 2);
      if (!ok || !tm || tm->id != id || tm->threads != 256 || tm->lds_bytes != tile_kernel_lds_bytes(64, 8, 8) || rec.block != (unsigned)tm->threads || rec.smem != (unsigned)tm->lds_bytes) {
        std::fprintf(stderr, "grouped list (real %d) id %d: dispatched %d with %u threads, %u B of LDS\n", real, id, (int)ok, rec.block, rec.smem);
        return 1;
      }
      if (find_tile_kernel(128, real != 0, sum, sum ? 1 : 2) || find_tile_kernel(64, real != 0, !sum, sum ? 1 : 2)) {
        std::fprintf(stderr, "grouped list (real %d): an entry that should not exist\n", real);
        return 1;
      }
    }
    // the other lists keep their lengths: two single-channel entries (64, 128), one sum entry
    if (!find_tile_kernel(64, real != 0) || !find_tile_kernel(128, real != 0) || !find_tile_kernel(64, real != 0, true) || find_tile_kernel(128, real != 0, true)) {
      std::fprintf(stderr, "single-channel / sum lists (real %d) changed\n", real);
      return 1;
    }
  }
  std::printf("registry: %d grouped entries per data type, 256 threads, %d B of LDS\n", entries, tile_kernel_lds_bytes(64, 8, 8));
  return 0;
}

// pointwise_group_sum_kernel on exactly sized blocks: out[b][i] = sum_{c < Cg} data[b C + g Cg + c][i] conj(kern[c][i]) for the LAST group (its last line ends the
// data block), a grid smaller than the work
int run_pointwise() {
  const long long L = 1031, B = 3;
  const int C = 6, Cg = 2, g = 2;
  cf* data = (cf*)std::malloc(sizeof(cf) * B * C * L);
  cf* kern = (cf*)std::malloc(sizeof(cf) * Cg * L);
  cf* out = (cf*)std::malloc(sizeof(cf) * B * L);
  for (long long i = 0; i < B * C * L; ++i) data[i] = cf{rnd(), rnd()};
  for (long long i = 0; i < Cg * L; ++i) kern[i] = cf{rnd(), rnd()};
  Launcher l;
  l.launch(pointwise_group_sum_kernel, 2u, 256u, 0u, (const cf*)(data + g * Cg * L), out, (const cf*)kern, L, B * L, Cg, C, 1, 0.5f);
  double num = 0, den = 0;
  for (long long b = 0; b < B; ++b) for (long long i = 0; i < L; ++i) {
    double re = 0, im = 0;
    for (int c = 0; c < Cg; ++c) {
      const cf x = data[(b * C + g * Cg + c) * L + i], h = kern[c * L + i];
      re += (double)x.x * h.x + (double)x.y * h.y; im += (double)x.y * h.x - (double)x.x * h.y;
    }
    const double dr = out[b * L + i].x - 0.5 * re, di = out[b * L + i].y - 0.5 * im;
    num += dr * dr + di * di; den += 0.25 * (re * re + im * im);
  }
  const double rel = std::sqrt(num / den);
  std::printf("pointwise-group-sum %lld x %lld points, C = %d, Cg = %d, group %d: rel_l2 %.3e\n", B, L, C, Cg, g, rel);
  std::free(data); std::free(kern); std::free(out);
  if (!(rel <= 1e-6)) { std::fprintf(stderr, "pointwise-group-sum differs from the direct sum: rel_l2 %.3e\n", rel); return 1; }
  return 0;
}
}  // namespace

int main() {
  int bad = 0;
  bad |= check_registry();
  bad |= run_tiles(false);
  bad |= run_tiles(true);
  bad |= run_pointwise();
  if (!bad) std::printf("ok\n");
  return bad;
}
