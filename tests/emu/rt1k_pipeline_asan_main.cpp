// Stand-alone program for the out-of-bounds guard of fft_xcd_rt1k_kernel's boundary prefetch (kern_regtile.hpp, MI355_RT1K_PREFETCH_X).  In its
// last phase-B tile of a transform a workgroup requests the head of the group's NEXT line — which exists only if tr + groups < num_transforms.
// Input and output are heap blocks of exactly batch * N * 8 bytes, so a request behind the last line is a heap-buffer-overflow report; batch 1
// has no next line at all, batch 3 on one group of 3 workgroups has one after the first and second transform and none after the third.  One
// line of each run is compared with a plain radix-2 FFT in double precision.
// Built with emu.cpp and plan.cpp under AddressSanitizer + UBSan (the flags of the Makefile's libmi355emu_asan.so rule without -shared):
//   clang++ $(CXXFLAGS) -DMI355_RT1K_PREFETCH=32 -DMI355_RT1K_PREFETCH_X=32 -fsanitize=address,undefined -fno-omit-frame-pointer -ftls-model=initial-exec \
//       rt1k_pipeline_asan_main.cpp emu.cpp $(CSRC)/plan.cpp -o rt1k_pipeline_asan
// (the two -D flags build the guarded request in: the boundary prefetch is off by default, and without them this is a plain correctness check of batches 1 and 3)
//   ASAN_OPTIONS=detect_leaks=0 ./rt1k_pipeline_asan      (exit status 0, two rel_l2 lines and "ok", no sanitizer report)
// No test builds it: instrumenting emu.cpp (every kernel of the project, both sanitizers) is one compiler job of 45 minutes; the run itself takes
// 4 s (profiles/rt1k_pipeline_ab.log has the one taken with all three depths at 32).  Linked against the plain libmi355emu.so instead, the
// program checks the same lines without the sanitizers.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mi355fft.h"

extern "C" int emu_run_plan(const mi355fft_plan_desc* desc, void* input, uint64_t input_bytes, void* output, uint64_t output_bytes, void* kernel,
                            uint64_t kernel_bytes, int force_generic, uint64_t chunk_bytes, char* err, size_t err_bytes, char* route, size_t route_bytes,
                            int* launches);

namespace {
constexpr int LOG2N = 20;
constexpr size_t N = (size_t)1 << LOG2N;

// in-place iterative radix-2, e^{-2 pi i jk/N}
void fft_ref(std::vector<std::complex<double>>& a) {
  for (size_t i = 1, j = 0; i < N; ++i) {
    size_t bit = N >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  const double pi = std::acos(-1.0);
  for (size_t len = 2; len <= N; len <<= 1) {
    std::vector<std::complex<double>> w(len / 2);
    for (size_t m = 0; m < len / 2; ++m) w[m] = std::polar(1.0, -2.0 * pi * (double)m / (double)len);
    for (size_t i = 0; i < N; i += len)
      for (size_t m = 0; m < len / 2; ++m) {
        const std::complex<double> u = a[i + m], v = a[i + m + len / 2] * w[m];
        a[i + m] = u + v;
        a[i + m + len / 2] = u - v;
      }
  }
}

int run(int batch, int check_line) {
  const size_t floats = 2 * N * (size_t)batch, bytes = floats * sizeof(float);   // exactly batch * N * 8 bytes each
  float* in = (float*)std::malloc(bytes);
  float* out = (float*)std::malloc(bytes);
  if (!in || !out) { std::fprintf(stderr, "out of memory\n"); return 2; }
  uint64_t s = 0x9E3779B97F4A7C15ull + (uint64_t)batch;
  for (size_t i = 0; i < floats; ++i) {   // xorshift64*, uniform in (-0.5, 0.5)
    s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
    in[i] = (float)((double)((s * 0x2545F4914F6CDD1Dull) >> 40) / (double)(1 << 24) - 0.5);
  }
  std::memset(out, 0, bytes);
  mi355fft_plan_desc d;
  std::memset(&d, 0, sizeof d);
  d.struct_size = (uint32_t)sizeof d;
  d.type = MI355FFT_C2C; d.rank = 1; d.direction = MI355FFT_FORWARD; d.normalize = MI355FFT_NORM_NONE;
  d.shape[0] = (int64_t)N; d.batch = batch; d.conv_kernel_count = 1;
  char err[512] = "", route[256] = "";
  int launches = 0;
  const int rc = emu_run_plan(&d, in, bytes, out, bytes, nullptr, 0, 0, 0, err, sizeof err, route, sizeof route, &launches);
  int bad = 0;
  if (rc) { std::fprintf(stderr, "batch %d: emu_run_plan failed (%d): %s\n", batch, rc, err); bad = 1; }
  if (!bad && (std::strncmp(route, "xcd-fused-rt32[N=1024x1024]", 27) != 0 || launches != 2)) {
    std::fprintf(stderr, "batch %d: route %s, %d launches: not the headline kernel\n", batch, route, launches); bad = 1;
  }
  if (!bad) {
    std::vector<std::complex<double>> a(N);
    const float* x = in + 2 * N * (size_t)check_line;
    for (size_t i = 0; i < N; ++i) a[i] = {x[2 * i], x[2 * i + 1]};
    fft_ref(a);
    const float* y = out + 2 * N * (size_t)check_line;
    double num = 0, den = 0;
    for (size_t i = 0; i < N; ++i) {
      const std::complex<double> g(y[2 * i], y[2 * i + 1]);
      num += std::norm(g - a[i]); den += std::norm(a[i]);
    }
    const double rel = std::sqrt(num / den);
    std::printf("batch %d line %d route %s rel_l2 %.3e\n", batch, check_line, route, rel);
    if (!(rel <= 1e-4)) { std::fprintf(stderr, "batch %d line %d differs from the reference FFT: rel_l2 %.3e\n", batch, check_line, rel); bad = 1; }   // (loose: f32 at 2^20 sits near 3e-7)
  }
  std::free(in);
  std::free(out);
  return bad;
}
}  // namespace

int main() {
  // one XCD, one group of 3 workgroups on the 32-line tiles, one slot: the shipped headline configuration in small
  setenv("MI355_EMU_XCD_FUSED", "1", 1); setenv("MI355_EMU_XCD_HX", "2", 1); setenv("MI355_EMU_CUS", "3", 1); setenv("MI355_EMU_XCDS", "1", 1);
  setenv("MI355_EMU_XCD_SPLIT", "1", 1); setenv("MI355_EMU_XCD_SLOTS", "1", 1);
  int bad = run(1, 0);
  bad |= run(3, 2);
  if (!bad) std::printf("ok\n");
  return bad;
}
