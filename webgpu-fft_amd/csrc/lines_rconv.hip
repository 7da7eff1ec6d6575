// device code + launch stubs of the real fftconv line kernel (kern_lines.hpp fft_lines_rconv_kernel): one instance per forward ROW
// configuration of line_kernels.def with an LDS line buffer (see dispatch.hpp launch_lines_rconv), and of its overlap-save form
// (fft_lines_rconv_ols_kernel, dispatch.hpp launch_lines_rconv_ols): half lengths 64 .. 4096
#define MI355_RCONV_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
#define LINE_ROW(N, R0, R1, R2, T) \
  template bool launch_lines_rconv<LineCfg<N, R0, R1, R2, T, false, false, false, false, 0>, HipLauncher>(const LineArgs&, unsigned, HipLauncher&);
#define LINE_ROW_TRIG(N, R0, R1, R2, T)
#define LINE_PASS_A(N, R0, R1, R2, T)
#define LINE_PASS_B(N, R0, R1, R2, T)
#define LINE_COL_RAGGED(N, R0, R1, R2, T)
#include "line_kernels.def"
#undef LINE_ROW
#undef LINE_ROW_TRIG
#undef LINE_PASS_A
#undef LINE_PASS_B
#undef LINE_COL_RAGGED
template bool launch_lines_rconv_ols<HipLauncher>(int, const RconvOlsArgs&, unsigned, HipLauncher&);
}
