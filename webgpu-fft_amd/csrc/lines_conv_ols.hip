// device code + launch stubs of the complex overlap-save line kernel (kern_lines.hpp fft_lines_conv_ols_kernel): one instance per forward
// ROW configuration of line_kernels.def with an LDS line buffer, P = 128 .. 4096 (see dispatch.hpp launch_lines_conv_ols).  A unit of its own:
// kernels compiled together change each other's register allocation, and the other units' device code stays what it was
#define MI355_CONV_OLS_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
template bool launch_lines_conv_ols<HipLauncher>(int, const RconvOlsArgs&, unsigned, HipLauncher&);
}
