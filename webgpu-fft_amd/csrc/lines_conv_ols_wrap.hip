// device code + launch stubs of the complex overlap-save line kernel's circular form (kern_lines.hpp fft_lines_conv_ols_kernel on OlsWrap<C>): block lengths 2048 and 4096
// (see dispatch.hpp launch_lines_conv_ols_wrap).  A unit of its own: kernels compiled together change each other's register allocation, and the other units'
// device code stays what it was
#define MI355_CONV_OLS_WRAP_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
template bool launch_lines_conv_ols_wrap<HipLauncher>(int, const RconvOlsArgs&, unsigned, HipLauncher&);
}
