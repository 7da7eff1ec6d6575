// device code + launch stubs of the real overlap-save line kernel's circular form (kern_lines.hpp fft_lines_rconv_ols_kernel on OlsWrap<C>): block lengths
// 1024, 2048 and 8192 (see dispatch.hpp launch_lines_rconv_ols_wrap).  A unit of its own: kernels compiled together change each other's register allocation,
// and the other units' device code stays what it was
#define MI355_RCONV_OLS_WRAP_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
template bool launch_lines_rconv_ols_wrap<HipLauncher>(int, const RconvOlsArgs&, unsigned, HipLauncher&);
}
