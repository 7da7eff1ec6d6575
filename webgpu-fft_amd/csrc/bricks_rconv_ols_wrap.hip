// device code + launch stubs of the rank-3 overlap-save brick kernel's circular form on real brick pairs (kern_bricks.hpp fft_bricks_conv_ols_kernel on a WRBrickCfg): one instance per entry of MI355_BRICK_KERNEL_LIST
// (see dispatch.hpp launch_bricks_rconv_ols_wrap).  A unit of its own: kernels compiled together change each other's register allocation, and the other units'
// device code stays what it was
#define MI355_RBRICKS_WRAP_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
template bool launch_bricks_rconv_ols_wrap<HipLauncher>(int, const BricksArgs&, unsigned, HipLauncher&);
}
