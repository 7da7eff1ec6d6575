// device code + launch stubs of the rank-3 overlap-save brick kernel on real brick pairs (kern_bricks.hpp fft_bricks_conv_ols_kernel on an RBrickCfg): one
// instance per entry of MI355_BRICK_KERNEL_LIST (see dispatch.hpp launch_bricks_rconv_ols).  A unit of its own, as bricks_conv_ols.hip is
#define MI355_RBRICKS_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
template bool launch_bricks_rconv_ols<HipLauncher>(int, const BricksArgs&, unsigned, HipLauncher&);
}
