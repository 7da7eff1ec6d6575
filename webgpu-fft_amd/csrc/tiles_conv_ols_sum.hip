// device code + launch stubs of the rank-2 overlap-save tile kernel's sum form over input channels (kern_tiles.hpp fft_tiles_conv_ols_kernel on an STileCfg): one
// instance per entry of MI355_TILE_SUM_KERNEL_LIST (see dispatch.hpp launch_tiles_conv_ols_sum).  A unit of its own: kernels compiled together change each
// other's register allocation, and the other units' device code stays what it was
#define MI355_TILES_SUM_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
template bool launch_tiles_conv_ols_sum<HipLauncher>(int, const TilesSumArgs&, unsigned, HipLauncher&);
}
