// device code + launch stubs of the rank-2 overlap-save tile kernel's grouped forms on real tile pairs (fftConv.groups > 1; kern_tiles.hpp
// fft_tiles_conv_ols_group_kernel on a GRTileCfg / DRTileCfg): one instance per entry of MI355_TILE_GROUP_KERNEL_LIST (see dispatch.hpp
// launch_tiles_rconv_ols_group).  A unit of its own: kernels compiled together change each other's register allocation, and the other units' device code stays what it was
#define MI355_RTILES_GROUP_DEFINE_INSTANCES
#include "hip_launcher.hpp"
namespace mi355 {
template bool launch_tiles_rconv_ols_group<HipLauncher>(int, const TilesGroupArgs&, unsigned, HipLauncher&);
}
