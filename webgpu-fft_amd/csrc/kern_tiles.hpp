// kern_tiles.hpp — overlap-save on rank-2 complex tiles (type MI355FFT_FFTCONV, route tiles-conv-ols): forward 2-D FFT, product with one kernel
// spectrum and inverse 2-D FFT of a P x P tile without leaving LDS.  The 2-D form of kern_lines.hpp fft_lines_conv_ols_kernel: its block
// geometry once per axis a (axis 0 fastest, as everywhere in the planner):
//   M_a = kernelShape[a], pre_a = M_a - 1, L_a = P - pre_a, fN_a = shape[a] + M_a - 1, nb_a = ceil(fN_a / L_a)
//   tile (j0, j1) of image b holds signal indices [s0_a, s0_a + P), s0_a = j_a L_a - pre_a, and gives the L0 x L1 results of its window
//   [w0_a, w0_a + L_a): w0_a = pre_a (convolution) or 0 (correlation); q_a = s0_a + i_a < plim_a (shape[a] when correlating, else fN_a);
//   logical index m_a = q_a < 0 ? q_a + fN_a : q_a (the negative lags of a correlation sit at the top of each axis of the domain)
//
// One workgroup owns a tile.  A pass transforms the P lines of one axis with the two Stockham stages of kern_lines.hpp (butterflies: radix.hpp);
// in BOTH passes lane -> line (line = t % P, butterfly u = t / P), so that a wave's 64 lanes sit on 64 neighbouring lines:
//   column pass (axis 1, the line is column i0 = line): element idx of the line at lds[idx * PITCH + line] — consecutive lanes, consecutive
//                addresses: conflict-free whatever the stage's index pattern, and in global memory runs of 64 elements along axis 0
//   row pass    (axis 0, the line is row i1 = line):    lds[line * PITCH + idx] — lanes PITCH apart.  PITCH = P + 1 is odd, so the 32 lanes a
//                ds_read_b64 / ds_write_b64 serves at once fall on 32 different bank pairs: conflict-free as well
// Forward runs columns then rows, the inverse rows then columns: the tile's first stage loads straight from global memory and its last stage
// stores straight to it, both contiguous along axis 0, and no load or store sweep over LDS exists.
//   load    : 8-byte loads through imap; on both axes its bounds are moved by the tile's origin ([lo_a - s0_a, hi_a - s0_a) cut to [0, P)), zero
//             elsewhere: the embed and zeroPad.read are the map's predicates, strided lanes its strides.  Nothing outside [lo, hi) is dereferenced
//   product : a lane reads the bins its first inverse stage starts from, multiplies them by the spectrum (conjugated when correlating) and swaps
//             re and im, so that the inverse re-uses the forward stages: no product pass over LDS.  The spectrum is read per tile (cache hits), not
//             kept in registers (profiles/fftconv_cols_ab.log: that cost a workgroup per CU in 1-D).  Its order is the tile's own: bin (k0, k1) at
//             [k0 * P + k1], which the row pass reads with consecutive lanes; LM_TILES_SPECTRUM is this kernel's forward half storing that order
//   store   : positions inside both windows, then the crop [lo_a, hi_a) of omap, zeroPad.write (zlo, zhi) and the output lane; scale 1/P^2
// Element indices are 32-bit (the planner keeps every fN_a and the number of tiles below 2^31 - 16384); buffer offsets are formed in 64 bits
//
// Real data (type MI355FFT_FFTCONV_REAL, route tiles-rconv-ols, the kernel on an RTileCfg): two real tiles a and b ride one complex tile as z = a + i b.
// The kernel h is real, so IFFT(FFT(z) H) = (a (*) h) + i (b (*) h), and with conj(H) the two correlations: the real parts are tile a's results and the
// imaginary parts tile b's; no Hermitian split, no packed bins, no separation pass.  Everything between the first load and the last store is the complex
// kernel's.  The partners are neighbours on axis 1: work item (sb, j0, jp) holds tile (j0, 2 jp) in .x and tile (j0, 2 jp + 1) in .y.  They share s0_0, the
// lane's column, its axis-0 predicates and both base pointers and differ in s0_1 alone, s0_1(b) = s0_1(a) + L_1, which is the same for every lane (SGPRs).
// pairs_1 = ceil(nb_1 / 2); with odd nb_1 the last pair's partner does not exist and needs no special case: s0_1(b) >= shape[1], so every load of its
// fails the map's hi bound, and s0_1(b) + w0_1 >= plim_1, so its window is empty.  Sides are 4-byte elements: every access is naturally aligned whatever s0_0.
// The kernel spectra come from the same kernel (LM_TILES_RSPECTRUM): one kernel per work item in .x; nb_1 = 1 and L_1 = P put partner b at s0_1 = P, beyond the
// kernel map's hi: zero imaginary parts, and the full complex P x P spectrum in the order above
#pragma once
#include <type_traits>
#include "platform.hpp"
#include "radix.hpp"
#include "plan.hpp"

// a value the optimizer must take as new at this point: comparisons of a lane's positions with it stay inside the tile loop instead of being hoisted
// out of it as one 64-bit lane mask per position (32 such masks: 64 SGPRs, spilt)
#ifdef MI355_HOST_EMU
#define MI_TILE_OPAQUE(x) do { } while (0)
#define MI_TILE_OPAQUE_LANE(x) do { } while (0)
#else
#define MI_TILE_OPAQUE(x) asm volatile("" : "+s"(x))
#define MI_TILE_OPAQUE_LANE(x) asm volatile("" : "+v"(x))     // the same for a lane's value: its 16 positions u + d are formed where they are used, not held in 16 VGPRs
#endif

namespace mi355 {

struct TileAxis { int fN, plim, nb, L, w0, pre; };   // RconvOls (kern_lines.hpp) of one axis
struct TilesArgs {
  const cf* in;         // the real form (RTileCfg) reads `in` and writes `out` as float arrays: the maps count 4-byte elements
  cf* out;
  const cf* tw;         // stage-1 roots [R1 - 1][R0] of order P (the table of a line kernel of P = R0 R1 points)
  const cf* spectrum;   // the kernel spectrum on P x P, bin (k0, k1) at [k0 * P + k1]
  long long num_tiles;  // work items: tiles, or tile pairs in the real form (ax[1].nb stays the number of tiles)
  float scale;
  int conj;             // correlation: the spectrum's conjugate
  int spectrum_only;    // LM_TILES_SPECTRUM: forward half only; tile k is kernel k, its spectrum stored dense at out + k P^2
  TileAxis ax[2];
  SideMap imap, omap;
};

template <int P_, int R0_, int R1_, int THREADS_>
struct TileCfg {
  static constexpr int P = P_, R0 = R0_, R1 = R1_, THREADS = THREADS_;
  static constexpr bool REAL = false;               // RTileCfg: real tile pairs
  static constexpr bool WRAP = false;               // WTileCfg, WRTileCfg: circular boundary, signal indices modulo fN_a
  static_assert(R0 * R1 == P, "radix product");
  static_assert(THREADS % P == 0 && THREADS <= 1024, "a thread stays on one line");
  static constexpr int TPL = THREADS / P;           // threads per line
  static constexpr int E = P / TPL;                 // complex values per thread
  static_assert(E % R0 == 0 && E % R1 == 0, "whole butterflies per thread");
  static constexpr int PITCH = P + 1;
  static constexpr int DATA_ELEMS = P * PITCH, TW_ELEMS = (R1 - 1) * R0;
  static constexpr int LDS_BYTES = tile_kernel_lds_bytes(P, R0, R1);
  static_assert(LDS_BYTES == (DATA_ELEMS + TW_ELEMS) * 8 && LDS_BYTES <= 160 * 1024, "tile does not fit LDS");
  // waves per SIMD when a CU holds the workgroups its 160 KB of LDS take (four of P = 64, one of P = 128: 16 waves, 4 a SIMD): the register budget
  // P = 128: the 16 positions u + d of a lane's loads and of its stores are formed again in every tile (MI_TILE_OPAQUE_LANE) instead of living in VGPRs across
  // the kernel: 124 VGPRs and no scratch where holding them spilt 8; P = 64 fits its 128 VGPRs holding them and spilt 4 without
  static constexpr bool REFORM_POSITIONS = P >= 128;
  static constexpr int WAVES_PER_SIMD = ((160 * 1024) / LDS_BYTES) * (THREADS / 64) / 4;
};

template <class C, int S> struct TileStage {
  static constexpr int R = S == 0 ? C::R0 : C::R1;
  static constexpr int NSP = S == 0 ? 1 : C::R0;
  static constexpr int NB = C::E / R;               // butterflies per thread
};

template <class C, bool COLS> MI_DEV int tile_index(int line, int idx) { return COLS ? idx * C::PITCH + line : line * C::PITCH + idx; }

// the inputs of stage S of this thread's butterflies, from LDS
template <class C, int S, bool COLS> MI_DEV void tile_stage_read(cf (&v)[C::E], const cf* lds, int line, int u) {
  using I = TileStage<C, S>;
#pragma unroll
  for (int b = 0; b < I::NB; ++b)
#pragma unroll
    for (int q = 0; q < I::R; ++q) v[b * I::R + q] = lds[tile_index<C, COLS>(line, u + b * C::TPL + q * (C::P / I::R))];
}
// roots and butterflies of stage S in registers: v[b R + q] becomes output q of butterfly b
template <class C, int S> MI_DEV void tile_stage_compute(cf (&v)[C::E], const cf* tw_lds, int u) {
  using I = TileStage<C, S>;
#pragma unroll
  for (int b = 0; b < I::NB; ++b) {
    cf w[I::R];
#pragma unroll
    for (int q = 0; q < I::R; ++q) w[q] = v[b * I::R + q];
    if constexpr (S > 0) {
      const int k = (u + b * C::TPL) % I::NSP;
#pragma unroll
      for (int q = 1; q < I::R; ++q) w[q] = cmul(w[q], tw_lds[(q - 1) * I::NSP + k]);
    }
    fft_radix<I::R>(w);
#pragma unroll
    for (int q = 0; q < I::R; ++q) v[b * I::R + q] = w[q];
  }
}
// the index along the line of output q of butterfly b (Stockham autosort: natural order behind the last stage)
template <class C, int S> MI_DEV int tile_stage_out(int u, int b, int q) {
  using I = TileStage<C, S>;
  const int j = u + b * C::TPL;
  return (j / I::NSP) * (I::NSP * I::R) + j % I::NSP + q * I::NSP;
}
template <class C, int S, bool COLS> MI_DEV void tile_stage_write(const cf (&v)[C::E], cf* lds, int line, int u) {
  using I = TileStage<C, S>;
#pragma unroll
  for (int b = 0; b < I::NB; ++b)
#pragma unroll
    for (int q = 0; q < I::R; ++q) lds[tile_index<C, COLS>(line, tile_stage_out<C, S>(u, b, q))] = v[b * I::R + q];
}

// C::REAL: two real tiles, neighbours on axis 1, as re / im of the complex tile (see the header); the form differs at the loads, at the stores and where a
// work item's tile is found.  It is a property of the configuration, not a second template parameter: the complex instances keep their names and their code
template <class C>
__global__ void __launch_bounds__(C::THREADS, C::WAVES_PER_SIMD) fft_tiles_conv_ols_kernel(const TilesArgs a) {
  constexpr bool REAL = C::REAL;
  MI_SMEM_DECL(smem);
  cf* lds = reinterpret_cast<cf*>(smem);
  cf* tw_lds = lds + C::DATA_ELEMS;
  const int t = threadIdx.x;
  for (int i = t; i < C::TW_ELEMS; i += C::THREADS) tw_lds[i] = a.tw[i];
  __syncthreads();
  const int line = t % C::P, u = t / C::P;
  using I0 = TileStage<C, 0>;
  using I1 = TileStage<C, 1>;
  const SideMap& im = a.imap;
  const SideMap& om = a.omap;
  const TileAxis& A0 = a.ax[0];
  const TileAxis& A1 = a.ax[1];
  const unsigned per_image = (unsigned)A0.nb * (REAL ? ((unsigned)A1.nb + 1u) / 2u : (unsigned)A1.nb);
  for (long long tile = blockIdx.x; tile < a.num_tiles; tile += gridDim.x) {
    const unsigned sb = (unsigned)tile / per_image, r = (unsigned)tile - sb * per_image, j1 = r / (unsigned)A0.nb, j0 = r - j1 * (unsigned)A0.nb;
    const int s00 = (int)j0 * A0.L - A0.pre, s01 = (int)(REAL ? 2u * j1 : j1) * A1.L - A1.pre;      // the tile's first signal index on each axis (REAL: partner a's)
    cf v[C::E];
#define MI_TILE_IN_LINE (long long)sb
#include "kern_tiles_forward.inc"
#undef MI_TILE_IN_LINE
    if (a.spectrum_only) {      // the spectrum as the product reads it: bin (k0, k1 = line) at [k0 * P + k1]
      cf* g = a.out + (long long)sb * (C::P * C::P);
      for (int k0 = u; k0 < C::P; k0 += C::TPL) g[k0 * C::P + line] = lds[tile_index<C, false>(line, k0)];
      __syncthreads();          // LDS is re-used by the next tile
      continue;
    }
    // ---- product in the loads of the inverse's first stage; inverse, rows ----
#pragma unroll
    for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
      for (int q = 0; q < I0::R; ++q) {
        const int k0 = u + b * C::TPL + q * (C::P / I0::R);
        cf h = a.spectrum[k0 * C::P + line];
        if (a.conj) h.y = -h.y;
        v[b * I0::R + q] = cswap(cmul(lds[tile_index<C, false>(line, k0)], h));
      }
    }
    __syncthreads();
#define MI_TILE_OUT_ORIGIN om.offset + (long long)sb * om.batch_stride
#include "kern_tiles_inverse.inc"
#undef MI_TILE_OUT_ORIGIN
  }
}

// the real form: instantiated in a unit of its own (tiles_rconv_ols.hip)
template <int P_, int R0_, int R1_, int THREADS_> struct RTileCfg : TileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool REAL = true; };
// the circular forms of both (routes tiles-conv-ols[..,wrap], tiles-rconv-ols[..,wrap]): units of their own again (tiles_conv_ols_wrap.hip, tiles_rconv_ols_wrap.hip)
template <int P_, int R0_, int R1_, int THREADS_> struct WTileCfg : TileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool WRAP = true; };
template <int P_, int R0_, int R1_, int THREADS_> struct WRTileCfg : RTileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool WRAP = true; };

// ---- the sum over input channels (fftConv.inputChannels = C > 1; routes tiles-conv-ols-sum, tiles-rconv-ols-sum): y[b][k] = sum_c x[b][c] (*) h[k][c], the sum
// taken in the frequency domain of the tile.  A work item loops over c: channel c's tile from input line sb C + c (the origin, the windows and the lane's
// positions do not depend on c), the forward passes, then acc += spectrum of the tile * H[c] in the registers the inverse's first stage starts from; after the loop
// ONE inverse and ONE store.  Per tile position and output kernel: C tile reads and forward transforms, as C single-channel launches would take, but one inverse
// transform and one tile-window write instead of C, and no partial results to add.  `spectrum` holds the C spectra of the launch's output kernel, channel c at
// c P^2 (LM_TILES_SPECTRUM on K C kernels stores that order).  Real pairs need nothing new: sum_c IFFT(FFT(a_c + i b_c) H_c) keeps tile a's sum in the real parts
// and tile b's in the imaginary parts, and an absent partner stays absent in every channel.  The load, the forward passes, the inverse and the store are the
// single-channel kernel's text (the two .inc files).  Linear boundaries only.
// The accumulators are E more complex values a thread: the configurations re-form the lane's positions in every tile (REFORM_POSITIONS, as P = 128 does) and
// then hold 128 VGPRs without scratch at P = 64, four workgroups a CU as before (profiles/fftconv_sum_resource_usage.log).
// The existing kernels take TilesArgs by value, so the channel count travels in a wrapper (as RconvOlsArgs wraps LineArgs)
struct TilesSumArgs { TilesArgs a; int channels; };
template <int P_, int R0_, int R1_, int THREADS_> struct STileCfg : TileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool CSUM = true, REFORM_POSITIONS = true; };
template <int P_, int R0_, int R1_, int THREADS_> struct SRTileCfg : RTileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool CSUM = true, REFORM_POSITIONS = true; };

template <class C>
__global__ void __launch_bounds__(C::THREADS, C::WAVES_PER_SIMD) fft_tiles_conv_ols_sum_kernel(const TilesSumArgs sa) {
  static_assert(C::CSUM && !C::WRAP, "the sum configurations: linear boundaries");
  constexpr bool REAL = C::REAL;
  const TilesArgs& a = sa.a;
  const int channels = sa.channels;
  MI_SMEM_DECL(smem);
  cf* lds = reinterpret_cast<cf*>(smem);
  cf* tw_lds = lds + C::DATA_ELEMS;
  const int t = threadIdx.x;
  for (int i = t; i < C::TW_ELEMS; i += C::THREADS) tw_lds[i] = a.tw[i];
  __syncthreads();
  const int line = t % C::P, u = t / C::P;
  using I0 = TileStage<C, 0>;
  using I1 = TileStage<C, 1>;
  const SideMap& im = a.imap;
  const SideMap& om = a.omap;
  const TileAxis& A0 = a.ax[0];
  const TileAxis& A1 = a.ax[1];
  const unsigned per_image = (unsigned)A0.nb * (REAL ? ((unsigned)A1.nb + 1u) / 2u : (unsigned)A1.nb);
  for (long long tile = blockIdx.x; tile < a.num_tiles; tile += gridDim.x) {
    const unsigned sb = (unsigned)tile / per_image, r = (unsigned)tile - sb * per_image, j1 = r / (unsigned)A0.nb, j0 = r - j1 * (unsigned)A0.nb;
    const int s00 = (int)j0 * A0.L - A0.pre, s01 = (int)(REAL ? 2u * j1 : j1) * A1.L - A1.pre;
    cf v[C::E], acc[C::E];
#pragma unroll
    for (int i = 0; i < C::E; ++i) acc[i] = cf{0.0f, 0.0f};
    for (int c = 0; c < channels; ++c) {
#define MI_TILE_IN_LINE ((long long)sb * channels + c)
#include "kern_tiles_forward.inc"
#undef MI_TILE_IN_LINE
      // the bins the inverse's first stage starts from, times channel c's spectrum (conjugated when correlating), into the running sums
      const cf* hs = a.spectrum + (long long)c * (C::P * C::P);
#pragma unroll
      for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
        for (int q = 0; q < I0::R; ++q) {
          const int k0 = u + b * C::TPL + q * (C::P / I0::R);
          cf h = hs[k0 * C::P + line];
          if (a.conj) h.y = -h.y;
          acc[b * I0::R + q] += cmul(lds[tile_index<C, false>(line, k0)], h);
        }
      }
      __syncthreads();          // LDS is re-used by the next channel, and then by the inverse
    }
#pragma unroll
    for (int i = 0; i < C::E; ++i) v[i] = cswap(acc[i]);
#define MI_TILE_OUT_ORIGIN om.offset + (long long)sb * om.batch_stride
#include "kern_tiles_inverse.inc"
#undef MI_TILE_OUT_ORIGIN
  }
}

// ---- grouped and depthwise convolution (fftConv.groups = G > 1; routes tiles-conv-ols-group, tiles-rconv-ols-group): y[b][k] = sum_{c < Cg} x[b][g Cg + c] (*) h[k][c],
// g = k / Kg, Cg = C / G, Kg = K / G, EVERY output kernel in one launch.  A work item is (sb, k, tile): item = (sb K + k) per_image + tile, tile fastest, so that
// the items of one image and kernel are neighbours (they share the kernel's spectra) and the K kernels of an image follow each other (those of a group read the
// same input tiles).  The decomposition is 32-bit unsigned and the same for every lane; of it only three values stay live across the item: the first input line
// sb C + g Cg, the kernel's first spectrum k Cg P^2 and the origin of the output lane om.offset + k lane_k + sb om.batch_stride (the store map is kernel 0's).
// Two forms:
//   Cg > 1 (GTileCfg / GRTileCfg)  the sum kernel's item: a loop over the group's channels around load, forward and multiply-accumulate, one inverse, one store
//   Cg = 1 (DTileCfg / DRTileCfg)  depthwise (with a channel multiplier when Kg > 1): the single-channel kernel's item, the product in the loads of the inverse's
//                                  first stage, no accumulators
// Linear boundaries only.  The load, the forward passes, the inverse and the store are the two .inc files' text.  All four configurations re-form the lane's
// positions in every tile (REFORM_POSITIONS): the depthwise ones spilt 44 / 52 bytes a lane holding them, as the single-channel P = 64 instances do, and take
// 113 / 114 VGPRs without; the sum ones sit at 128 like the sum kernel's.  No scratch, four workgroups a CU (profiles/fftconv_group_resource_usage.log)
struct TilesGroupArgs { TilesArgs a; int channels, item_lines, kernels, kernels_per_group; long long out_kernel_stride; };   // Cg, C, K, Kg, ConvGeom::lane_k
template <int P_, int R0_, int R1_, int THREADS_> struct GTileCfg : STileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool DEPTHWISE = false; };
template <int P_, int R0_, int R1_, int THREADS_> struct GRTileCfg : SRTileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool DEPTHWISE = false; };
template <int P_, int R0_, int R1_, int THREADS_> struct DTileCfg : TileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool DEPTHWISE = true, REFORM_POSITIONS = true; };
template <int P_, int R0_, int R1_, int THREADS_> struct DRTileCfg : RTileCfg<P_, R0_, R1_, THREADS_> { static constexpr bool DEPTHWISE = true, REFORM_POSITIONS = true; };
template <int P_, int R0_, int R1_, int THREADS_, int DW, bool REAL> struct GroupTileCfgOf {
  using type = typename std::conditional<DW != 0, typename std::conditional<REAL, DRTileCfg<P_, R0_, R1_, THREADS_>, DTileCfg<P_, R0_, R1_, THREADS_>>::type,
                                         typename std::conditional<REAL, GRTileCfg<P_, R0_, R1_, THREADS_>, GTileCfg<P_, R0_, R1_, THREADS_>>::type>::type;
};
template <int P_, int R0_, int R1_, int THREADS_, int DW, bool REAL> using GroupTileCfg = typename GroupTileCfgOf<P_, R0_, R1_, THREADS_, DW, REAL>::type;

template <class C>
__global__ void __launch_bounds__(C::THREADS, C::WAVES_PER_SIMD) fft_tiles_conv_ols_group_kernel(const TilesGroupArgs ga) {
  static_assert(!C::WRAP, "the grouped configurations: linear boundaries");
  constexpr bool REAL = C::REAL;
  const TilesArgs& a = ga.a;
  MI_SMEM_DECL(smem);
  cf* lds = reinterpret_cast<cf*>(smem);
  cf* tw_lds = lds + C::DATA_ELEMS;
  const int t = threadIdx.x;
  for (int i = t; i < C::TW_ELEMS; i += C::THREADS) tw_lds[i] = a.tw[i];
  __syncthreads();
  const int line = t % C::P, u = t / C::P;
  using I0 = TileStage<C, 0>;
  using I1 = TileStage<C, 1>;
  const SideMap& im = a.imap;
  const SideMap& om = a.omap;
  const TileAxis& A0 = a.ax[0];
  const TileAxis& A1 = a.ax[1];
  const unsigned per_image = (unsigned)A0.nb * (REAL ? ((unsigned)A1.nb + 1u) / 2u : (unsigned)A1.nb);
  for (long long tile = blockIdx.x; tile < a.num_tiles; tile += gridDim.x) {
    const unsigned sk = (unsigned)tile / per_image, r = (unsigned)tile - sk * per_image, j1 = r / (unsigned)A0.nb, j0 = r - j1 * (unsigned)A0.nb;
    const int s00 = (int)j0 * A0.L - A0.pre, s01 = (int)(REAL ? 2u * j1 : j1) * A1.L - A1.pre;
    // the item's image sb and kernel k, and what is kept of them: its first input line, its first spectrum, the origin of its output lane
    long long in_line, out_origin;
    const cf* hs;
    {
      const unsigned sb = sk / (unsigned)ga.kernels, k = sk - sb * (unsigned)ga.kernels, g = k / (unsigned)ga.kernels_per_group;
      in_line = (long long)sb * ga.item_lines + (long long)g * ga.channels;
      hs = a.spectrum + (long long)k * ga.channels * (C::P * C::P);
      out_origin = om.offset + (long long)k * ga.out_kernel_stride + (long long)sb * om.batch_stride;
    }
    cf v[C::E];
    if constexpr (C::DEPTHWISE) {
#define MI_TILE_IN_LINE in_line
#include "kern_tiles_forward.inc"
#undef MI_TILE_IN_LINE
      // ---- product in the loads of the inverse's first stage ----
#pragma unroll
      for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
        for (int q = 0; q < I0::R; ++q) {
          const int k0 = u + b * C::TPL + q * (C::P / I0::R);
          cf h = hs[k0 * C::P + line];
          if (a.conj) h.y = -h.y;
          v[b * I0::R + q] = cswap(cmul(lds[tile_index<C, false>(line, k0)], h));
        }
      }
      __syncthreads();
    } else {
      cf acc[C::E];
#pragma unroll
      for (int i = 0; i < C::E; ++i) acc[i] = cf{0.0f, 0.0f};
      for (int c = 0; c < ga.channels; ++c) {
#define MI_TILE_IN_LINE (in_line + c)
#include "kern_tiles_forward.inc"
#undef MI_TILE_IN_LINE
        const cf* hc = hs + (long long)c * (C::P * C::P);
#pragma unroll
        for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
          for (int q = 0; q < I0::R; ++q) {
            const int k0 = u + b * C::TPL + q * (C::P / I0::R);
            cf h = hc[k0 * C::P + line];
            if (a.conj) h.y = -h.y;
            acc[b * I0::R + q] += cmul(lds[tile_index<C, false>(line, k0)], h);
          }
        }
        __syncthreads();          // LDS is re-used by the next channel, and then by the inverse
      }
#pragma unroll
      for (int i = 0; i < C::E; ++i) v[i] = cswap(acc[i]);
    }
#define MI_TILE_OUT_ORIGIN out_origin
#include "kern_tiles_inverse.inc"
#undef MI_TILE_OUT_ORIGIN
  }
}

}  // namespace mi355
