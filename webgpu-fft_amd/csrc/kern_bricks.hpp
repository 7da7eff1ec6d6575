// kern_bricks.hpp — overlap-save on rank-3 complex bricks (type MI355FFT_FFTCONV, route bricks-conv-ols): forward 3-D FFT, product with one kernel
// spectrum and inverse 3-D FFT of a 16 x 16 x 16 brick without leaving LDS.  The 3-D form of kern_tiles.hpp fft_tiles_conv_ols_kernel: its block
// geometry once per axis a (axis 0 fastest, as everywhere in the planner):
//   M_a = kernelShape[a], pre_a = M_a - 1, L_a = 16 - pre_a, fN_a = shape[a] + M_a - 1, nb_a = ceil(fN_a / L_a)
//   brick (j0, j1, j2) of volume b holds signal indices [s0_a, s0_a + 16), s0_a = j_a L_a - pre_a, and gives the L0 x L1 x L2 results of its window
//   [w0_a, w0_a + L_a): w0_a = pre_a (convolution) or 0 (correlation); q_a = s0_a + i_a < plim_a (shape[a] when correlating, else fN_a);
//   logical index m_a = q_a < 0 ? q_a + fN_a : q_a (the negative lags of a correlation sit at the top of each axis of the domain)
//
// One workgroup of 256 threads owns a brick.  A pass transforms the 256 lines of one axis, one line a thread: the line's 16 values sit in registers and
// the pass is one fft_radix<16> (radix.hpp): no stage structure, no root table.  A thread reads its whole line before it writes it back to the same
// places, so one barrier between two passes is all the ordering there is.  With t the thread:
//   pass 2 (lines along axis 2): lane (i0 = t % 16, i1 = t / 16) — consecutive lanes are consecutive along axis 0: runs of 16 elements in global memory
//   pass 1 (lines along axis 1): lane (i0 = t % 16, k2 = t / 16)
//   pass 0 (lines along axis 0): lane (k1 = t % 16, k2 = t / 16)
// Forward runs passes 2, 1, 0 and the inverse 0, 1, 2: pass 2 loads straight from global memory going in and stores straight to it coming out, and the
// forward and the inverse pass 0 are the same thread on the same line, so the product happens in registers between them.  Four barriers a brick; none
// between bricks (the inverse pass 2 reads, and the next brick's pass 2 writes, the thread's own line).
//   load    : 8-byte loads through imap; on all three axes its bounds are moved by the brick's origin, zero elsewhere: the embed and zeroPad.read are the
//             map's predicates, strided lanes its strides.  Nothing outside [lo, hi) is dereferenced
//   product : v[k0] * spectrum (conjugated when correlating), re and im swapped so that the inverse re-uses the forward butterflies.  The spectrum is read
//             per brick (cache hits) in the order pass 0 holds it: bin (k0, k1, k2) at [k0 * 256 + k2 * 16 + k1] = [k0 * 256 + t], consecutive lanes on
//             consecutive elements; LM_BRICKS_SPECTRUM is this kernel's forward half storing that order
//   store   : positions inside all three windows, then the crop [lo_a, hi_a) of omap, zeroPad.write (zlo, zhi) and the output lane; scale 1 / 4096
// Element indices are 32-bit (the planner keeps every fN_a, the bricks a volume and the work items below 2^31 - 16384); buffer offsets are formed in 64 bits
//
// LDS: element (i0, i1, i2) at i0 + P1 i1 + P2 i2, 8 bytes each, P1 = 17, P2 = 16 P1 = 272.  The bank rule: a ds_read_b64 serves 32 lanes at once on 64
// banks of 4 bytes, so a half-wave is conflict-free iff its 32 element addresses differ mod 32; a ds_write_b64 serves 16 contiguous lanes on 32 banks:
// iff their 16 addresses differ mod 16.  For register r of a lane the three passes touch
//   pass 2:  i0 + 17 i1 + 272 r,  half-wave: i0 = 0..15, i1 = {2m, 2m+1}
//   pass 1:  i0 + 17 r + 272 k2,  half-wave: i0 = 0..15, k2 = {2m, 2m+1}:  272 = 16 mod 32 puts the two k2 on the two halves of the 32 residues: free
//   pass 0:  r + 17 k1 + 272 k2,  half-wave: k1 = 0..15, k2 = {2m, 2m+1}:  17 k1 mod 32 = k1 + 16 (k1 & 1), 16 residues whose complement is the same set
//            + 16, which the other k2 takes: free.  Every write: i0 or 17 k1 = k1 mod 16 over 16 lanes: free
//   pass 2's writes are free (i0 over 16 lanes); its reads (the inverse's last pass, 16 of a brick's 64 reads a thread) are not: the two i1 rows cover
//   [c, c + 15] and [c + 17, c + 32] mod 32, which meet on one bank: one 2-way conflict a half-wave.
// No pair of pitches removes that: whatever the lanes, a pass is conflict-free only if its 256 addresses fall 8 on each residue mod 32.  For i0 + P1 i1
// and i0 + P2 i2 that takes P1 and P2 even (counted for every pitch mod 32: each odd one leaves some residue with 9 cells; 17 gives residue 0 the cell
// (0, 0) and the eight with i0 + i1 = 16, i1 odd), and then every address P1 k1 + P2 k2 of pass 0 is even: 16 residues for 256 addresses.  So one pass keeps
// a conflict under any pitches i0 + P1 i1 + P2 i2, and these put the cheapest one (a read, 2 LDS cycles where a write takes 6) on one pass and leave the other
// five access patterns free (counters: profiles/fftconv_bricks_resource_usage.log).
//
// Real data (type MI355FFT_FFTCONV_REAL, route bricks-rconv-ols, the kernel on an RBrickCfg): two real bricks a and b ride one complex brick as z = a + i b.
// The kernel h is real, so IFFT(FFT(z) H) = (a (*) h) + i (b (*) h), and with conj(H) the two correlations: the real parts are brick a's results and the
// imaginary parts brick b's, as in kern_tiles.hpp.  The partners are neighbours on axis 2: work item (sb, j0, j1, jp) holds brick (j0, j1, 2 jp) in .x and
// brick (j0, j1, 2 jp + 1) in .y.  They share everything but s0_2(b) = s0_2(a) + L_2, the same for every lane.  pairs_2 = ceil(nb_2 / 2); with odd nb_2 the
// last pair's partner does not exist and needs no special case: s0_2(b) >= shape[2], so every load of its fails the map's hi bound, and
// s0_2(b) + w0_2 >= plim_2, so its window is empty.  Sides are 4-byte elements.  The kernel spectra come from the same kernel (LM_BRICKS_RSPECTRUM): one
// kernel per work item in .x; nb_2 = 1 and L_2 = 16 put partner b at s0_2 = 16, beyond the kernel map's hi: zero imaginary parts, the full complex spectrum
#pragma once
#include "platform.hpp"
#include "radix.hpp"
#include "plan.hpp"
#include "kern_tiles.hpp"   // TileAxis

namespace mi355 {

struct BricksArgs {
  const cf* in;         // the real form (RBrickCfg) reads `in` and writes `out` as float arrays: the maps count 4-byte elements
  cf* out;
  const cf* spectrum;   // the kernel spectrum on 16^3, bin (k0, k1, k2) at [k0 * 256 + k2 * 16 + k1]
  long long num_items;  // work items: bricks, or brick pairs in the real form (ax[2].nb stays the number of bricks)
  float scale;
  int conj;             // correlation: the spectrum's conjugate
  int spectrum_only;    // LM_BRICKS_SPECTRUM: forward half only; item k is kernel k, its spectrum stored dense at out + k 16^3
  TileAxis ax[3];
  SideMap imap, omap;
};

template <int P_, int THREADS_>
struct BrickCfg {
  static constexpr int P = P_, THREADS = THREADS_;
  static constexpr bool REAL = false;               // RBrickCfg: real brick pairs
  static constexpr bool WRAP = false;               // WBrickCfg, WRBrickCfg: circular boundary, signal indices modulo fN_a
  static_assert(P == 16 && THREADS == P * P, "a thread per line, a line per radix-16 butterfly");
  static constexpr int P1 = P + 1, P2 = P * P1;     // the pitches of axes 1 and 2 (see the header)
  static constexpr int VOLUME = P * P * P;
  static constexpr int LDS_BYTES = brick_kernel_lds_bytes(P);
  static_assert(LDS_BYTES == P * P2 * 8 && (P - 1) * (1 + P1 + P2) < P * P2, "brick does not fit its LDS");
  static constexpr int WG_PER_CU = 4;               // 34 KB each of a CU's 160 KB: 16 waves, 4 a SIMD: 128 VGPRs
  static_assert(WG_PER_CU * LDS_BYTES <= 160 * 1024, "four bricks a CU");
  static constexpr int WAVES_PER_SIMD = WG_PER_CU * (THREADS / 64) / 4;
};

// C::REAL: two real bricks, neighbours on axis 2, as re / im of the complex brick (see the header); the form differs at the loads, at the stores and where a
// work item's brick is found
template <class C>
__global__ void __launch_bounds__(C::THREADS, C::WAVES_PER_SIMD) fft_bricks_conv_ols_kernel(const BricksArgs a) {
  constexpr bool REAL = C::REAL;
  constexpr int P = C::P, P1 = C::P1, P2 = C::P2;
  MI_SMEM_DECL(smem);
  cf* lds = reinterpret_cast<cf*>(smem);
  const int t = threadIdx.x;
  const int tl = t % P, th = t / P;                 // pass 2: (i0, i1); pass 1: (i0, k2); pass 0: (k1, k2)
  cf* line2 = lds + tl + th * P1;                   // + r P2
  cf* line1 = lds + tl + th * P2;                   // + r P1
  cf* line0 = lds + tl * P1 + th * P2;              // + r
  const SideMap& im = a.imap;
  const SideMap& om = a.omap;
  const TileAxis& A0 = a.ax[0];
  const TileAxis& A1 = a.ax[1];
  const TileAxis& A2 = a.ax[2];
  const unsigned n01 = (unsigned)A0.nb * (unsigned)A1.nb;
  const unsigned per_volume = n01 * (REAL ? ((unsigned)A2.nb + 1u) / 2u : (unsigned)A2.nb);
  for (long long item = blockIdx.x; item < a.num_items; item += gridDim.x) {
    const unsigned sb = (unsigned)item / per_volume, r3 = (unsigned)item - sb * per_volume, j2 = r3 / n01, r2 = r3 - j2 * n01;
    const unsigned j1 = r2 / (unsigned)A0.nb, j0 = r2 - j1 * (unsigned)A0.nb;
    // the brick's first signal index on each axis (REAL: partner a's)
    const int s00 = (int)j0 * A0.L - A0.pre, s01 = (int)j1 * A1.L - A1.pre, s02 = (int)(REAL ? 2u * j2 : j2) * A2.L - A2.pre;
    const int s02b = s02 + A2.L;                    // REAL, partner b: the next brick on axis 2
    const int q0 = s00 + tl, q1 = s01 + th;         // pass 2: this lane's line
    cf v[P];
    // ---- forward, pass 2: from global memory ----
    if constexpr (C::WRAP) {
      // circular: signal index (s0_a + i_a) mod fN_a on the three axes, as in kern_tiles.hpp: fN_a >= 2 P, one conditional add and one conditional subtract.
      // Axes 0 and 1 are the lane's line, wrapped once per item; on axis 2 the head's wrap moves the brick's origin, the same for every lane, and past the
      // seam the index falls back by fN_2.  The map's bounds apply to the wrapped indices, the only ones that are dereferenced.  REAL: an absent partner b
      // (odd nb_2) loads nothing, under a predicate every lane shares
      const int N0 = A0.fN, N1 = A1.fN, N2 = A2.fN;
      const int h0 = q0 < 0 ? q0 + N0 : q0, c0 = h0 >= N0 ? h0 - N0 : h0, h1 = q1 < 0 ? q1 + N1 : q1, c1 = h1 >= N1 ? h1 - N1 : h1;
      const bool ok = c0 >= im.lo[0] && c0 < im.hi[0] && c1 >= im.lo[1] && c1 < im.hi[1];
      const long long base = im.offset + (long long)sb * im.batch_stride + (long long)c0 * im.stride[0] + (long long)c1 * im.stride[1];
      const long long s2 = im.stride[2];
      const int lo2 = im.lo[2], hi2 = im.hi[2], s02w = s02 < 0 ? s02 + N2 : s02;
      if constexpr (REAL) {
        const float* x = reinterpret_cast<const float*>(a.in) + base;
        const int s02bw = s02b < 0 ? s02b + N2 : (s02b >= N2 ? s02b - N2 : s02b);
        const bool okb = ok && 2u * j2 + 1u < (unsigned)A2.nb;
#pragma unroll
        for (int r = 0; r < P; ++r) {
          const int ta = s02w + r, qa = ta >= N2 ? ta - N2 : ta, tb = s02bw + r, qb = tb >= N2 ? tb - N2 : tb;
          cf xv = {0.0f, 0.0f};
          if (ok && qa >= lo2 && qa < hi2) xv.x = x[(long long)qa * s2];
          if (okb && qb >= lo2 && qb < hi2) xv.y = x[(long long)qb * s2];
          v[r] = xv;
        }
      } else {
        const cf* x = a.in + base;
#pragma unroll
        for (int r = 0; r < P; ++r) {
          const int t2 = s02w + r, q2 = t2 >= N2 ? t2 - N2 : t2;
          cf xv = {0.0f, 0.0f};
          if (ok && q2 >= lo2 && q2 < hi2) xv = x[(long long)q2 * s2];
          v[r] = xv;
        }
      }
    } else {
      const bool ok = q0 >= im.lo[0] && q0 < im.hi[0] && q1 >= im.lo[1] && q1 < im.hi[1];
      const long long base = im.offset + (long long)sb * im.batch_stride + (long long)q0 * im.stride[0] + (long long)q1 * im.stride[1];   // (dereferenced inside [lo, hi) only)
      const long long s2 = im.stride[2];
      const int l2 = im.lo[2] - s02, h2 = im.hi[2] - s02;
      const int lo2 = l2 < 0 ? 0 : l2, hi2 = h2 > P ? P : h2;                     // the brick's share of [lo, hi) on axis 2
      if constexpr (REAL) {
        const float* x = reinterpret_cast<const float*>(a.in) + base;
        const int l2b = im.lo[2] - s02b, h2b = im.hi[2] - s02b;
        const int lo2b = l2b < 0 ? 0 : l2b, hi2b = h2b > P ? P : h2b;             // partner b's
#pragma unroll
        for (int r = 0; r < P; ++r) {
          cf xv = {0.0f, 0.0f};
          if (ok && r >= lo2 && r < hi2) xv.x = x[(long long)(s02 + r) * s2];
          if (ok && r >= lo2b && r < hi2b) xv.y = x[(long long)(s02b + r) * s2];
          v[r] = xv;
        }
      } else {
        const cf* x = a.in + base;
#pragma unroll
        for (int r = 0; r < P; ++r) {
          cf xv = {0.0f, 0.0f};
          if (ok && r >= lo2 && r < hi2) xv = x[(long long)(s02 + r) * s2];
          v[r] = xv;
        }
      }
    }
    fft_radix<P>(v);
#pragma unroll
    for (int r = 0; r < P; ++r) line2[r * P2] = v[r];
    __syncthreads();
    // ---- forward, pass 1 ----
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = line1[r * P1];
    fft_radix<P>(v);
#pragma unroll
    for (int r = 0; r < P; ++r) line1[r * P1] = v[r];
    __syncthreads();
    // ---- forward, pass 0: the spectrum of the brick, bin (k0 = r, k1 = tl, k2 = th), stays in registers ----
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = line0[r];
    fft_radix<P>(v);
    if (a.spectrum_only) {      // the spectrum as the product reads it
      cf* g = a.out + (long long)sb * C::VOLUME;
#pragma unroll
      for (int r = 0; r < P; ++r) g[r * (P * P) + t] = v[r];
      __syncthreads();          // the other lanes' pass-0 reads, before the next item's pass 2 writes
      continue;
    }
    // ---- product; inverse, pass 0 ----
#pragma unroll
    for (int r = 0; r < P; ++r) {
      cf h = a.spectrum[r * (P * P) + t];
      if (a.conj) h.y = -h.y;
      v[r] = cswap(cmul(v[r], h));
    }
    fft_radix<P>(v);
#pragma unroll
    for (int r = 0; r < P; ++r) line0[r] = v[r];
    __syncthreads();
    // ---- inverse, pass 1 ----
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = line1[r * P1];
    fft_radix<P>(v);
#pragma unroll
    for (int r = 0; r < P; ++r) line1[r * P1] = v[r];
    __syncthreads();
    // ---- inverse, pass 2: to global memory ----
#pragma unroll
    for (int r = 0; r < P; ++r) v[r] = line2[r * P2];
    fft_radix<P>(v);
    {
      const int m0 = q0 < 0 ? q0 + A0.fN : q0, m1 = q1 < 0 ? q1 + A1.fN : q1;   // (the negative lags of a correlation sit at the top of the domain)
      const bool ok = tl >= A0.w0 && tl < A0.w0 + A0.L && q0 < A0.plim && m0 >= om.lo[0] && m0 < om.hi[0] &&
                      th >= A1.w0 && th < A1.w0 + A1.L && q1 < A1.plim && m1 >= om.lo[1] && m1 < om.hi[1];
      const bool z01 = m0 < om.zlo[0] || m0 >= om.zhi[0] || m1 < om.zlo[1] || m1 >= om.zhi[1];
      const long long base = om.offset + (long long)sb * om.batch_stride + (long long)m0 * om.stride[0] + (long long)m1 * om.stride[1];   // (dereferenced inside the crop only)
      const long long s2 = om.stride[2];
      const int wlo = A2.w0, wend = A2.w0 + A2.L, pend = A2.plim - s02, whi = wend < pend ? wend : pend;   // the window, cut at the last index the signal gives
      if constexpr (REAL) {
        float* y = reinterpret_cast<float*>(a.out) + base;
        const int pendb = A2.plim - s02b, whib = wend < pendb ? wend : pendb;   // an absent partner's is empty: s0_2(b) + w0_2 >= plim_2 in both modes
#pragma unroll
        for (int r = 0; r < P; ++r) {
          if (!ok || r < wlo) continue;
          const cf res = cswap(v[r]) * a.scale;
          if (r < whi) {
            const int q2 = s02 + r, m2 = q2 < 0 ? q2 + A2.fN : q2;
            if (m2 >= om.lo[2] && m2 < om.hi[2]) y[(long long)m2 * s2] = (z01 || m2 < om.zlo[2] || m2 >= om.zhi[2]) ? 0.0f : res.x;
          }
          if (r < whib) {
            const int q2 = s02b + r, m2 = q2 < 0 ? q2 + A2.fN : q2;
            if (m2 >= om.lo[2] && m2 < om.hi[2]) y[(long long)m2 * s2] = (z01 || m2 < om.zlo[2] || m2 >= om.zhi[2]) ? 0.0f : res.y;
          }
        }
      } else {
        cf* y = a.out + base;
#pragma unroll
        for (int r = 0; r < P; ++r) {
          if (!ok || r < wlo || r >= whi) continue;
          const int q2 = s02 + r, m2 = q2 < 0 ? q2 + A2.fN : q2;
          if (m2 < om.lo[2] || m2 >= om.hi[2]) continue;
          cf res = cswap(v[r]) * a.scale;
          if (z01 || m2 < om.zlo[2] || m2 >= om.zhi[2]) res = cf{0.0f, 0.0f};
          y[(long long)m2 * s2] = res;
        }
      }
    }
  }
}

// the real form: instantiated in a unit of its own (bricks_rconv_ols.hip)
template <int P_, int THREADS_> struct RBrickCfg : BrickCfg<P_, THREADS_> { static constexpr bool REAL = true; };
// the circular forms of both (routes bricks-conv-ols[..,wrap], bricks-rconv-ols[..,wrap]): units of their own again (bricks_conv_ols_wrap.hip, bricks_rconv_ols_wrap.hip)
template <int P_, int THREADS_> struct WBrickCfg : BrickCfg<P_, THREADS_> { static constexpr bool WRAP = true; };
template <int P_, int THREADS_> struct WRBrickCfg : RBrickCfg<P_, THREADS_> { static constexpr bool WRAP = true; };

}  // namespace mi355
