// kern_tiles_forward.inc — a tile's load and forward 2-D FFT, the text shared by fft_tiles_conv_ols_kernel and fft_tiles_conv_ols_sum_kernel (kern_tiles.hpp, which
// includes it inside the tile loop; the names it uses are that loop's).  Shared as text and not as a function: the single-channel instances compile from the
// token sequence they always had, so their registers and schedules stay what they were.  MI_TILE_IN_LINE: the input line the tile is loaded from
// (the work item's image sb; in the sum form channel c of it)
    // ---- forward, columns: stage 0 from global memory (this lane: column i0 = line) ----
    if constexpr (C::WRAP) {
      // circular: signal index (s0_a + i_a) mod fN_a on both axes; fN_a >= 2 P, so one conditional add (the head of a convolution's first tile) and one
      // conditional subtract (past the seam) wrap it.  Axis 0 is the lane's: its wrapped column once per tile.  On axis 1 the head's wrap moves the tile's
      // origin, the same for every lane; past the seam the index falls back by fN_1.  The map's bounds apply to the wrapped indices, the only ones that
      // are dereferenced.  REAL: the two partners wrap independently; an absent partner b (odd nb_1) loads nothing, under a predicate every lane shares
      const int N0 = A0.fN, N1 = A1.fN, p0 = s00 + line, h0 = p0 < 0 ? p0 + N0 : p0, q0 = h0 >= N0 ? h0 - N0 : h0;
      const bool ok0 = q0 >= im.lo[0] && q0 < im.hi[0];
      const long long base = im.offset + MI_TILE_IN_LINE * im.batch_stride + (long long)q0 * im.stride[0];
      const int lo1 = im.lo[1], hi1 = im.hi[1], s01w = s01 < 0 ? s01 + N1 : s01;
      const long long s1 = im.stride[1];
      int ul = u;
      if constexpr (C::REFORM_POSITIONS) MI_TILE_OPAQUE_LANE(ul);
      if constexpr (REAL) {
        const float* x = reinterpret_cast<const float*>(a.in) + base;
        const int s01b = s01 + A1.L, s01bw = s01b < 0 ? s01b + N1 : (s01b >= N1 ? s01b - N1 : s01b);
        const bool okb = ok0 && 2u * j1 + 1u < (unsigned)A1.nb;
#pragma unroll
        for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
          for (int q = 0; q < I0::R; ++q) {
            const int i1 = ul + b * C::TPL + q * (C::P / I0::R);
            const int ta = s01w + i1, qa = ta >= N1 ? ta - N1 : ta, tb = s01bw + i1, qb = tb >= N1 ? tb - N1 : tb;
            cf xv = {0.0f, 0.0f};
            if (ok0 && qa >= lo1 && qa < hi1) xv.x = x[(long long)qa * s1];
            if (okb && qb >= lo1 && qb < hi1) xv.y = x[(long long)qb * s1];
            v[b * I0::R + q] = xv;
          }
        }
      } else {
        const cf* x = a.in + base;
#pragma unroll
        for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
          for (int q = 0; q < I0::R; ++q) {
            const int t1 = s01w + ul + b * C::TPL + q * (C::P / I0::R), q1 = t1 >= N1 ? t1 - N1 : t1;
            cf xv = {0.0f, 0.0f};
            if (ok0 && q1 >= lo1 && q1 < hi1) xv = x[(long long)q1 * s1];
            v[b * I0::R + q] = xv;
          }
        }
      }
    } else if constexpr (REAL) {
      const int q0 = s00 + line;
      const bool ok0 = q0 >= im.lo[0] && q0 < im.hi[0];
      const float* x = reinterpret_cast<const float*>(a.in) + (im.offset + MI_TILE_IN_LINE * im.batch_stride + (long long)q0 * im.stride[0]);   // (dereferenced inside [lo, hi) only)
      const int s01b = s01 + A1.L;                                                 // partner b: the next tile on axis 1
      const int l1 = im.lo[1] - s01, h1 = im.hi[1] - s01, l1b = im.lo[1] - s01b, h1b = im.hi[1] - s01b;
      const int lo1 = l1 < 0 ? 0 : l1, hi1 = h1 > C::P ? C::P : h1;               // each partner's share of [lo, hi) on axis 1
      const int lo1b = l1b < 0 ? 0 : l1b, hi1b = h1b > C::P ? C::P : h1b;
      const long long s1 = im.stride[1];
      int ul = u;
      if constexpr (C::REFORM_POSITIONS) MI_TILE_OPAQUE_LANE(ul);
#pragma unroll
      for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
        for (int q = 0; q < I0::R; ++q) {
          const int i1 = ul + b * C::TPL + q * (C::P / I0::R);
          cf xv = {0.0f, 0.0f};
          if (ok0 && i1 >= lo1 && i1 < hi1) xv.x = x[(long long)(s01 + i1) * s1];
          if (ok0 && i1 >= lo1b && i1 < hi1b) xv.y = x[(long long)(s01b + i1) * s1];
          v[b * I0::R + q] = xv;
        }
      }
    } else {
      const int q0 = s00 + line;
      const bool ok0 = q0 >= im.lo[0] && q0 < im.hi[0];
      const cf* x = a.in + (im.offset + MI_TILE_IN_LINE * im.batch_stride + (long long)q0 * im.stride[0]);   // (dereferenced inside [lo, hi) only)
      const int l1 = im.lo[1] - s01, h1 = im.hi[1] - s01;
      const int lo1 = l1 < 0 ? 0 : l1, hi1 = h1 > C::P ? C::P : h1;               // the tile's share of [lo, hi) on axis 1
      const long long s1 = im.stride[1];
      int ul = u;
      if constexpr (C::REFORM_POSITIONS) MI_TILE_OPAQUE_LANE(ul);
#pragma unroll
      for (int b = 0; b < I0::NB; ++b) {
#pragma unroll
        for (int q = 0; q < I0::R; ++q) {
          const int i1 = ul + b * C::TPL + q * (C::P / I0::R);
          cf xv = {0.0f, 0.0f};
          if (ok0 && i1 >= lo1 && i1 < hi1) xv = x[(long long)(s01 + i1) * s1];
          v[b * I0::R + q] = xv;
        }
      }
    }
    tile_stage_compute<C, 0>(v, tw_lds, u);
    tile_stage_write<C, 0, true>(v, lds, line, u);
    __syncthreads();
    tile_stage_read<C, 1, true>(v, lds, line, u);
    __syncthreads();
    tile_stage_compute<C, 1>(v, tw_lds, u);
    tile_stage_write<C, 1, true>(v, lds, line, u);
    __syncthreads();
    // ---- forward, rows (this lane: row i1 = line) ----
    tile_stage_read<C, 0, false>(v, lds, line, u);
    __syncthreads();
    tile_stage_compute<C, 0>(v, tw_lds, u);
    tile_stage_write<C, 0, false>(v, lds, line, u);
    __syncthreads();
    tile_stage_read<C, 1, false>(v, lds, line, u);
    __syncthreads();
    tile_stage_compute<C, 1>(v, tw_lds, u);
    tile_stage_write<C, 1, false>(v, lds, line, u);
    __syncthreads();
