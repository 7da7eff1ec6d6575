// kern_tiles_inverse.inc — a tile's inverse 2-D FFT from the products in v[] and its store, the text shared by fft_tiles_conv_ols_kernel and
// fft_tiles_conv_ols_sum_kernel (kern_tiles.hpp; see kern_tiles_forward.inc).  MI_TILE_OUT_ORIGIN: the element the work item's output lane starts at, without
// parentheses (om.offset + sb * om.batch_stride in the kernels whose launch has one output kernel: the tokens they always had; the grouped kernel adds its kernel's lane)
    tile_stage_compute<C, 0>(v, tw_lds, u);
    tile_stage_write<C, 0, false>(v, lds, line, u);
    __syncthreads();
    tile_stage_read<C, 1, false>(v, lds, line, u);
    __syncthreads();
    tile_stage_compute<C, 1>(v, tw_lds, u);
    tile_stage_write<C, 1, false>(v, lds, line, u);
    __syncthreads();
    // ---- inverse, columns: the last stage stores to global memory ----
    tile_stage_read<C, 0, true>(v, lds, line, u);
    __syncthreads();
    tile_stage_compute<C, 0>(v, tw_lds, u);
    tile_stage_write<C, 0, true>(v, lds, line, u);
    __syncthreads();
    tile_stage_read<C, 1, true>(v, lds, line, u);
    __syncthreads();            // everyone has its inputs: LDS is free for the next tile
    tile_stage_compute<C, 1>(v, tw_lds, u);
    if constexpr (REAL) {
      const int q0 = s00 + line;
      const int m0 = q0 < 0 ? q0 + A0.fN : q0;                                   // (the negative lags of a correlation sit at the top of the domain)
      const bool ok0 = line >= A0.w0 && line < A0.w0 + A0.L && q0 < A0.plim && m0 >= om.lo[0] && m0 < om.hi[0];
      const bool z0 = m0 < om.zlo[0] || m0 >= om.zhi[0];
      float* y = reinterpret_cast<float*>(a.out) + (MI_TILE_OUT_ORIGIN + (long long)m0 * om.stride[0]);   // (dereferenced inside the crop only)
      const long long s1 = om.stride[1];
      const int s01b = s01 + A1.L;
      int wlo = A1.w0, us = u;
      MI_TILE_OPAQUE(wlo);
      if constexpr (C::REFORM_POSITIONS) MI_TILE_OPAQUE_LANE(us);
      const int wend = A1.w0 + A1.L, pend = A1.plim - s01, whi = wend < pend ? wend : pend;   // each partner's window, cut at the last index the signal gives;
      const int pendb = A1.plim - s01b, whib = wend < pendb ? wend : pendb;                    // an absent partner's is empty: s0_1(b) + w0_1 >= plim_1 in both modes
#pragma unroll
      for (int b = 0; b < I1::NB; ++b) {
#pragma unroll
        for (int q = 0; q < I1::R; ++q) {
          const int i1 = tile_stage_out<C, 1>(us, b, q);
          if (!ok0 || i1 < wlo) continue;
          const cf r = cswap(v[b * I1::R + q]) * a.scale;
          if (i1 < whi) {
            const int q1 = s01 + i1, m1 = q1 < 0 ? q1 + A1.fN : q1;
            if (m1 >= om.lo[1] && m1 < om.hi[1]) y[(long long)m1 * s1] = (z0 || m1 < om.zlo[1] || m1 >= om.zhi[1]) ? 0.0f : r.x;
          }
          if (i1 < whib) {
            const int q1 = s01b + i1, m1 = q1 < 0 ? q1 + A1.fN : q1;
            if (m1 >= om.lo[1] && m1 < om.hi[1]) y[(long long)m1 * s1] = (z0 || m1 < om.zlo[1] || m1 >= om.zhi[1]) ? 0.0f : r.y;
          }
        }
      }
    } else {
      const int q0 = s00 + line;
      const int m0 = q0 < 0 ? q0 + A0.fN : q0;                                   // (the negative lags of a correlation sit at the top of the domain)
      const bool ok0 = line >= A0.w0 && line < A0.w0 + A0.L && q0 < A0.plim && m0 >= om.lo[0] && m0 < om.hi[0];
      const bool z0 = m0 < om.zlo[0] || m0 >= om.zhi[0];
      cf* y = a.out + (MI_TILE_OUT_ORIGIN + (long long)m0 * om.stride[0]);   // (dereferenced inside the crop only)
      const long long s1 = om.stride[1];
      int wlo = A1.w0, us = u;
      MI_TILE_OPAQUE(wlo);
      if constexpr (C::REFORM_POSITIONS) MI_TILE_OPAQUE_LANE(us);
      const int wend = A1.w0 + A1.L, pend = A1.plim - s01, whi = wend < pend ? wend : pend;   // the window, cut at the last index the signal gives
#pragma unroll
      for (int b = 0; b < I1::NB; ++b) {
#pragma unroll
        for (int q = 0; q < I1::R; ++q) {
          const int i1 = tile_stage_out<C, 1>(us, b, q), q1 = s01 + i1;
          if (!ok0 || i1 < wlo || i1 >= whi) continue;
          const int m1 = q1 < 0 ? q1 + A1.fN : q1;
          if (m1 < om.lo[1] || m1 >= om.hi[1]) continue;
          cf r = cswap(v[b * I1::R + q]) * a.scale;
          if (z0 || m1 < om.zlo[1] || m1 >= om.zhi[1]) r = cf{0.0f, 0.0f};
          y[(long long)m1 * s1] = r;
        }
      }
    }
