// kern_f16.hpp — binary16 <-> f32 streaming conversions of f16-storage plans (plan.cpp wrap_f16_storage; reference
// src/kernels/f16_storage.js).  A plan whose f32 route is not a single dense line launch runs unchanged on f32 staging
// regions in the workspace: one launch widens the caller's binary16 input in front of it, one rounds the f32 result to
// binary16 behind it.  Both count SCALARS: a complex run of n elements is 2n of them, a real run n (odd counts included).
//
// Widening is exact; narrowing rounds to nearest even (values beyond +-65504 become +-inf, NaN stays NaN).  The casts are
// plain conversions: hipcc -O3 for gfx950 turns them into v_cvt_f32_f16 and v_cvt_pk_f16_f32 (never the round-toward-zero
// v_cvt_pkrtz form).
#pragma once
#include "platform.hpp"

namespace mi355 {

typedef _Float16 h8v __attribute__((ext_vector_type(8)));   // 16 bytes of binary16
typedef float f4v __attribute__((ext_vector_type(4)));      // 16 bytes of f32

// a lane moves 8 scalars per trip: one 16-byte access on the binary16 side, two on the f32 side.  Pointers that are not
// 16-byte aligned (exec offsets need only be multiples of 4) take the scalar loop for the whole run; so does the tail.
static __global__ void __launch_bounds__(256) f16_to_f32_kernel(const _Float16* __restrict__ src, float* __restrict__ dst, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  const long long nv = vec ? n / 8 : 0;
  for (long long i = t0; i < nv; i += stride) {
    const h8v h = reinterpret_cast<const h8v*>(src)[i];
    f4v lo, hi;
    lo.x = (float)h[0]; lo.y = (float)h[1]; lo.z = (float)h[2]; lo.w = (float)h[3];
    hi.x = (float)h[4]; hi.y = (float)h[5]; hi.z = (float)h[6]; hi.w = (float)h[7];
    reinterpret_cast<f4v*>(dst)[2 * i] = lo;
    reinterpret_cast<f4v*>(dst)[2 * i + 1] = hi;
  }
  for (long long i = nv * 8 + t0; i < n; i += stride) dst[i] = (float)src[i];
}

static __global__ void __launch_bounds__(256) f32_to_f16_kernel(const float* __restrict__ src, _Float16* __restrict__ dst, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  const long long nv = vec ? n / 8 : 0;
  for (long long i = t0; i < nv; i += stride) {
    const f4v lo = reinterpret_cast<const f4v*>(src)[2 * i], hi = reinterpret_cast<const f4v*>(src)[2 * i + 1];
    h8v h;
    h[0] = (_Float16)lo.x; h[1] = (_Float16)lo.y; h[2] = (_Float16)lo.z; h[3] = (_Float16)lo.w;
    h[4] = (_Float16)hi.x; h[5] = (_Float16)hi.y; h[6] = (_Float16)hi.z; h[7] = (_Float16)hi.w;
    reinterpret_cast<h8v*>(dst)[i] = h;
  }
  for (long long i = nv * 8 + t0; i < n; i += stride) dst[i] = (_Float16)src[i];
}

}  // namespace mi355
