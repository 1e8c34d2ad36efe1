// The per-sample gather of the colour renders' adjoints in the density (absorb.hip, exposure.hip): ONE stencil (ray_coords,
// axis_setup: common.h) gathers the C channels of the emission q [D,H,W,C] and contracts them with the ray's gradient g[C],
//   a = sum_c g[c] trilinear(q[..., c]),
// and, WITH_D, the sample s = trilinear(d) of the density from the same corners (without it d is not read and s is 0).
// As x-pairs where W >= 2 (one load of 2 C floats of q, and an 8-byte load of d, per (z, y) corner pair; clamped stencils
// select within the pair) and through tri_setup and scalar loads where W == 1.  The sums run in tri_setup's corner order,
// x innermost, whichever kernel includes this.  axis_setup clamps every corner into the volume whatever the matrix is (also
// for NaN coordinates), and a pair load reads x = min(i0, W - 2) and its neighbour; offsets into q (times C <= 4) are 64-bit.
#pragma once
#include "common.h"

namespace nfs {

template <int N>
struct __attribute__((packed, aligned(4))) FNu { float v[N]; };

template <int C, bool WITH_D>
__device__ __forceinline__ void ray_sample_pairs(const float* __restrict__ d, const float* __restrict__ q, const float* r,
                                                 const float* g, int D, int H, int W, int z, int h, int x, float& s,
                                                 float& a) {
  float cx, cy, cz;
  ray_coords(r, D, H, W, z, h, x, cx, cy, cz);
  const Axis az = axis_setup(cx, D), ay = axis_setup(cy, H), ax = axis_setup(cz, W);
  const int xb = min(ax.i0, W - 2);                 // pair base; clamped stencils select below
  const bool x0_lo = ax.i0 == xb, x1_lo = ax.i1 == xb;
  const float wz[2] = {1.f - az.w1, az.w1}, wy[2] = {1.f - ay.w1, ay.w1}, wx[2] = {1.f - ax.w1, ax.w1};
  const int iz[2] = {az.i0, az.i1}, iy[2] = {ay.i0, ay.i1};
  float sv = 0.f, qc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) qc[c] = 0.f;
#pragma unroll
  for (int ia = 0; ia < 2; ++ia)
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      const int64_t o = ((int64_t)iz[ia] * H + iy[ib]) * W + xb;
      F2u p = {0.f, 0.f};
      if constexpr (WITH_D) p = *reinterpret_cast<const F2u*>(d + o);
      const FNu<2 * C> pq = *reinterpret_cast<const FNu<2 * C>*>(q + o * C);
      const float w0 = wz[ia] * wy[ib] * wx[0], w1 = wz[ia] * wy[ib] * wx[1];
      if constexpr (WITH_D) {
        sv += w0 * (x0_lo ? p.x : p.y);
        sv += w1 * (x1_lo ? p.x : p.y);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        qc[c] += w0 * (x0_lo ? pq.v[c] : pq.v[C + c]);
        qc[c] += w1 * (x1_lo ? pq.v[c] : pq.v[C + c]);
      }
    }
  float av = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) av += g[c] * qc[c];
  s = sv;
  a = av;
}

template <int C, bool WITH_D>
__device__ __forceinline__ void ray_sample_scalar(const float* __restrict__ d, const float* __restrict__ q, const float* r,
                                                  const float* g, int D, int H, int W, int z, int h, int x, float& s,
                                                  float& a) {
  float cx, cy, cz;
  ray_coords(r, D, H, W, z, h, x, cx, cy, cz);
  Tri t; Axis ax, ay, az;
  tri_setup(cx, cy, cz, D, H, W, t, ax, ay, az);
  float sv = 0.f, qc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) qc[c] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if constexpr (WITH_D) sv += t.w[k] * d[t.o[k]];
    const float* p = q + t.o[k] * C;
#pragma unroll
    for (int c = 0; c < C; ++c) qc[c] += t.w[k] * p[c];
  }
  float av = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) av += g[c] * qc[c];
  s = sv;
  a = av;
}

// do [a, a + na) and [b, b + nb) floats share an address?  (a null range shares none)
static inline bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * 4, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * 4;
  return a0 < b1 && b0 < a1;
}

}  // namespace nfs
