// The axis rule of the cell-centred grid <-> particle links, written once: nfs_g2p_fwd (splat.hip, libnfs_hip.so) and the
// carrier kernels (carrier.hip, libnfs_carrier.so: the same sampling and its transpose in the grid) include this file, so
// both libraries form indices and weights with the same text.  So does flow.hip (libnfs_flow.so), which also needs the
// weights' derivatives: g2p_axis_d below.
// g [X,Y,(Z),C] cell-centred, p [N,nd] in [0,1] (axis order = array order): x = p * n, base = floor(x - 0.5).
// linear: cells (base, base+1) clipped to [0,n-1], weight dx = x - (clipped base + 0.5) (so outside the centre
// lattice both cells coincide and the value is the border cell's); cubic: cells base-1..base+2 clipped,
// t = x - (clipped base + 0.5), Catmull-Rom weights of the reference's _hermite (transform.py:771-1231).
// Every index is clamped into [0, n-1] whatever x is (a NaN x gives base -4, i.e. cell 0), and the indices of an axis
// are non-decreasing in the tap: idx[0] is a particle's lowest cell on that axis, idx[taps - 1] its highest.
#pragma once
#include "common.h"

namespace nfs {

__device__ __forceinline__ void g2p_axis(float x, int n, int cubic, int* idx, float* w) {
  const float fb = floorf(x - 0.5f);
  const int b = (int)fminf(fmaxf(fb, -4.f), (float)n + 4.f);
  if (!cubic) {
    idx[0] = min(max(b, 0), n - 1);
    idx[1] = min(max(b + 1, 0), n - 1);
    const float dx = x - ((float)idx[0] + 0.5f);
    w[0] = 1.f - dx; w[1] = dx;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) idx[k] = min(max(b - 1 + k, 0), n - 1);
  const float t = x - ((float)idx[1] + 0.5f);
  const float t2 = t * t, t3 = t2 * t;
  w[0] = -0.5f * t3 + t2 - 0.5f * t;
  w[1] = 1.5f * t3 - 2.5f * t2 + 1.f;
  w[2] = -1.5f * t3 + 2.f * t2 + 0.5f * t;
  w[3] = 0.5f * t3 - 0.5f * t2;
}

// the derivatives of g2p_axis's weights in x, from the indices g2p_axis returned for the same x (flow.hip,
// libnfs_flow.so): the clipped index does not move with x, so d/dx = d/dt (cubic: t formed as above) or d/ddx (linear:
// constants; where both taps were clipped onto one cell the two terms cancel in the sum over the taps)
__device__ __forceinline__ void g2p_axis_d(float x, int cubic, const int* idx, float* dw) {
  if (!cubic) {
    dw[0] = -1.f; dw[1] = 1.f;
    return;
  }
  const float t = x - ((float)idx[1] + 0.5f);
  const float t2 = t * t;
  dw[0] = -1.5f * t2 + 2.f * t - 0.5f;
  dw[1] = 4.5f * t2 - 5.f * t;
  dw[2] = -4.5f * t2 + 4.f * t + 0.5f;
  dw[3] = 1.5f * t2 - t;
}

// the stencil of particle i: per axis d < nd the taps' cells ix[d][.] and weights wx[d][.]; an axis beyond nd is the one
// cell 0 with weight 1
__device__ __forceinline__ void g2p_stencil(const float* __restrict__ p, int64_t i, int nd, const int* n, int cubic,
                                            int (*ix)[4], float (*wx)[4]) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d < nd) {
      g2p_axis(p[i * nd + d] * (float)n[d], n[d], cubic, ix[d], wx[d]);
    } else {
      ix[d][0] = 0; wx[d][0] = 1.f;
    }
  }
}

// the sample of particle i from its stencil, four channels at a time, taps in the order axis 0 outermost, the weight of a
// tap formed as (w0 w1) w2: put(c, value) receives channel c
template <class F>
__device__ __forceinline__ void g2p_gather(const float* __restrict__ g, int nd, const int* n, int C, int cubic,
                                           const int (*ix)[4], const float (*wx)[4], F&& put) {
  const int taps = cubic ? 4 : 2;
  const int t2 = nd >= 3 ? taps : 1;
  for (int c0 = 0; c0 < C; c0 += 4) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int cn = min(4, C - c0);
    for (int ka = 0; ka < taps; ++ka)
      for (int kb = 0; kb < taps; ++kb) {
        const float wab = wx[0][ka] * wx[1][kb];
        const int64_t rowb = (int64_t)ix[0][ka] * n[1] + ix[1][kb];
        for (int kc = 0; kc < t2; ++kc) {
          const float w = wab * wx[2][kc];
          const float* gp = g + ((nd >= 3 ? rowb * n[2] + ix[2][kc] : rowb) * C + c0);
          for (int c = 0; c < cn; ++c) acc[c] += w * gp[c];
        }
      }
    for (int c = 0; c < cn; ++c) put(c0 + c, acc[c]);
  }
}

}  // namespace nfs
