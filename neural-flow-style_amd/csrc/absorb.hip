// libnfs_absorb.so (include/nfs_absorb.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and the other five libraries' alone.
// The derivative of a liquid colour render (include/nfs_liquid.h) with respect to the density it is seen through:
//   liquid_absorb_bwd_kernel   g_S[v,z] = tau (a w psi(tau S) - P - t b),  a = sum_c g_J[c] Q[z,c],  b = sum_c g_J[c] bg[c],
//                              P = sum_{z'' < z} a w,  S = rotate(d, R_v) and Q = rotate(q, R_v) gathered on the fly
// The twin of liquid_weights_kernel: one lane per ray, a wave on 64 consecutive x of one (view, row), but NEAR end first
// (z = 0 upwards: what lies in front of a sample is what its weight is seen through), P in a register.  One stencil per
// sample (ray_sample_pairs / ray_sample_scalar of ray_gather.h, which exposure.hip takes without the density; ray_coords,
// axis_setup) gathers the sample of d and the C channels of q: as x-pairs where W >= 2 (an 8-byte load
// of d and one load of 2 C floats of q per (z, y) corner pair; four samples' gathers issued before any is consumed), and
// through tri_setup and scalar loads where W == 1.  The only [V,D,H,W] traffic is w read and g_s written (a z step of a wave
// moves 256 contiguous bytes each way); nothing of size [V,D,H,W,C] exists.  No LDS, no atomics.  g_s may be the buffer w
// itself: a lane reads w[z] before it writes g_s[z], and no other lane touches that ray.
// psi(x) = phi'(x) / phi(x) = 1 / (e^x - 1) - 1 / x for x >= 0, psi(0) = -1/2, |psi| <= 1/2, -> -1 / x.  Three branches:
//   x < 1:    the series -1/2 + x/12 - x^3/720 + x^5/30240 - x^7/1209600 (Bernoulli numbers; alternating with decreasing
//             terms for 0 <= x < 1, so the truncation is below the next term x^9/47900160 < 2.1e-8: a third of 2^-24), in
//             Horner form in x^2: four roundings against values below 1/12 and the last sum against 1/2, under 2 x 2^-24
//             absolute;
//   x < 32:   1 / expm1(x) - 1 / x, where the two quotients are at most 0.59 and 1, so what the subtraction cancels is
//             bounded: expm1 within 2 ulp and its quotient's rounding (5 x 2^-24 x 0.59), the second quotient's rounding
//             (2^-24) and the difference's (2^-25): under 4.5 x 2^-24 absolute (psi <= -0.41 there: a few ulp);
//   x >= 32:  -1 / x; what is left out, 1 / (e^x - 1) < 1.3e-14, is below 2^-24 |psi| by five orders, and e^x is never
//             formed, so it cannot overflow.  psi is finite for every x >= 0.
// A negative x (a caller's own negative density) takes the series for -1 < x < 0, where it still converges (|x| < 2 pi), and
// the quotient below that; the bounds of tests/absorb_ref.py are stated for x >= 0 only.
// A sample of -0.0 counts as 0 (s + 0.f, as in the forward kernel).  A ray with t = 0 (flushed by the forward kernel) or
// w = 0 only multiplies by them.  A NaN sample makes g_s NaN on ITS ray (from where the forward kernel's weights are NaN
// on) and touches no other ray.
// Every index: V * D * H * W < 2^30 (checked), so ray and sample indices are ints and offsets into q (times C <= 4) are
// 64-bit; axis_setup clamps every corner into the volume whatever the matrix is (also for NaN coordinates), and a pair load
// reads x = min(i0, W - 2) and its neighbour.
#include "common.h"
#include "ray_gather.h"
#include "../../include/nfs_absorb.h"

namespace nfs {

constexpr float PSI_SERIES_BELOW = 1.f;              // see above
constexpr float PSI_TAIL_FROM = 32.f;

__device__ __forceinline__ float liquid_psi(float x) {
  if (fabsf(x) < PSI_SERIES_BELOW) {
    const float x2 = x * x;
    return -0.5f + x * (1.f / 12.f - x2 * (1.f / 720.f - x2 * (1.f / 30240.f - x2 * (1.f / 1209600.f))));
  }
  if (x >= PSI_TAIL_FROM) return -1.f / x;
  return 1.f / expm1f(x) - 1.f / x;
}

// (w and g_s carry no __restrict__: they may be one buffer)
template <int C>
__global__ void __launch_bounds__(256) liquid_absorb_bwd_kernel(const float* __restrict__ g_img, const float* __restrict__ q,
                                                                const float* __restrict__ d, const float* __restrict__ rot,
                                                                const float* w, const float* __restrict__ t_total,
                                                                const float* __restrict__ bg, float* g_s, int V, int D,
                                                                int H, int W, float tau) {
  const int HW = H * W;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= V * HW) return;
  const int v = gid / HW, px = gid - v * HW, h = px / W, x = px - h * W;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = rot[v * 9 + i];
  float g[C], b = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    g[c] = g_img[(int64_t)gid * C + c];
    b += g[c] * bg[c];
  }
  const float tb = t_total[gid] * b;
  const int64_t col = (int64_t)v * D * HW + px;
  const float* wcol = w + col;
  float* gcol = g_s + col;
  float P = 0.f;                                       // sum of a w over the samples in front of the one at hand
  // one sample: its gradient from the sum so far, then a w into the sum (s + 0.f: a -0.0 sample counts as +0)
#define NFS_ABSORB_TAKE(s, a, wz, z)                                                     \
  do {                                                                                   \
    const float aw = (a) * (wz);                                                         \
    gcol[(int64_t)(z) * HW] = tau * (aw * liquid_psi(tau * ((s) + 0.f)) - P - tb);      \
    P += aw;                                                                             \
  } while (0)
  if (W >= 2) {
    int z = 0;
    for (; z + 3 < D; z += 4) {
      float sv[4], av[4], wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        wv[u] = wcol[(int64_t)(z + u) * HW];
        ray_sample_pairs<C, true>(d, q, r, g, D, H, W, z + u, h, x, sv[u], av[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) NFS_ABSORB_TAKE(sv[u], av[u], wv[u], z + u);
    }
    for (; z < D; ++z) {
      float sone, aone;
      const float wone = wcol[(int64_t)z * HW];
      ray_sample_pairs<C, true>(d, q, r, g, D, H, W, z, h, x, sone, aone);
      NFS_ABSORB_TAKE(sone, aone, wone, z);
    }
  } else {
    for (int z = 0; z < D; ++z) {
      float sone, aone;
      const float wone = wcol[(int64_t)z * HW];
      ray_sample_scalar<C, true>(d, q, r, g, D, H, W, z, h, x, sone, aone);
      NFS_ABSORB_TAKE(sone, aone, wone, z);
    }
  }
#undef NFS_ABSORB_TAKE
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_absorb_version(void) { return NFS_ABSORB_ABI_VERSION; }

int nfs_liquid_absorb_bwd(const float* g_img, const float* q, const float* d, const float* rot, const float* w,
                          const float* t_total, const float* bg, float tau, float* g_s, int V, int D, int H, int W, int C,
                          nfs_stream_t stream) {
  NFS_REQUIRE(g_img && q && d && rot && w && t_total && bg && g_s, "nfs_liquid_absorb_bwd: null pointer");
  NFS_REQUIRE(V >= 1 && D >= 1 && H >= 1 && W >= 1,
              "nfs_liquid_absorb_bwd: V, D, H and W must be at least 1 (got %d, %d x %d x %d)", V, D, H, W);
  NFS_REQUIRE(C >= 1 && C <= 4, "nfs_liquid_absorb_bwd: C must be 1..4 (got %d)", C);
  NFS_REQUIRE((int64_t)V * D * H * W < ((int64_t)1 << 30), "nfs_liquid_absorb_bwd: V * D * H * W must be below 2^30");
  const int64_t nd = (int64_t)D * H * W, nw = (int64_t)V * nd, nimg = (int64_t)V * H * W, nrot = (int64_t)V * 9;
  NFS_REQUIRE(!overlaps(g_s, nw, g_img, nimg * C) && !overlaps(g_s, nw, q, nd * C) && !overlaps(g_s, nw, d, nd) &&
                  !overlaps(g_s, nw, rot, nrot) && !overlaps(g_s, nw, t_total, nimg) && !overlaps(g_s, nw, bg, C),
              "nfs_liquid_absorb_bwd: g_s must not alias g_img, q, d, rot, t_total or bg");
  NFS_REQUIRE((const float*)g_s == w || !overlaps(g_s, nw, w, nw),
              "nfs_liquid_absorb_bwd: g_s may be w itself, but must not overlap it otherwise");
  const dim3 grid(blocks_for(nimg, 256)), block(256);
  hipStream_t s = as_stream(stream);
#define NFS_ABSORB_LAUNCH(CC)                                                                                          \
  hipLaunchKernelGGL(liquid_absorb_bwd_kernel<CC>, grid, block, 0, s, g_img, q, d, rot, w, t_total, bg, g_s, V, D, H, W, tau)
  switch (C) {
    case 1: NFS_ABSORB_LAUNCH(1); break;
    case 2: NFS_ABSORB_LAUNCH(2); break;
    case 3: NFS_ABSORB_LAUNCH(3); break;
    default: NFS_ABSORB_LAUNCH(4); break;
  }
#undef NFS_ABSORB_LAUNCH
  return check_launch("nfs_liquid_absorb_bwd");
}

}  // extern "C"
