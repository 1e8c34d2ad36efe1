// libnfs_exposure.so (include/nfs_exposure.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and the other six libraries' alone.
// The smoke colour render at a fixed exposure -- emission-absorption with NO maximum of the grey image -- and its derivative
// in the density it is seen through:
//   exposure_weights_kernel      w[v,z] = kappa tau exp(-tau sum_{z' >= z} S),  grey = sum_z w S,  S = rotate(d, R_v)
//                                gathered on the fly
//   exposure_absorb_bwd_kernel   g_S[v,z] = -tau sum_{z' <= z} a w,  a = sum_c g_J[c] Q[z,c],  Q = rotate(q, R_v) gathered on
//                                the fly
// Both: one lane per ray, a wave on 64 consecutive x of one (view, row); no LDS, no atomics, no scratch.
// The weights are the twin of liquid_weights_kernel (liquid.hip): far end first, the running sum in a register, d gathered
// as nfs_rotate_render_fwd gathers it (x-pairs from 8-byte loads, four samples in flight before the serial sum consumes
// them; tri_setup and eight scalar loads where W == 1).  The sum is INCLUSIVE (the sample is added before its weight is
// formed: nfs_render_fwd's transmittance, ray_weights_kernel's numerator), and the transmittance goes through exp2_rate and
// the hardware exp2 as theirs does.  The only [V,D,H,W] traffic is the 4 V D H W bytes of w written: the smoke render's
// route to its weights (rotate + render with the samples kept, the maximum, T / M in place) writes them twice and reads them
// once.
// The adjoint is the twin of liquid_absorb_bwd_kernel (absorb.hip) without everything that needed the density: NEAR end
// first (z = 0 upwards: a sample dims every weight at or in front of it), the prefix in a register, one stencil per sample
// for the C channels of q (ray_gather.h, the gather absorb.hip takes with the density), four samples' gathers issued before
// any is consumed.  The only [V,D,H,W] traffic is w read and g_s written; g_s may be the buffer w itself: a lane reads w[z]
// before it writes g_s[z], and no other lane touches that ray.
// A sample of -0.0 counts as 0 (s + 0.f).  A NaN sample makes w and grey NaN on ITS ray from that sample towards the viewer
// and touches no other ray; a NaN in q or w does the same to g_s from that sample away from the viewer.
// Every index: V * D * H * W < 2^30 (checked), so ray and sample indices are ints and offsets into q (times C <= 4) are
// 64-bit; axis_setup clamps every corner into the volume whatever the matrix is (also for NaN coordinates), and a pair load
// reads x = min(i0, W - 2) and its neighbour.
#include "common.h"
#include "ray_gather.h"
#include "../../include/nfs_exposure.h"

#include <math.h>

namespace nfs {

__global__ void __launch_bounds__(256) exposure_weights_kernel(const float* __restrict__ d, const float* __restrict__ rot,
                                                               float* __restrict__ wout, float* __restrict__ grey, int V,
                                                               int D, int H, int W, float tau, float gain) {
  const int HW = H * W;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= V * HW) return;
  const int v = gid / HW, px = gid - v * HW, h = px / W, x = px - h * W;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = rot[v * 9 + i];
  const float ntau = exp2_rate(tau), kt = gain * tau;
  float* wcol = wout + (int64_t)v * D * HW + px;
  float acc = 0.f, gsum = 0.f;                         // the sum of the samples from the far end up to the one at hand
  // one sample: into the sum, then its weight from the sum (s + 0.f: a -0.0 sample counts as +0)
#define NFS_EXPOSURE_TAKE(s, z)                                      \
  do {                                                               \
    const float s0 = (s) + 0.f;                                      \
    acc += s0;                                                       \
    const float wz = kt * __builtin_amdgcn_exp2f(acc * ntau);        \
    wcol[(int64_t)(z) * HW] = wz;                                    \
    gsum += wz * s0;                                                 \
  } while (0)
  if (W >= 2) {
    int z = D - 1;
    for (; z >= 3; z -= 4) {
      float sv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float cx, cy, cz;
        ray_coords(r, D, H, W, z - u, h, x, cx, cy, cz);
        const Axis az = axis_setup(cx, D), ay = axis_setup(cy, H), ax = axis_setup(cz, W);
        sv[u] = tri_sample_pairs(d, H, W, az, ay, ax);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) NFS_EXPOSURE_TAKE(sv[u], z - u);
    }
    for (; z >= 0; --z) {
      float cx, cy, cz;
      ray_coords(r, D, H, W, z, h, x, cx, cy, cz);
      const Axis az = axis_setup(cx, D), ay = axis_setup(cy, H), ax = axis_setup(cz, W);
      const float sone = tri_sample_pairs(d, H, W, az, ay, ax);
      NFS_EXPOSURE_TAKE(sone, z);
    }
  } else {
    for (int z = D - 1; z >= 0; --z) {
      float cx, cy, cz;
      ray_coords(r, D, H, W, z, h, x, cx, cy, cz);
      Tri t; Axis ax, ay, az;
      tri_setup(cx, cy, cz, D, H, W, t, ax, ay, az);
      float sone = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) sone += t.w[k] * d[t.o[k]];
      NFS_EXPOSURE_TAKE(sone, z);
    }
  }
#undef NFS_EXPOSURE_TAKE
  if (grey) grey[gid] = gsum;
}

// (w and g_s carry no __restrict__: they may be one buffer)
// Two waves per SIMD for C <= 3, asked for by name.  Left to itself the compiler fits the loop into 124 VGPRs (C = 3) to
// keep four waves, and does so by waiting for each corner pair's loads before it issues the next: two loads in flight where
// the source has the gathers of four samples, and 659 us at 200^3 x 8 views where liquid_absorb_bwd_kernel, which gathers
// one volume MORE, takes 604 (its 214 VGPRs leave the scheduler nothing to save, and it keeps 50 loads in flight).  With the
// target stated the four samples' 32 loads are issued before the first is consumed (161 / 178 / 222 VGPRs for C = 1 / 2 / 3,
// no scratch).  C = 4 under the same target spills 7 registers, so it stays as the compiler has it (144 VGPRs).
template <int C>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(C <= 3 ? 2 : 1, C <= 3 ? 2 : 8)))
exposure_absorb_bwd_kernel(const float* __restrict__ g_img, const float* __restrict__ q, const float* __restrict__ rot,
                           const float* w, float* g_s, int V, int D, int H, int W, float tau) {
  const int HW = H * W;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= V * HW) return;
  const int v = gid / HW, px = gid - v * HW, h = px / W, x = px - h * W;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = rot[v * 9 + i];
  float g[C];
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = g_img[(int64_t)gid * C + c];
  const int64_t col = (int64_t)v * D * HW + px;
  const float* wcol = w + col;
  float* gcol = g_s + col;
  const float mtau = -tau;
  float P = 0.f;                                       // sum of a w over the samples in front of and at the one at hand
  float unused;
  if (W >= 2) {
    int z = 0;
    for (; z + 3 < D; z += 4) {
      float av[4], wv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        wv[u] = wcol[(int64_t)(z + u) * HW];
        ray_sample_pairs<C, false>(nullptr, q, r, g, D, H, W, z + u, h, x, unused, av[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        P += av[u] * wv[u];
        gcol[(int64_t)(z + u) * HW] = mtau * P;
      }
    }
    for (; z < D; ++z) {
      float aone;
      const float wone = wcol[(int64_t)z * HW];
      ray_sample_pairs<C, false>(nullptr, q, r, g, D, H, W, z, h, x, unused, aone);
      P += aone * wone;
      gcol[(int64_t)z * HW] = mtau * P;
    }
  } else {
    for (int z = 0; z < D; ++z) {
      float aone;
      const float wone = wcol[(int64_t)z * HW];
      ray_sample_scalar<C, false>(nullptr, q, r, g, D, H, W, z, h, x, unused, aone);
      P += aone * wone;
      gcol[(int64_t)z * HW] = mtau * P;
    }
  }
}

static bool finite_positive(float x) { return isfinite(x) && x > 0.f; }

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_exposure_version(void) { return NFS_EXPOSURE_ABI_VERSION; }

int nfs_exposure_weights(const float* d, const float* rot, float tau, float gain, float* w, float* grey, int V, int D, int H,
                         int W, nfs_stream_t stream) {
  NFS_REQUIRE(d && rot && w, "nfs_exposure_weights: null pointer (d, rot and w are required; grey may be null)");
  NFS_REQUIRE(V >= 1 && D >= 1 && H >= 1 && W >= 1,
              "nfs_exposure_weights: V, D, H and W must be at least 1 (got %d, %d x %d x %d)", V, D, H, W);
  NFS_REQUIRE((int64_t)V * D * H * W < ((int64_t)1 << 30), "nfs_exposure_weights: V * D * H * W must be below 2^30");
  NFS_REQUIRE(finite_positive(tau), "nfs_exposure_weights: tau must be finite and positive (got %g)", (double)tau);
  NFS_REQUIRE(finite_positive(gain), "nfs_exposure_weights: gain must be finite and positive (got %g)", (double)gain);
  const int64_t nd = (int64_t)D * H * W, nw = (int64_t)V * nd, nimg = (int64_t)V * H * W, nrot = (int64_t)V * 9;
  NFS_REQUIRE(!overlaps(w, nw, d, nd) && !overlaps(w, nw, rot, nrot), "nfs_exposure_weights: w must not alias d or rot");
  NFS_REQUIRE(!overlaps(grey, nimg, d, nd) && !overlaps(grey, nimg, rot, nrot) && !overlaps(grey, nimg, w, nw),
              "nfs_exposure_weights: grey must not alias d, rot or w");
  hipLaunchKernelGGL(exposure_weights_kernel, dim3(blocks_for(nimg, 256)), dim3(256), 0, as_stream(stream), d, rot, w, grey,
                     V, D, H, W, tau, gain);
  return check_launch("nfs_exposure_weights");
}

int nfs_exposure_absorb_bwd(const float* g_img, const float* q, const float* rot, const float* w, float tau, float* g_s,
                            int V, int D, int H, int W, int C, nfs_stream_t stream) {
  NFS_REQUIRE(g_img && q && rot && w && g_s, "nfs_exposure_absorb_bwd: null pointer");
  NFS_REQUIRE(V >= 1 && D >= 1 && H >= 1 && W >= 1,
              "nfs_exposure_absorb_bwd: V, D, H and W must be at least 1 (got %d, %d x %d x %d)", V, D, H, W);
  NFS_REQUIRE(C >= 1 && C <= 4, "nfs_exposure_absorb_bwd: C must be 1..4 (got %d)", C);
  NFS_REQUIRE((int64_t)V * D * H * W < ((int64_t)1 << 30), "nfs_exposure_absorb_bwd: V * D * H * W must be below 2^30");
  NFS_REQUIRE(finite_positive(tau), "nfs_exposure_absorb_bwd: tau must be finite and positive (got %g)", (double)tau);
  const int64_t nd = (int64_t)D * H * W, nw = (int64_t)V * nd, nimg = (int64_t)V * H * W, nrot = (int64_t)V * 9;
  NFS_REQUIRE(!overlaps(g_s, nw, g_img, nimg * C) && !overlaps(g_s, nw, q, nd * C) && !overlaps(g_s, nw, rot, nrot),
              "nfs_exposure_absorb_bwd: g_s must not alias g_img, q or rot");
  NFS_REQUIRE((const float*)g_s == w || !overlaps(g_s, nw, w, nw),
              "nfs_exposure_absorb_bwd: g_s may be w itself, but must not overlap it otherwise");
  const dim3 grid(blocks_for(nimg, 256)), block(256);
  hipStream_t s = as_stream(stream);
#define NFS_EXPOSURE_LAUNCH(CC)                                                                                         \
  hipLaunchKernelGGL(exposure_absorb_bwd_kernel<CC>, grid, block, 0, s, g_img, q, rot, w, g_s, V, D, H, W, tau)
  switch (C) {
    case 1: NFS_EXPOSURE_LAUNCH(1); break;
    case 2: NFS_EXPOSURE_LAUNCH(2); break;
    case 3: NFS_EXPOSURE_LAUNCH(3); break;
    default: NFS_EXPOSURE_LAUNCH(4); break;
  }
#undef NFS_EXPOSURE_LAUNCH
  return check_launch("nfs_exposure_absorb_bwd");
}

}  // extern "C"
