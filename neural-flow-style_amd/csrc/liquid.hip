// libnfs_liquid.so (include/nfs_liquid.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and the other four libraries' alone.
// The ray weights of a liquid colour render (front-to-back alpha compositing over a background):
//   liquid_weights_kernel   w[v,z] = tau exp(-tau B) phi(tau S),  B = sum_{z' > z} S,  S = rotate(d, R_v) gathered on the fly;
//                           t_total = exp(-tau sum_z S), grey = 1 - t_total per ray
// One lane per ray, a wave on 64 consecutive x of one (view, row), far end first.  Unlike the smoke weights (rotate + render,
// the maximum of the grey image, then T / M: three passes over [V,D,H,W]) nothing here needs a global maximum, so one pass
// forms them: the only [V,D,H,W] traffic is the 4 V D H W bytes of w written (a z step of a wave writes 256 contiguous
// bytes); d is gathered as nfs_rotate_render_fwd gathers it (x-pairs from 8-byte loads, four samples in flight before the
// serial sum consumes them) and stays in cache for small rotations; a volume one cell wide (W == 1) has no pair to load and
// takes tri_setup -- the same three axis_setup calls -- and eight scalar loads.  No LDS, no atomics.
// phi(x) = (1 - exp(-x)) / x for x >= 0.  For 0 <= x < 2^-5 the series 1 - x/2 + x^2/6 - x^3/24 (alternating with
// decreasing terms BECAUSE x >= 0, so the truncation is below the next term x^4/120 <= 2^-20 / 120 < 2^-26.9: under a sixth
// of an ulp of phi ~ 1); from there on -expm1(-x) / x, whose numerator is relatively accurate (no 1 - exp cancellation) --
// either branch is within a few ulp for every x >= 0.  x = tau S is never negative where the weights are used: S is sampled
// with non-negative trilinear weights from a volume that nfs_smooth3d_relu_fwd cut at 0, and tau > 0.  A negative x (a
// caller's own negative density) still takes a defined branch -- for -2^-5 < x < 0 the series, all of whose terms are then
// positive, so its truncation is below x^4/120 (1 + |x|/6 + ...) < 2^-26.8, no worse -- but the bounds of
// tests/colour_liquid_ref.py are stated for x >= 0 only.  The transmittance exp(-tau B) goes through exp2_rate and the
// hardware exp2, as ray_weights_kernel's does.
// Every index: V * D * H * W < 2^30 (checked), so ray and sample indices are ints; axis_setup clamps every corner into the
// volume whatever the matrix is (also for NaN coordinates), and the pair load reads x = min(i0, W - 2) and its neighbour.
#include "common.h"
#include "../../include/nfs_liquid.h"

namespace nfs {

constexpr float PHI_SERIES_BELOW = 0.03125f;        // 2^-5: see above

// (x >= 0 in use; fabsf keeps a small negative x off the quotient's branch: see above)
__device__ __forceinline__ float liquid_phi(float x) {
  if (fabsf(x) < PHI_SERIES_BELOW) return 1.f - x * (0.5f - x * (1.f / 6.f - x * (1.f / 24.f)));
  return -expm1f(-x) / x;
}

__global__ void __launch_bounds__(256) liquid_weights_kernel(const float* __restrict__ d, const float* __restrict__ rot,
                                                             float* __restrict__ wout, float* __restrict__ grey,
                                                             float* __restrict__ t_total, int V, int D, int H, int W,
                                                             float tau) {
  const int HW = H * W;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= V * HW) return;
  const int v = gid / HW, px = gid - v * HW, h = px / W, x = px - h * W;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = rot[v * 9 + i];
  const float ntau = exp2_rate(tau);
  float* wcol = wout + (int64_t)v * D * HW + px;
  float acc = 0.f;                                     // B: the sum of the samples behind the one at hand
  // one sample: its weight from the sum so far, then into the sum (s + 0.f: a -0.0 sample counts as +0)
#define NFS_LIQUID_TAKE(s, z)                                                            \
  do {                                                                                   \
    const float s0 = (s) + 0.f;                                                          \
    wcol[(int64_t)(z) * HW] = tau * __builtin_amdgcn_exp2f(acc * ntau) * liquid_phi(tau * s0); \
    acc += s0;                                                                           \
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
      for (int u = 0; u < 4; ++u) NFS_LIQUID_TAKE(sv[u], z - u);
    }
    for (; z >= 0; --z) {
      float cx, cy, cz;
      ray_coords(r, D, H, W, z, h, x, cx, cy, cz);
      const Axis az = axis_setup(cx, D), ay = axis_setup(cy, H), ax = axis_setup(cz, W);
      const float sone = tri_sample_pairs(d, H, W, az, ay, ax);
      NFS_LIQUID_TAKE(sone, z);
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
      NFS_LIQUID_TAKE(sone, z);
    }
  }
#undef NFS_LIQUID_TAKE
  const float t = __builtin_amdgcn_exp2f(acc * ntau);
  if (t_total) t_total[gid] = t;
  if (grey) grey[gid] = 1.f - t;
}

// do [a, a + na) and [b, b + nb) floats share an address?  (a null range shares none)
static bool overlaps(const float* a, int64_t na, const float* b, int64_t nb) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, a1 = a0 + (uintptr_t)na * 4, b0 = (uintptr_t)b, b1 = b0 + (uintptr_t)nb * 4;
  return a0 < b1 && b0 < a1;
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_liquid_version(void) { return NFS_LIQUID_ABI_VERSION; }

int nfs_liquid_weights(const float* d, const float* rot, float tau, float* w, float* grey, float* t_total, int V, int D,
                       int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(d && rot && w, "nfs_liquid_weights: null pointer (d, rot and w are required; grey and t_total may be null)");
  NFS_REQUIRE(V >= 1 && D >= 1 && H >= 1 && W >= 1,
              "nfs_liquid_weights: V, D, H and W must be at least 1 (got %d, %d x %d x %d)", V, D, H, W);
  NFS_REQUIRE((int64_t)V * D * H * W < ((int64_t)1 << 30), "nfs_liquid_weights: V * D * H * W must be below 2^30");
  const int64_t nd = (int64_t)D * H * W, nw = (int64_t)V * nd, nimg = (int64_t)V * H * W, nrot = (int64_t)V * 9;
  NFS_REQUIRE(!overlaps(w, nw, d, nd) && !overlaps(w, nw, rot, nrot), "nfs_liquid_weights: w must not alias d or rot");
  NFS_REQUIRE(!overlaps(grey, nimg, d, nd) && !overlaps(grey, nimg, rot, nrot),
              "nfs_liquid_weights: grey must not alias d or rot");
  NFS_REQUIRE(!overlaps(t_total, nimg, d, nd) && !overlaps(t_total, nimg, rot, nrot),
              "nfs_liquid_weights: t_total must not alias d or rot");
  NFS_REQUIRE(!overlaps(grey, nimg, w, nw) && !overlaps(t_total, nimg, w, nw) && !overlaps(grey, nimg, t_total, nimg),
              "nfs_liquid_weights: w, grey and t_total must not alias one another");
  hipLaunchKernelGGL(liquid_weights_kernel, dim3(blocks_for(nimg, 256)), dim3(256), 0, as_stream(stream), d, rot, w, grey,
                     t_total, V, D, H, W, tau);
  return check_launch("nfs_liquid_weights");
}

}  // extern "C"
