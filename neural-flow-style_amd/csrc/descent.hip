// libnfs_descent.so (include/nfs_descent.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and libnfs_grid2d.so's alone.
// The update of Laplacian-normalised descent (engine.LapDescentState): x <- fmaf(-lr, g, x) with g the normalised gradient,
// alone (descent_kernel) or, for a velocity variable, fused with the next iteration's forward advect:
//   advect_descent4_kernel    3-D, a multiple of 4 voxels: advect1_kernel's lane layout and lean stencil (advect_stencil.h)
//   advect_descent1_kernel    3-D, any other voxel count: the reference stencil, one voxel per lane
//   advect2d_descent_kernel   2-D: grid2d.hip's stencil, one pixel per lane
// HBM-bound streaming kernels: per voxel 12 B of g + 12 B of velocity in and out + the d0 gather + 4 B (+ 1/8 B of mask);
// no LDS, no atomics; the 12-byte vectors as dwordx3 accesses, a wave's lanes on consecutive voxels.  Every index is an
// int (D * H * W < 2^30) and comes out of lean_cell / axis2d, clamped into the grid whatever the velocity is.
#include "advect_stencil.h"
#include "../../include/nfs_descent.h"

namespace nfs {

// the one expression of the update: a fused multiply-add, one rounding
__device__ __forceinline__ float descent(float x, float g, float lr) { return fmaf(-lr, g, x); }
__device__ __forceinline__ F3u descent(const F3u& x, const F3u& g, float lr) {
  return F3u{descent(x.x, g.x, lr), descent(x.y, g.y, lr), descent(x.z, g.z, lr)};
}

// four consecutive floats per lane where the pointers allow (vec: both 16-byte aligned), the tail and the unaligned case
// one float per lane
__global__ void __launch_bounds__(256) descent_kernel(float* __restrict__ x, const float* __restrict__ g, int64_t n, float lr,
                                                      int vec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const int64_t n4 = n >> 2;
    if (i < n4) {
      float4 a = reinterpret_cast<float4*>(x)[i];
      const float4 b = reinterpret_cast<const float4*>(g)[i];
      a.x = descent(a.x, b.x, lr); a.y = descent(a.y, b.y, lr); a.z = descent(a.z, b.z, lr); a.w = descent(a.w, b.w, lr);
      reinterpret_cast<float4*>(x)[i] = a;
    } else if (i < n4 + (n & 3)) {
      const int64_t k = (n4 << 2) + (i - n4);
      x[k] = descent(x[k], g[k], lr);
    }
  } else if (i < n) {
    x[i] = descent(x[i], g[i], lr);
  }
}

// A wave owns 256 consecutive voxels, lane l takes l, l + 64, l + 128, l + 192 (advect1_kernel's layout, MODE 0): the new
// velocity is stored, then back-traced from registers.  n = D * H * W is a multiple of 4 (the launch path checks).
template <bool LIVE>
__global__ void __launch_bounds__(256) advect_descent4_kernel(const float* __restrict__ d, float* vel,
                                                              const float* __restrict__ g, float lr, float* __restrict__ out,
                                                              unsigned long long* __restrict__ live, int D, int H, int W) {
  const int n = D * H * W;
  const int lane = threadIdx.x & 63, first = lane_first<4, true>(blockDim.x, lane);
  if (first - lane >= n) return;
  F3u* v3 = reinterpret_cast<F3u*>(vel);
  const F3u* g3 = reinterpret_cast<const F3u*>(g);
  F3u vv[4], gg[4];
  bool ok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = first + 64 * j;
    ok[j] = idx < n;
    const int ic = ok[j] ? idx : n - 1;
    vv[j] = v3[ic];
    gg[j] = g3[ic];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    vv[j] = descent(vv[j], gg[j], lr);
    if (ok[j]) v3[first + 64 * j] = vv[j];
  }
  const LeanDims dm = lean_dims(D, H, W);
  int w, h, z;
  lane_start(first, n, H, W, w, h, z);
  F2u p[4][4];
  float wz[4], wy[4], wx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const LeanCell c = lean_cell(vv[j], z, h, w, dm);
    wz[j] = c.wz; wy[j] = c.wy; wx[j] = c.wx;
    lean_gather(d, c.o, dm, p[j]);
    walk64(w, h, z, W, H, D - 1);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (ok[j]) out[first + 64 * j] = lean_sample(p[j], wx[j], wy[j], wz[j]);
    if constexpr (LIVE) {
      const unsigned long long lv = __ballot(ok[j] && corners_differ(p[j]));
      if (lane == 0 && first + 64 * j < n) live[(first + 64 * j) >> 6] = lv;
    }
  }
}

// any voxel count: one voxel per lane on the reference stencil (what nfs_advect_fwd runs where the lean kernel does not apply)
__global__ void __launch_bounds__(256) advect_descent1_kernel(const float* __restrict__ d, float* vel,
                                                              const float* __restrict__ g, float lr, float* __restrict__ out,
                                                              int D, int H, int W) {
  const int vox = blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= D * H * W) return;
  const int w = vox % W, t = vox / W, h = t % H, z = t / H;
  const F3u v = descent(reinterpret_cast<const F3u*>(vel)[vox], reinterpret_cast<const F3u*>(g)[vox], lr);
  reinterpret_cast<F3u*>(vel)[vox] = v;
  out[vox] = advect3d_ref_sample(d, z, h, w, D, H, W, v);
}

__global__ void __launch_bounds__(256) advect2d_descent_kernel(const float* __restrict__ d, float* vel,
                                                               const float* __restrict__ g, float lr, float* __restrict__ out,
                                                               int H, int W) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  const int x = pix % W, y = pix / W;
  const F2u v0 = reinterpret_cast<const F2u*>(vel)[pix], gv = reinterpret_cast<const F2u*>(g)[pix];
  const F2u v = F2u{descent(v0.x, gv.x, lr), descent(v0.y, gv.y, lr)};
  reinterpret_cast<F2u*>(vel)[pix] = v;
  out[pix] = advect2d_sample(d, bilinear_setup(y, x, H, W, v.x, v.y));
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_descent_version(void) { return NFS_DESCENT_ABI_VERSION; }

int nfs_descent_step(float* x, const float* g, int64_t n, float lr, nfs_stream_t stream) {
  NFS_REQUIRE(x && g, "nfs_descent_step: null pointer");
  NFS_REQUIRE(x != g, "nfs_descent_step: g must not alias x");
  NFS_REQUIRE(n >= 0, "nfs_descent_step: n must not be negative (got %lld)", (long long)n);
  if (n == 0) return NFS_OK;
  const int vec = aligned16(x) && aligned16(g);
  const int64_t lanes = vec ? (n >> 2) + (n & 3) : n;
  NFS_REQUIRE(blocks_for(lanes, 256) == (lanes + 255) / 256, "nfs_descent_step: n = %lld is beyond one launch", (long long)n);
  hipLaunchKernelGGL(descent_kernel, dim3(blocks_for(lanes, 256)), dim3(256), 0, as_stream(stream), x, g, n, lr, vec);
  return check_launch("nfs_descent_step");
}

int nfs_advect_descent_fwd(const float* d0, float* vel, const float* g, float lr, float* adv_next,
                           unsigned long long* live_next, int D, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(d0 && vel && g && adv_next, "nfs_advect_descent_fwd: null pointer");
  NFS_REQUIRE(D >= 2 && H >= 2 && W >= 2, "nfs_advect_descent_fwd: D, H and W must be at least 2 (got %d x %d x %d)", D, H, W);
  const int64_t n = (int64_t)D * H * W;
  NFS_REQUIRE(n < ((int64_t)1 << 30), "nfs_advect_descent_fwd: D * H * W must be below 2^30");
  NFS_REQUIRE(adv_next != d0 && adv_next != vel && adv_next != g && g != vel && (const float*)vel != d0,
              "nfs_advect_descent_fwd: adv_next must not alias d0, vel or g, nor g or d0 vel");
  NFS_REQUIRE(!live_next || n % 4 == 0,
              "nfs_advect_descent_fwd: live_next needs a multiple of 4 voxels (as nfs_advect_fwd_live does)");
  if (n % 4 == 0) {
    // 256 threads x 4 voxels; whole rounds of the 8 XCDs (lane_first's order)
    const dim3 grid((blocks_for(n, 1024) + 7) / 8 * 8);
    if (live_next)
      hipLaunchKernelGGL(advect_descent4_kernel<true>, grid, dim3(256), 0, as_stream(stream), d0, vel, g, lr, adv_next,
                         live_next, D, H, W);
    else
      hipLaunchKernelGGL(advect_descent4_kernel<false>, grid, dim3(256), 0, as_stream(stream), d0, vel, g, lr, adv_next,
                         live_next, D, H, W);
  } else {
    hipLaunchKernelGGL(advect_descent1_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), d0, vel, g, lr,
                       adv_next, D, H, W);
  }
  return check_launch("nfs_advect_descent_fwd");
}

int nfs_advect2d_descent_fwd(const float* d0, float* vel, const float* g, float lr, float* adv_next, int H, int W,
                             nfs_stream_t stream) {
  NFS_REQUIRE(d0 && vel && g && adv_next, "nfs_advect2d_descent_fwd: null pointer");
  NFS_REQUIRE(H >= 2 && W >= 2, "nfs_advect2d_descent_fwd: H and W must be at least 2 (got %d x %d)", H, W);
  NFS_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), "nfs_advect2d_descent_fwd: H * W must be below 2^30");
  NFS_REQUIRE(adv_next != d0 && adv_next != vel && adv_next != g && g != vel && (const float*)vel != d0,
              "nfs_advect2d_descent_fwd: adv_next must not alias d0, vel or g, nor g or d0 vel");
  hipLaunchKernelGGL(advect2d_descent_kernel, dim3(blocks_for((int64_t)H * W, 256)), dim3(256), 0, as_stream(stream), d0,
                     vel, g, lr, adv_next, H, W);
  return check_launch("nfs_advect2d_descent_fwd");
}

}  // extern "C"
