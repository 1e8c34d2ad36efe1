// libnfs_colour.so (include/nfs_colour.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and the other two libraries' alone.
// Emission-absorption rendering of a colour volume q [D,H,W,C] through V views whose absorption is a grey density:
//   ray_weights_kernel          w = T / M from the rotated grey samples: one lane per ray, far end first
//   colour_project_fwd_kernel   img[v,y,x,:] = sum_z w[v,z,y,x] trilinear(q; R_v x): one lane per ray, C accumulators
//   colour_project_bwd_kernel   the transpose: one lane per sample, 8 C global float atomic adds
// Sample coordinates and the stencil are nfs_rotate_fwd's (ray_coords, tri_setup: common.h).
// Layout: a wave's lanes on 64 consecutive x of one (view, row): every z step reads 256 contiguous bytes of w, the
// gathers of q are near-coalesced for small rotations, and the atomics of a wave land on runs of C * 64 floats.
// Bytes: weights 8 V D H W; forward 4 V D H W (w) + the gathers of q (C * 4 D H W when they hit in cache) + 4 C V H W;
// transpose 4 V D H W + 4 C V H W read and 8 * C * 4 B of atomic adds per sample with a non-zero product: measured at
// 0.24 TB/s of added bytes (25.6 ms at 200^3 x 8 views, C = 3), so ops.colour_project_bwd takes the scatter only where the
// launch count decides (up to 2^19 samples) and the output-stationary rotate adjoint per channel above.
// Every index: V * D * H * W < 2^30 (checked), so sample and ray indices are ints; offsets into q / g_q (times C <= 4)
// are 64-bit.  tri_setup clamps every corner into the volume whatever the matrix is.
#include "common.h"
#include "../../include/nfs_colour.h"

namespace nfs {

__global__ void __launch_bounds__(256) ray_weights_kernel(const float* d_rot, const float* __restrict__ gmax, float* w,
                                                          int V, int D, int HW, int per_group, float tau) {
  const float ntau = exp2_rate(tau);
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= V * HW) return;
  const int v = gid / HW, px = gid - v * HW;
  const float m = gmax[v / per_group];
  const int64_t base = (int64_t)v * D * HW + px;
  float acc = 0.f;
#pragma unroll 4
  for (int z = D - 1; z >= 0; --z) {
    const int64_t o = base + (int64_t)z * HW;
    acc += d_rot[o];                                   // (read before the write below: w may alias d_rot)
    w[o] = __builtin_amdgcn_exp2f(acc * ntau) / m;
  }
}

template <int C>
__global__ void __launch_bounds__(256) colour_project_fwd_kernel(const float* __restrict__ q, const float* __restrict__ rot,
                                                                 const float* __restrict__ w, float* __restrict__ img,
                                                                 int V, int D, int H, int W) {
  const int HW = H * W;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= V * HW) return;
  const int v = gid / HW, px = gid - v * HW, h = px / W, x = px - h * W;
  float r[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) r[i] = rot[v * 9 + i];
  const float* wcol = w + (int64_t)v * D * HW + px;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int z = D - 1; z >= 0; --z) {
    const float wz = wcol[(int64_t)z * HW];
    float cx, cy, cz;
    ray_coords(r, D, H, W, z, h, x, cx, cy, cz);
    Tri t; Axis ax, ay, az;
    tri_setup(cx, cy, cz, D, H, W, t, ax, ay, az);
    float s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float* p = q + t.o[k] * C;
#pragma unroll
      for (int c = 0; c < C; ++c) s[c] += t.w[k] * p[c];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(wz, s[c], acc[c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) img[(int64_t)gid * C + c] = acc[c];
}

template <int C>
__global__ void __launch_bounds__(256) colour_project_bwd_kernel(const float* __restrict__ g_img,
                                                                 const float* __restrict__ rot, const float* __restrict__ w,
                                                                 float* __restrict__ g_q, int V, int D, int H, int W) {
  const int HW = H * W, n = D * HW;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= V * n) return;
  const int v = gid / n, vox = gid - v * n, z = vox / HW, px = vox - z * HW, h = px / W, x = px - h * W;
  const float wz = w[gid];
  if (wz == 0.f) return;
  float g[C];
  bool any = false;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    g[c] = wz * g_img[((int64_t)v * HW + px) * C + c];
    any |= g[c] != 0.f;
  }
  if (!any) return;
  float cx, cy, cz;
  ray_coords(rot + v * 9, D, H, W, z, h, x, cx, cy, cz);
  Tri t; Axis ax, ay, az;
  tri_setup(cx, cy, cz, D, H, W, t, ax, ay, az);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (t.w[k] == 0.f) continue;                       // (the upper corners of a clamped or on-lattice sample)
    float* p = g_q + t.o[k] * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float contrib = t.w[k] * g[c];
      if (contrib != 0.f) atomicAdd(p + c, contrib);
    }
  }
}

static int check_colour_dims(const char* who, int V, int D, int H, int W) {
  NFS_REQUIRE(V >= 1 && D >= 1 && H >= 1 && W >= 1, "%s: V, D, H and W must be at least 1 (got %d, %d x %d x %d)", who, V, D,
              H, W);
  NFS_REQUIRE((int64_t)V * D * H * W < ((int64_t)1 << 30), "%s: V * D * H * W must be below 2^30", who);
  return NFS_OK;
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_colour_version(void) { return NFS_COLOUR_ABI_VERSION; }

int nfs_ray_weights(const float* d_rot, float tau, const float* gmax, int G, float* w, int V, int D, int H, int W,
                    nfs_stream_t stream) {
  NFS_REQUIRE(d_rot && gmax && w, "nfs_ray_weights: null pointer");
  if (int e = check_colour_dims("nfs_ray_weights", V, D, H, W)) return e;
  NFS_REQUIRE(G >= 1 && G <= V && V % G == 0, "nfs_ray_weights: G must divide V (got G = %d, V = %d)", G, V);
  NFS_REQUIRE((const float*)w != gmax && d_rot != gmax, "nfs_ray_weights: gmax must not alias d_rot or w");
  hipLaunchKernelGGL(ray_weights_kernel, dim3(blocks_for((int64_t)V * H * W, 256)), dim3(256), 0, as_stream(stream), d_rot,
                     gmax, w, V, D, H * W, V / G, tau);
  return check_launch("nfs_ray_weights");
}

int nfs_colour_project_fwd(const float* q, const float* rot, const float* w, float* img, int V, int D, int H, int W, int C,
                           nfs_stream_t stream) {
  NFS_REQUIRE(q && rot && w && img, "nfs_colour_project_fwd: null pointer");
  if (int e = check_colour_dims("nfs_colour_project_fwd", V, D, H, W)) return e;
  NFS_REQUIRE(C >= 1 && C <= 4, "nfs_colour_project_fwd: C must be 1..4 (got %d)", C);
  NFS_REQUIRE((const float*)img != q && (const float*)img != w && (const float*)img != rot,
              "nfs_colour_project_fwd: img must not alias q, w or rot");
  const dim3 grid(blocks_for((int64_t)V * H * W, 256)), block(256);
  hipStream_t s = as_stream(stream);
  switch (C) {
    case 1: hipLaunchKernelGGL(colour_project_fwd_kernel<1>, grid, block, 0, s, q, rot, w, img, V, D, H, W); break;
    case 2: hipLaunchKernelGGL(colour_project_fwd_kernel<2>, grid, block, 0, s, q, rot, w, img, V, D, H, W); break;
    case 3: hipLaunchKernelGGL(colour_project_fwd_kernel<3>, grid, block, 0, s, q, rot, w, img, V, D, H, W); break;
    default: hipLaunchKernelGGL(colour_project_fwd_kernel<4>, grid, block, 0, s, q, rot, w, img, V, D, H, W); break;
  }
  return check_launch("nfs_colour_project_fwd");
}

int nfs_colour_project_bwd(const float* g_img, const float* rot, const float* w, float* g_q, int overwrite, int V, int D,
                           int H, int W, int C, nfs_stream_t stream) {
  NFS_REQUIRE(g_img && rot && w && g_q, "nfs_colour_project_bwd: null pointer");
  if (int e = check_colour_dims("nfs_colour_project_bwd", V, D, H, W)) return e;
  NFS_REQUIRE(C >= 1 && C <= 4, "nfs_colour_project_bwd: C must be 1..4 (got %d)", C);
  NFS_REQUIRE((const float*)g_q != g_img && (const float*)g_q != w && (const float*)g_q != rot,
              "nfs_colour_project_bwd: g_q must not alias g_img, w or rot");
  hipStream_t s = as_stream(stream);
  if (overwrite) zero_words(g_q, (long long)D * H * W * C, s);          // (a kernel, not a memset node: common.h)
  const dim3 grid(blocks_for((int64_t)V * D * H * W, 256)), block(256);
  switch (C) {
    case 1: hipLaunchKernelGGL(colour_project_bwd_kernel<1>, grid, block, 0, s, g_img, rot, w, g_q, V, D, H, W); break;
    case 2: hipLaunchKernelGGL(colour_project_bwd_kernel<2>, grid, block, 0, s, g_img, rot, w, g_q, V, D, H, W); break;
    case 3: hipLaunchKernelGGL(colour_project_bwd_kernel<3>, grid, block, 0, s, g_img, rot, w, g_q, V, D, H, W); break;
    default: hipLaunchKernelGGL(colour_project_bwd_kernel<4>, grid, block, 0, s, g_img, rot, w, g_q, V, D, H, W); break;
  }
  return check_launch("nfs_colour_project_bwd");
}

}  // extern "C"
