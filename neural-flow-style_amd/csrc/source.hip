// The stand-alone operators of the variables a velocity can be a function of, and their fused updates (source_ops.h holds
// the per-voxel arithmetic, shared with advect1_kernel): curl of a stream function (transform.py:517-555) and
// gradient of a potential (transform.py:508-515), forward and adjoint; the stream / potential / Helmholtz updates.
// One thread per voxel; the adjoints are gathers (no atomics, deterministic).
#include "source_ops.h"
#include <type_traits>

namespace nfs {

// 2-D: s [H,W] -> [H,W,2]: u = ds/dy (axis 0), v = -ds/dx (axis 1).  3-D: s [D,H,W,3] -> [D,H,W,3]:
//   u = dw/dy - dv/dz, v = du/dz - dw/dx, w = dv/dx - du/dy   with x = axis W, y = axis H, z = axis D
// -- source_velocity<SRC_STREAM> with the channels reversed (zero along an axis of length 1).
__global__ void __launch_bounds__(256) curl_fwd_kernel(const float* __restrict__ s, float* __restrict__ out, int D, int H,
                                                       int W, int nd) {
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  if (nd == 2) {
    const FdEnd<true> ex(x, W), ey(y, H);
    const float p = s[vox];
    out[vox * 2] = ey.d(p, s[ey.other(vox, W)]);
    out[vox * 2 + 1] = ex.d(s[ex.other(vox, 1)], p);     // the ends exchanged: -ds/dx as a difference, not a negation
    return;
  }
  const F3u v = source_velocity<SRC_STREAM, true>(s, vox, z, y, x, D, H, W);
  reinterpret_cast<F3u*>(out)[vox] = F3u{v.z, v.y, v.x};
}

// adjoint: g_s = curl^T g, g in the reference's channel order
__global__ void __launch_bounds__(256) curl_bwd_kernel(const float* __restrict__ g, float* __restrict__ gs, int D, int H,
                                                       int W, int nd) {
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  if (nd == 2) {
    // u = +d/dy s, v = -d/dx s
    gs[vox] = fd_adj(g, x, W, y, H, 0, 2) - fd_adj(g, (int64_t)y * W, 1, x, W, 1, 2);
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) gs[vox * 3 + c] = source_adj<SRC_STREAM>(g, z, y, x, D, H, W, 2, 1, 0, c);
}

// p [D,H,W] -> [D,H,W,3] = (dx, dy, dz) with x = axis W, y = axis H, z = axis D (the reference's channel order; zero along
// an axis of length 1): source_velocity<SRC_POTENTIAL> with the channels reversed
__global__ void __launch_bounds__(256) grad_fwd_kernel(const float* __restrict__ p, float* __restrict__ out, int D, int H,
                                                       int W) {
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  const F3u v = source_velocity<SRC_POTENTIAL, true>(p, vox, z, y, x, D, H, W);
  out[vox * 3] = v.z;
  out[vox * 3 + 1] = v.y;
  out[vox * 3 + 2] = v.x;
}

__global__ void __launch_bounds__(256) grad_bwd_kernel(const float* __restrict__ g, float* __restrict__ gp, int D, int H,
                                                       int W) {
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  gp[vox] = source_adj<SRC_POTENTIAL>(g, z, y, x, D, H, W, 2, 1, 0, 0);
}

// ---- the updates: g_var = source_adj<SRC>(g_vel), consumed on the spot by TF ApplyAdam on the variable ----------------------
// g_vel [D,H,W,3] is a velocity gradient in advect's channel order.  A thread reads g_vel at its neighbours and its own
// variable, m, v only -- one vector of each (12 bytes, a float, a float4), lanes contiguous: in place.  g_var is never
// stored: per voxel 12 B of g_vel + 6 x the variable (s 84 B, phi 36 B, a 108 B) against 108, 44 and 152 B for the
// stand-alone adjoint(s) followed by nfs_adam_tf_step.  (adam_tf: source_ops.h)
template <int SRC>
__global__ void __launch_bounds__(256) source_bwd_adam_kernel(const float* __restrict__ g, float* __restrict__ var,
                                                              float* __restrict__ m, float* __restrict__ v, int D, int H,
                                                              int W, float lr_t, float b1, float b2, float eps) {
  typedef std::conditional_t<SRC == SRC_STREAM, F3u, std::conditional_t<SRC == SRC_POTENTIAL, float, float4>> Vec;
  constexpr int NCH = sizeof(Vec) / sizeof(float);
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  Vec xs = reinterpret_cast<const Vec*>(var)[vox], ms = reinterpret_cast<const Vec*>(m)[vox],
      us = reinterpret_cast<const Vec*>(v)[vox];
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  if constexpr (SRC == SRC_HELMHOLTZ) {   // the four calls this update has always been: as a loop its m and v change bits
    adam_tf(xs.x, ms.x, us.x, source_adj<SRC>(g, z, y, x, D, H, W, 0, 1, 2, 0), lr_t, b1, b2, eps);
    adam_tf(xs.y, ms.y, us.y, source_adj<SRC>(g, z, y, x, D, H, W, 0, 1, 2, 1), lr_t, b1, b2, eps);
    adam_tf(xs.z, ms.z, us.z, source_adj<SRC>(g, z, y, x, D, H, W, 0, 1, 2, 2), lr_t, b1, b2, eps);
    adam_tf(xs.w, ms.w, us.w, source_adj<SRC>(g, z, y, x, D, H, W, 0, 1, 2, 3), lr_t, b1, b2, eps);
  } else {
    float* xp = reinterpret_cast<float*>(&xs); float* mp = reinterpret_cast<float*>(&ms); float* up = reinterpret_cast<float*>(&us);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      adam_tf(xp[c], mp[c], up[c], source_adj<SRC>(g, z, y, x, D, H, W, 0, 1, 2, c), lr_t, b1, b2, eps);
  }
  reinterpret_cast<Vec*>(var)[vox] = xs;
  reinterpret_cast<Vec*>(m)[vox] = ms;
  reinterpret_cast<Vec*>(v)[vox] = us;
}

static int check_volume(const char* who, int D, int H, int W, int C) {
  NFS_REQUIRE(D > 0 && H > 0 && W > 0, "%s: non-positive dimension", who);
  NFS_REQUIRE((int64_t)D * H * W * C < (int64_t)1 << 40, "%s: tensor too large", who);
  return NFS_OK;
}

// the variable x is s [D,H,W,3], phi [D,H,W] or a [D,H,W,4] (16-byte vectors), m and v of its shape
static int bwd_adam_launch(const char* who, int src, const float* g_vel, float* x, float* m, float* v, int D, int H, int W,
                           float lr_t, float beta1, float beta2, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(g_vel && x && m && v, "%s: null pointer", who);
  NFS_REQUIRE(g_vel != x && g_vel != m && g_vel != v, "%s: g_vel must not alias %s, m or v (it is a gather)", who,
              source_name(src));
  NFS_REQUIRE(src != SRC_HELMHOLTZ || (aligned16(x) && aligned16(m) && aligned16(v)), "%s: a, m and v must be 16-byte aligned",
              who);
  if (int e = check_volume(who, D, H, W, src == SRC_STREAM ? 3 : 4)) return e;
  hipLaunchKernelGGL(src == SRC_STREAM ? source_bwd_adam_kernel<SRC_STREAM>
                     : src == SRC_POTENTIAL ? source_bwd_adam_kernel<SRC_POTENTIAL> : source_bwd_adam_kernel<SRC_HELMHOLTZ>,
                     dim3(blocks_for((int64_t)D * H * W, 256)), dim3(256), 0, as_stream(stream), g_vel, x, m, v, D, H, W,
                     lr_t, beta1, beta2, eps);
  return check_launch(who);
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_curl_fwd(const float* s, float* out, int D, int H, int W, int nd, nfs_stream_t stream) {
  NFS_REQUIRE(s && out, "nfs_curl_fwd: null pointer");
  NFS_REQUIRE((nd == 2 && D == 1) || nd == 3, "nfs_curl_fwd: nd must be 2 (then D == 1) or 3");
  if (int e = check_volume("nfs_curl_fwd", D, H, W, 1)) return e;
  hipLaunchKernelGGL(curl_fwd_kernel, dim3(blocks_for((int64_t)D * H * W, 256)), dim3(256), 0, as_stream(stream), s, out, D,
                     H, W, nd);
  return check_launch("nfs_curl_fwd");
}

int nfs_curl_bwd(const float* g_out, float* g_s, int D, int H, int W, int nd, nfs_stream_t stream) {
  NFS_REQUIRE(g_out && g_s, "nfs_curl_bwd: null pointer");
  NFS_REQUIRE((nd == 2 && D == 1) || nd == 3, "nfs_curl_bwd: nd must be 2 (then D == 1) or 3");
  if (int e = check_volume("nfs_curl_bwd", D, H, W, 1)) return e;
  hipLaunchKernelGGL(curl_bwd_kernel, dim3(blocks_for((int64_t)D * H * W, 256)), dim3(256), 0, as_stream(stream), g_out,
                     g_s, D, H, W, nd);
  return check_launch("nfs_curl_bwd");
}

int nfs_grad_fwd(const float* p, float* out, int D, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(p && out, "nfs_grad_fwd: null pointer");
  NFS_REQUIRE(out != p, "nfs_grad_fwd: out must not alias p");
  if (int e = check_volume("nfs_grad_fwd", D, H, W, 3)) return e;
  hipLaunchKernelGGL(grad_fwd_kernel, dim3(blocks_for((int64_t)D * H * W, 256)), dim3(256), 0, as_stream(stream), p, out, D,
                     H, W);
  return check_launch("nfs_grad_fwd");
}

int nfs_grad_bwd(const float* g_out, float* g_p, int D, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(g_out && g_p, "nfs_grad_bwd: null pointer");
  NFS_REQUIRE(g_p != g_out, "nfs_grad_bwd: g_p must not alias g_out (it is a gather)");
  if (int e = check_volume("nfs_grad_bwd", D, H, W, 3)) return e;
  hipLaunchKernelGGL(grad_bwd_kernel, dim3(blocks_for((int64_t)D * H * W, 256)), dim3(256), 0, as_stream(stream), g_out,
                     g_p, D, H, W);
  return check_launch("nfs_grad_bwd");
}

int nfs_stream_bwd_adam(const float* g_vel, float* s, float* m, float* v, int D, int H, int W, float lr_t, float beta1,
                        float beta2, float eps, nfs_stream_t stream) {
  return bwd_adam_launch("nfs_stream_bwd_adam", SRC_STREAM, g_vel, s, m, v, D, H, W, lr_t, beta1, beta2, eps, stream);
}

int nfs_potential_bwd_adam(const float* g_vel, float* phi, float* m, float* v, int D, int H, int W, float lr_t, float beta1,
                           float beta2, float eps, nfs_stream_t stream) {
  return bwd_adam_launch("nfs_potential_bwd_adam", SRC_POTENTIAL, g_vel, phi, m, v, D, H, W, lr_t, beta1, beta2, eps, stream);
}

int nfs_helmholtz_bwd_adam(const float* g_vel, float* a, float* m, float* v, int D, int H, int W, float lr_t, float beta1,
                           float beta2, float eps, nfs_stream_t stream) {
  return bwd_adam_launch("nfs_helmholtz_bwd_adam", SRC_HELMHOLTZ, g_vel, a, m, v, D, H, W, lr_t, beta1, beta2, eps, stream);
}

}  // extern "C"
