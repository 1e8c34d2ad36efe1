// libnfs_grid2d.so (include/nfs_grid2d.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI alone.
// The 2-D grid stylizer's field operators (engine: grid2d.py; include/nfs_grid2d.h "stylising a 2-D grid"): the D = 1
// restriction of the 3-D variables of source_ops.h with the D component dropped, on the exact reference stencil of
// warp2d.hip (x0 = floor, x1 = x0 + 1, both clipped to [0, n-1], weight dx = x - float(clipped x0)):
//   source2d_velocity<SRC>()   the velocity [2] a variable stands for at one pixel (FdEnd of source_ops.h)
//   source2d_adj<SRC>()        its transpose at one pixel (fd_adj of source_ops.h: a gather, H then W)
//   advect2d_sample / _grad    nfs_advect2d_fwd's sample and nfs_advect2d_bwd's velocity gradient for C = 1, the very
//                              expressions of warp2d_fwd_kernel / warp2d_bwd_kernel (the same bits)
// Streaming kernels over at most a few MB: one pixel per lane, row-major, no LDS, no atomics.  H, W >= 2, H * W < 2^30:
// every index is an int, and every index a kernel forms comes out of axis2d (clamped into [0, n), NaN included) or
// FdEnd::other / fd_adj (a neighbour inside the array by construction).
#include "advect_stencil.h"
#include "../../include/nfs_grid2d.h"

namespace nfs {

// vel0 = along H (array axis 0), vel1 = along W.  psi: vel0 = -D_W psi (the ends exchanged: a difference, not a negation, as
// curl_fwd_kernel forms it), vel1 = D_H psi; phi: vel0 = D_H phi, vel1 = D_W phi; (psi, phi): each part, then added once.
template <int SRC>
__device__ __forceinline__ F2u source2d_velocity(const float* __restrict__ var, int pix, int y, int x, int H, int W) {
  if constexpr (SRC == SRC_VEL) {
    return *reinterpret_cast<const F2u*>(var + (size_t)pix * 2);
  } else {
    const FdEnd<false> ex(x, W), ey(y, H);
    if constexpr (SRC == SRC_STREAM) {
      const float p = var[pix];
      return F2u{ex.d(var[ex.other(pix, 1)], p), ey.d(p, var[ey.other(pix, W)])};
    } else if constexpr (SRC == SRC_POTENTIAL) {
      const float p = var[pix];
      return F2u{ey.d(p, var[ey.other(pix, W)]), ex.d(p, var[ex.other(pix, 1)])};
    } else {
      const F2u* a2 = reinterpret_cast<const F2u*>(var);
      const F2u p = a2[pix], qx = a2[ex.other(pix, 1)], qy = a2[ey.other(pix, W)];
      const float s0 = ex.d(qx.x, p.x), s1 = ey.d(p.x, qy.x);
      const float g0 = ey.d(p.y, qy.y), g1 = ex.d(p.y, qx.y);
      return F2u{s0 + g0, s1 + g1};
    }
  }
}

// Component c of the transpose at pixel (y, x) of g [H,W,2] (advect's channel order); c = 0: psi's (s, sp) or phi's (p),
// c = 1: phi's (sp).  Summed H, then W, wherever it is formed.
template <int SRC>
__device__ __forceinline__ float source2d_adj(const float* __restrict__ g, int y, int x, int H, int W, int c) {
  if constexpr (SRC == SRC_VEL) return g[((size_t)y * W + x) * 2 + c];
  auto ah = [&](int k) { return fd_adj(g, x, W, y, H, k, 2); };
  auto aw = [&](int k) { return fd_adj(g, (int64_t)y * W, 1, x, W, k, 2); };
  if (SRC == SRC_POTENTIAL || c == 1) return ah(0) + aw(1);
  return ah(1) - aw(0);
}

template <int SRC> struct Var2 { static constexpr int NCH = (SRC == SRC_VEL || SRC == SRC_HELMHOLTZ) ? 2 : 1; };

// (Bilinear, axis2d, bilinear_setup, advect2d_sample, advect2d_grad: advect_stencil.h, shared with descent.hip)

// MODE 0: out = advect2d(d, vel(var));  1: g_vel of that advect;  2 (SRC_VEL): g_vel consumed by ApplyAdam on var = vel,
// m, v in place, then out (nullable) = advect2d(d, updated vel) -- all local to the pixel (d is constant)
template <int SRC, int MODE>
__global__ void __launch_bounds__(256) advect2d_source_kernel(const float* __restrict__ d, const float* var,
                                                              const float* __restrict__ g_out, float* out, float* m,
                                                              float* v, int H, int W, float lr_t, float b1, float b2,
                                                              float eps) {
  static_assert(MODE != 2 || SRC == SRC_VEL, "the fused update is the velocity variable's");
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  const int x = pix % W, y = pix / W;
  F2u vel = source2d_velocity<SRC>(var, pix, y, x, H, W);
  const Bilinear b = bilinear_setup(y, x, H, W, vel.x, vel.y);
  if constexpr (MODE == 0) {
    out[pix] = advect2d_sample(d, b);
  } else {
    const F2u g = advect2d_grad(d, b, g_out[pix], H, W);
    if constexpr (MODE == 1) {
      reinterpret_cast<F2u*>(out)[pix] = g;
    } else {
      F2u ms = reinterpret_cast<const F2u*>(m)[pix], us = reinterpret_cast<const F2u*>(v)[pix];
      adam_tf(vel.x, ms.x, us.x, g.x, lr_t, b1, b2, eps);
      adam_tf(vel.y, ms.y, us.y, g.y, lr_t, b1, b2, eps);
      reinterpret_cast<F2u*>(const_cast<float*>(var))[pix] = vel;
      reinterpret_cast<F2u*>(m)[pix] = ms;
      reinterpret_cast<F2u*>(v)[pix] = us;
      if (out) out[pix] = advect2d_sample(d, bilinear_setup(y, x, H, W, vel.x, vel.y));
    }
  }
}

template <int SRC>
__global__ void __launch_bounds__(256) source2d_velocity_fwd_kernel(const float* __restrict__ var, float* __restrict__ vel,
                                                                    int H, int W) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  reinterpret_cast<F2u*>(vel)[pix] = source2d_velocity<SRC>(var, pix, pix / W, pix % W, H, W);
}

// g_var = the transpose, stored (a thread reads g at its neighbours only)
template <int SRC>
__global__ void __launch_bounds__(256) source2d_bwd_kernel(const float* __restrict__ g, float* __restrict__ g_var, int H,
                                                           int W) {
  constexpr int NCH = Var2<SRC>::NCH;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  const int x = pix % W, y = pix / W;
#pragma unroll
  for (int c = 0; c < NCH; ++c) g_var[(size_t)pix * NCH + c] = source2d_adj<SRC>(g, y, x, H, W, c);
}

// out = w_g * advect2d(g, scale * u) + w_add * addend on the LEAN stencil of warp.hip's transport_step_kernel, in 2-D: the
// coordinate in cells by one FMA (x = index - scale u (n-1)/2: exact where u is zero), clamped to [0, n-1] (fmaxf / fminf:
// a NaN lands on 0), base cell min(floor, n-2), weights in [0, 1]; the sample by chained FMAs, x within each row, then y
__global__ void __launch_bounds__(256) transport_step2d_kernel(const float* __restrict__ g, const float* __restrict__ u,
                                                               const float* __restrict__ addend, float* __restrict__ out,
                                                               int H, int W, int C, float scale, float w_g, float w_add) {
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  if (pix >= H * W) return;
  const int x = pix % W, y = pix / W;
  const F2u uv = reinterpret_cast<const F2u*>(u)[pix];
  const float hy = 0.5f * (float)(H - 1) * scale, hx = 0.5f * (float)(W - 1) * scale;
  const float cy = fminf(fmaxf(fmaf(-uv.x, hy, (float)y), 0.f), (float)(H - 1));
  const float cx = fminf(fmaxf(fmaf(-uv.y, hx, (float)x), 0.f), (float)(W - 1));
  const float by = fminf(floorf(cy), (float)(H - 2)), bx = fminf(floorf(cx), (float)(W - 2));
  const float wy = cy - by, wx = cx - bx;
  const size_t o = (size_t)((int)by * W + (int)bx) * C, row = (size_t)W * C;
  for (int c = 0; c < C; ++c) {
    const float p00 = g[o + c], p01 = g[o + C + c], p10 = g[o + row + c], p11 = g[o + row + C + c];
    const float a0 = fmaf(wx, p01 - p00, p00), a1 = fmaf(wx, p11 - p10, p10);
    float s = w_g * fmaf(wy, a1 - a0, a0);
    if (addend) s = fmaf(w_add, addend[(size_t)pix * C + c], s);
    out[(size_t)pix * C + c] = s;
  }
}

static int check_grid2d(const char* who, int H, int W, int src) {
  NFS_REQUIRE(H >= 2 && W >= 2, "%s: H and W must be at least 2 (got %d x %d)", who, H, W);
  NFS_REQUIRE((int64_t)H * W < ((int64_t)1 << 30), "%s: H * W must be below 2^30", who);
  NFS_REQUIRE(src >= SRC_VEL && src <= SRC_HELMHOLTZ, "%s: src %d is none of 0 (velocity), 1 (stream function), 2 (potential), "
              "3 (both)", who, src);
  return NFS_OK;
}

#define NFS_BY_SRC(src, KERNEL, ...)                                                              \
  ((src) == SRC_VEL ? KERNEL<SRC_VEL, __VA_ARGS__> : (src) == SRC_STREAM ? KERNEL<SRC_STREAM, __VA_ARGS__> \
   : (src) == SRC_POTENTIAL ? KERNEL<SRC_POTENTIAL, __VA_ARGS__> : KERNEL<SRC_HELMHOLTZ, __VA_ARGS__>)

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_grid2d_version(void) { return NFS_GRID2D_ABI_VERSION; }

int nfs_source2d_velocity_fwd(const float* var, int src, float* vel, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(var && vel, "nfs_source2d_velocity_fwd: null pointer");
  NFS_REQUIRE(vel != var, "nfs_source2d_velocity_fwd: vel must not alias var");
  if (int e = check_grid2d("nfs_source2d_velocity_fwd", H, W, src)) return e;
  hipLaunchKernelGGL(src == SRC_VEL ? source2d_velocity_fwd_kernel<SRC_VEL>
                     : src == SRC_STREAM ? source2d_velocity_fwd_kernel<SRC_STREAM>
                     : src == SRC_POTENTIAL ? source2d_velocity_fwd_kernel<SRC_POTENTIAL>
                                            : source2d_velocity_fwd_kernel<SRC_HELMHOLTZ>,
                     dim3(blocks_for((int64_t)H * W, 256)), dim3(256), 0, as_stream(stream), var, vel, H, W);
  return check_launch("nfs_source2d_velocity_fwd");
}

int nfs_source2d_velocity_bwd(const float* g_vel, int src, float* g_var, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(g_vel && g_var, "nfs_source2d_velocity_bwd: null pointer");
  NFS_REQUIRE(g_var != g_vel, "nfs_source2d_velocity_bwd: g_var must not alias g_vel (it is a gather)");
  if (int e = check_grid2d("nfs_source2d_velocity_bwd", H, W, src)) return e;
  hipLaunchKernelGGL(src == SRC_VEL ? source2d_bwd_kernel<SRC_VEL> : src == SRC_STREAM ? source2d_bwd_kernel<SRC_STREAM>
                     : src == SRC_POTENTIAL ? source2d_bwd_kernel<SRC_POTENTIAL> : source2d_bwd_kernel<SRC_HELMHOLTZ>,
                     dim3(blocks_for((int64_t)H * W, 256)), dim3(256), 0, as_stream(stream), g_vel, g_var, H, W);
  return check_launch("nfs_source2d_velocity_bwd");
}

int nfs_advect2d_source_fwd(const float* d, const float* var, int src, float* out, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(d && var && out, "nfs_advect2d_source_fwd: null pointer");
  NFS_REQUIRE(out != d && out != var, "nfs_advect2d_source_fwd: out must not alias d or var (it is a gather)");
  if (int e = check_grid2d("nfs_advect2d_source_fwd", H, W, src)) return e;
  hipLaunchKernelGGL(NFS_BY_SRC(src, advect2d_source_kernel, 0), dim3(blocks_for((int64_t)H * W, 256)), dim3(256), 0,
                     as_stream(stream), d, var, (const float*)nullptr, out, (float*)nullptr, (float*)nullptr, H, W, 0.f,
                     0.f, 0.f, 0.f);
  return check_launch("nfs_advect2d_source_fwd");
}

int nfs_advect2d_source_bwd(const float* d, const float* var, int src, const float* g_out, float* g_vel, int H, int W,
                            nfs_stream_t stream) {
  NFS_REQUIRE(d && var && g_out && g_vel, "nfs_advect2d_source_bwd: null pointer");
  NFS_REQUIRE(g_vel != d && g_vel != var && g_vel != g_out, "nfs_advect2d_source_bwd: g_vel must not alias an input");
  if (int e = check_grid2d("nfs_advect2d_source_bwd", H, W, src)) return e;
  hipLaunchKernelGGL(NFS_BY_SRC(src, advect2d_source_kernel, 1), dim3(blocks_for((int64_t)H * W, 256)), dim3(256), 0,
                     as_stream(stream), d, var, g_out, g_vel, (float*)nullptr, (float*)nullptr, H, W, 0.f, 0.f, 0.f, 0.f);
  return check_launch("nfs_advect2d_source_bwd");
}

int nfs_advect2d_bwd_adam_fwd(const float* d, float* vel, const float* g_out, float* m, float* v, float* adv_next, int H,
                              int W, float lr_t, float beta1, float beta2, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && g_out && m && v, "nfs_advect2d_bwd_adam_fwd: null pointer");
  NFS_REQUIRE(adv_next != d && adv_next != g_out && adv_next != vel && adv_next != m && adv_next != v,
              "nfs_advect2d_bwd_adam_fwd: adv_next must not alias d, g_out, vel, m or v");
  if (int e = check_grid2d("nfs_advect2d_bwd_adam_fwd", H, W, SRC_VEL)) return e;
  hipLaunchKernelGGL((advect2d_source_kernel<SRC_VEL, 2>), dim3(blocks_for((int64_t)H * W, 256)), dim3(256), 0,
                     as_stream(stream), d, vel, g_out, adv_next, m, v, H, W, lr_t, beta1, beta2, eps);
  return check_launch("nfs_advect2d_bwd_adam_fwd");
}

int nfs_transport_step2d(const float* g, const float* u, float scale, float w_g, const float* addend, float w_addend,
                         float* out, int H, int W, int C, nfs_stream_t stream) {
  NFS_REQUIRE(g && u && out, "nfs_transport_step2d: null pointer");
  NFS_REQUIRE(g != out && u != out, "nfs_transport_step2d: out must not alias g or u (it is a gather)");
  NFS_REQUIRE(C >= 1, "nfs_transport_step2d: C must be at least 1");
  if (int e = check_grid2d("nfs_transport_step2d", H, W, SRC_VEL)) return e;
  hipLaunchKernelGGL(transport_step2d_kernel, dim3(blocks_for((int64_t)H * W, 256)), dim3(256), 0, as_stream(stream), g, u,
                     addend, out, H, W, C, scale, w_g, w_addend);
  return check_launch("nfs_transport_step2d");
}

}  // extern "C"
