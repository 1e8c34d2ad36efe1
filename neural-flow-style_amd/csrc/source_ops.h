// The variables a velocity can be a function of -- a stream function s [D,H,W,3], a potential phi [D,H,W], a Helmholtz
// variable a [D,H,W,4] = (psi0, psi1, psi2, phi) -- and their operators, each written once:
//   source_velocity<SRC>()   the velocity the variable stands for at one voxel   (advect1_kernel, warp.hip; the stand-alone
//                            curl and gradient, source.hip)
//   source_adj<SRC>()        the transpose at one voxel                           (curl_bwd / grad_bwd and the fused updates,
//                            source.hip)
// Forward differences with the last slice replicated (transform.py:508-555): output i of an axis is s[l + 1] - s[l] at
// l = fd_lo(i, n).  Velocities are in advect's channel order (component k along array axis k); the reference's curl and
// gradient are the same values with the channels reversed.  Differences and sums only: nothing here can contract.
#pragma once
#include "common.h"

namespace nfs {

struct __attribute__((packed, aligned(4))) F3u { float x, y, z; };

// where advect1_kernel's velocity comes from: the stored field, or one of the three variables it is a function of
enum { SRC_VEL = 0, SRC_STREAM = 1, SRC_POTENTIAL = 2, SRC_HELMHOLTZ = 3 };
// (what the entry points' messages call the variable)
inline const char* source_name(int src) { return src == SRC_STREAM ? "s" : "the variable"; }

// One axis of the forward difference at index i of n, seen from the voxel's own sample p: p is one end of it -- the lower
// one (d = q - p, q the next sample), or the upper one on the last slice (d = p - q, q the previous sample).
// THIN: the axis may be shorter than 2; the difference is then zero and the other end is the voxel itself (nothing outside
// the array is read).  Without THIN the caller guarantees n >= 2.
template <bool THIN>
struct FdEnd {
  bool lower, flat;
  __device__ __forceinline__ FdEnd(int i, int n) : lower(fd_lo(i, n) == i), flat(THIN && n < 2) {}
  __device__ __forceinline__ size_t other(size_t own, size_t stride) const {
    return flat ? own : lower ? own + stride : own - stride;
  }
  __device__ __forceinline__ float d(float p, float q) const { return flat ? 0.f : lower ? q - p : p - q; }
};

// stream part: vel0 = D_W s1 - D_H s0,  vel1 = D_D s0 - D_W s2,  vel2 = D_H s2 - D_D s1
// (p: the voxel's own s; qx, qy, qz: the other end along W, H, D, the two components that axis differentiates)
template <bool THIN>
__device__ __forceinline__ F3u stream_part(const FdEnd<THIN>& ex, const FdEnd<THIN>& ey, const FdEnd<THIN>& ez, float p0, float p1,
                                           float p2, float qx1, float qx2, float qy0, float qy2, float qz0, float qz1) {
  const float dw1 = ex.d(p1, qx1), dw2 = ex.d(p2, qx2);
  const float dh0 = ey.d(p0, qy0), dh2 = ey.d(p2, qy2);
  const float dd0 = ez.d(p0, qz0), dd1 = ez.d(p1, qz1);
  return F3u{dw1 - dh0, dd0 - dw2, dh2 - dd1};
}

// potential part: vel0 = D_D phi,  vel1 = D_H phi,  vel2 = D_W phi
template <bool THIN>
__device__ __forceinline__ F3u potential_part(const FdEnd<THIN>& ex, const FdEnd<THIN>& ey, const FdEnd<THIN>& ez, float p, float qx,
                                              float qy, float qz) {
  return F3u{ez.d(p, qz), ey.d(p, qy), ex.d(p, qx)};
}

// The velocity of voxel (z, h, w), vox its linear index.  Helmholtz: each part formed as above, then added once.  The
// loads are per kind:
//   s    the own 12-byte vector and one further vector per axis, the components that axis differentiates (x: s1 s2 and
//        z: s0 s1 as one 8-byte load); in advect1_kernel the x neighbour is the next lane's own vector, the y and z
//        neighbours are re-reads of the next row / plane
//   phi  the own sample and one neighbour per axis
//   a    four 16-byte vectors (of which the compiler loads only the components used); a is 16-byte aligned
template <int SRC, bool THIN = false>
__device__ __forceinline__ F3u source_velocity(const float* __restrict__ var, size_t vox, int z, int h, int w, int D, int H,
                                               int W) {
  static_assert(SRC == SRC_STREAM || SRC == SRC_POTENTIAL || SRC == SRC_HELMHOLTZ, "a variable, not the stored velocity");
  const FdEnd<THIN> ex(w, W), ey(h, H), ez(z, D);
  if constexpr (SRC == SRC_STREAM) {
    const size_t own = vox * 3;
    const F3u p = *reinterpret_cast<const F3u*>(var + own);
    const F2u qx = *reinterpret_cast<const F2u*>(var + ex.other(own, 3) + 1);                   // s1, s2
    const F3u qy = *reinterpret_cast<const F3u*>(var + ey.other(own, (size_t)W * 3));           // s0, (s1), s2
    const F2u qz = *reinterpret_cast<const F2u*>(var + ez.other(own, (size_t)H * W * 3));       // s0, s1
    return stream_part(ex, ey, ez, p.x, p.y, p.z, qx.x, qx.y, qy.x, qy.z, qz.x, qz.y);
  } else if constexpr (SRC == SRC_POTENTIAL) {
    return potential_part(ex, ey, ez, var[vox], var[ex.other(vox, 1)], var[ey.other(vox, (size_t)W)],
                          var[ez.other(vox, (size_t)H * W)]);
  } else {
    const float4* a4 = reinterpret_cast<const float4*>(var);
    const float4 p = a4[vox], qx = a4[ex.other(vox, 1)], qy = a4[ey.other(vox, (size_t)W)],
                 qz = a4[ez.other(vox, (size_t)H * W)];
    const F3u s = stream_part(ex, ey, ez, p.x, p.y, p.z, qx.y, qx.z, qy.x, qy.z, qz.x, qz.y);
    const F3u g = potential_part(ex, ey, ez, p.w, qx.w, qy.w, qz.w);
    return F3u{s.x + g.x, s.y + g.y, s.z + g.z};
  }
}

// TF ApplyAdam of one element, as the plain expression (adam_kernel's, field.hip; fmaf here would choose bits): what the
// fused updates of source.hip and grid2d.hip consume their gradient with
__device__ __forceinline__ void adam_tf(float& x, float& m, float& u, float g, float lr_t, float b1, float b2, float eps) {
  m = b1 * m + (1.f - b1) * g;
  u = b2 * u + (1.f - b2) * g * g;
  x -= lr_t * m / (sqrtf(u) + eps);
}

// ---- the transposes ------------------------------------------------------------------------------------------------------
// A forward difference taken at cell l = fd_lo(i) contributes +g to s[l+1] and -g to s[l]; cell i receives from the outputs
// whose l equals i (outputs i, and n-1 as well when i == n-2) and whose l+1 equals i.
// Written as a gather over the (at most three) contributing outputs per axis: no atomics, deterministic.
__device__ __forceinline__ float fd_adj(const float* __restrict__ g, int64_t base, int64_t stride, int i, int n, int ch,
                                        int nch) {
  // sum over outputs o along this axis: coefficient of s[i] in (s[lo(o)+1] - s[lo(o)])
  if (n < 2) return 0.f;
  float r = 0.f;
  if (i >= 1) {                       // s[i] is the upper sample of outputs with lo == i-1
    r += g[(base + (int64_t)(i - 1) * stride) * nch + ch];
    if (i == n - 1) r += g[(base + (int64_t)(n - 1) * stride) * nch + ch];   // replicated last slice (lo = n-2)
  }
  if (i <= n - 2) {                   // s[i] is the lower sample of outputs with lo == i
    r -= g[(base + (int64_t)i * stride) * nch + ch];
    if (i == n - 2) r -= g[(base + (int64_t)(n - 1) * stride) * nch + ch];
  }
  return r;
}

// Component c of the transpose of source_velocity<SRC> at voxel (z, y, x): c = 0..2 the stream part's (s, a), c = 0 the
// potential part's (phi), c = 3 the potential part's (a).  cd, ch, cw: the channels of g [D,H,W,3] that hold the velocity
// component along D, H and W (0, 1, 2 in advect's order, 2, 1, 0 in the reference's).  Each fd_adj is a gather and the sums
// are formed in THIS order wherever they are formed -- the curl's as written, the gradient's D, then H, then W -- so that
// the stand-alone adjoints and the fused updates give the same bits.
template <int SRC>
__device__ __forceinline__ float source_adj(const float* __restrict__ g, int z, int y, int x, int D, int H, int W, int cd, int ch,
                                            int cw, int c) {
  const int64_t sz = (int64_t)H * W, bx = z * sz + (int64_t)y * W, by = z * sz + x, bz = (int64_t)y * W + x;
  auto ad = [&](int k) { return fd_adj(g, bz, sz, z, D, k, 3); };   // fd_adj along D, H and W of channel k
  auto ah = [&](int k) { return fd_adj(g, by, W, y, H, k, 3); };
  auto aw = [&](int k) { return fd_adj(g, bx, 1, x, W, k, 3); };
  if (SRC == SRC_POTENTIAL || c == 3) return ad(cd) + ah(ch) + aw(cw);
  // vel_D = D_W s1 - D_H s0 ; vel_H = D_D s0 - D_W s2 ; vel_W = D_H s2 - D_D s1
  return c == 0 ? ad(ch) - ah(cd) : c == 1 ? aw(cd) - ad(cw) : ah(cw) - aw(ch);
}

}  // namespace nfs
