// The advect stencils, each written once and shared by the libraries that must agree bit for bit:
//   the lean stencil (3-D, scalar field, a multiple of four voxels)   advect1_kernel / transport_step_kernel (warp.hip) and
//                                                                     advect_descent4_kernel (descent.hip)
//   the reference stencil in 2-D                                      grid2d.hip and advect2d_descent_kernel (descent.hip)
//   the reference stencil in 3-D for a scalar field                   advect_descent1_kernel (descent.hip): the bits of
//                                                                     warp_fwd_kernel<COORD_ADVECT> (warp.hip) for C = 1
// The lean pieces are explicit FMAs, differences and clamps (nothing a compiler can contract); the reference pieces are
// written with contraction off, see the comment above axis2d.
#pragma once
#include "source_ops.h"

namespace nfs {

// live mask (nullable; whole-volume launches only): bit i of the mask = "the eight density corners the back-traced point
// of voxel i interpolates are NOT all equal".  Where they are equal the sample does not depend on the coordinate and the
// velocity gradient of that voxel is g * 0 whatever g is, so the adjoint chain above it (rotate, smooth) need not
// produce g there (rotate_bwd_tiled_kernel skips the tiles / clips to the box that matter).  A wave's lanes hold 64
// consecutive voxels per j: one ballot = one 64-bit word of the mask.
__device__ __forceinline__ bool corners_differ(const F2u (&p)[4]) {
  const float a = p[0].x;
  return !(p[0].y == a && p[1].x == a && p[1].y == a && p[2].x == a && p[2].y == a && p[3].x == a && p[3].y == a);
}

// ---- the lean stencil (advect1_kernel, transport_step_kernel), every piece of it written once ---------------------
// per-volume constants: (n-1)/2 per axis (velocity -> voxels), n-1 per axis (the clamp), row and plane strides
struct LeanDims { float hz, hy, hx, nz1, ny1, nx1; unsigned uW, uHW; };
__device__ __forceinline__ LeanDims lean_dims(int D, int H, int W) {
  return {0.5f * (float)(D - 1), 0.5f * (float)(H - 1), 0.5f * (float)(W - 1),
          (float)(D - 1), (float)(H - 1), (float)(W - 1), (unsigned)W, (unsigned)(H * W)};
}

// back-traced point of voxel (z, h, w): coordinate x = index - vel * (n-1)/2 by one FMA (un-clamped: the gradient asks
// whether it lies inside), clamped to [0, n-1], base cell min(floor, n-2), weights in [0,1], linear offset of the base cell
struct LeanCell { float xz, xy, xx, wz, wy, wx; unsigned o; };
__device__ __forceinline__ LeanCell lean_cell(const F3u& v, int z, int h, int w, const LeanDims& s) {
  LeanCell c;
  c.xz = fmaf(-v.x, s.hz, (float)z); c.xy = fmaf(-v.y, s.hy, (float)h); c.xx = fmaf(-v.z, s.hx, (float)w);
  const float cz = __builtin_amdgcn_fmed3f(c.xz, 0.f, s.nz1), cy = __builtin_amdgcn_fmed3f(c.xy, 0.f, s.ny1),
              cx = __builtin_amdgcn_fmed3f(c.xx, 0.f, s.nx1);
  const float bz = fminf(floorf(cz), s.nz1 - 1.f), by = fminf(floorf(cy), s.ny1 - 1.f), bx = fminf(floorf(cx), s.nx1 - 1.f);
  c.wz = cz - bz; c.wy = cy - by; c.wx = cx - bx;
  c.o = (unsigned)(int)bz * s.uHW + (unsigned)(int)by * s.uW + (unsigned)(int)bx;
  return c;
}

// the four rows (z,y), (z,y+1), (z+1,y), (z+1,y+1) of the cell at offset o, each an (x, x+1) pair of T
template <typename T>
__device__ __forceinline__ void lean_gather(const T* d, unsigned o, const LeanDims& s, T (&lo)[4], T (&hi)[4]) {
  const unsigned r[4] = {o, o + s.uW, o + s.uHW, o + s.uHW + s.uW};
#pragma unroll
  for (int k = 0; k < 4; ++k) { lo[k] = d[r[k]]; hi[k] = d[r[k] + 1]; }
}
// ... of a scalar field: one dword-aligned 8-byte load per row
__device__ __forceinline__ void lean_gather(const float* d, unsigned o, const LeanDims& s, F2u (&p)[4]) {
  p[0] = *reinterpret_cast<const F2u*>(d + o);
  p[1] = *reinterpret_cast<const F2u*>(d + o + s.uW);
  p[2] = *reinterpret_cast<const F2u*>(d + o + s.uHW);
  p[3] = *reinterpret_cast<const F2u*>(d + o + s.uHW + s.uW);
}

// trilinear combine: x within each row (e: the row's difference, a: its value at wx), then y, then z
__device__ __forceinline__ void lean_rows(const F2u (&p)[4], float wx, float (&e)[4], float (&a)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { e[k] = p[k].y - p[k].x; a[k] = fmaf(wx, e[k], p[k].x); }
}
__device__ __forceinline__ float lean_sample(const F2u (&p)[4], float wx, float wy, float wz) {
  float e[4], a[4];
  lean_rows(p, wx, e, a);
  const float b0 = fmaf(wy, a[1] - a[0], a[0]), b1 = fmaf(wy, a[3] - a[2], a[2]);
  return fmaf(wz, b1 - b0, b0);
}

// gradient of that sample along (z, y, x), in cells: difference of the two faces, interpolated in the other two axes
// (the arithmetic of advect1_kernel's adjoint branch)
__device__ __forceinline__ void lean_grad(const F2u (&p)[4], float wx, float wy, float wz, float& dz, float& dy, float& dx) {
  float e[4], a[4];
  lean_rows(p, wx, e, a);
  const float f0 = fmaf(wy, e[1] - e[0], e[0]), f1 = fmaf(wy, e[3] - e[2], e[2]);
  dx = fmaf(wz, f1 - f0, f0);
  const float g0 = a[1] - a[0], g1 = a[3] - a[2];
  dy = fmaf(wz, g1 - g0, g0);
  const float b0 = fmaf(wy, g0, a[0]), b1 = fmaf(wy, g1, a[2]);
  dz = b1 - b0;
}

// next voxel of this lane: 64 further on (clamped at the end of the volume; those results are not stored)
__device__ __forceinline__ void walk64(int& w, int& h, int& z, int W, int H, int zlast) {
  w += 64;
  while (w >= W) { w -= W; if (++h == H) { h = 0; if (z < zlast) ++z; } }
}

// A wave owns NV x 64 consecutive voxels and lane l takes l, l + 64, ...: every streamed access (12-byte velocity /
// moment vectors, g_out, out) is then one contiguous run per instruction.  (Consecutive voxels per lane with float4
// accesses put the lanes 48 bytes apart: 24 cache lines per instruction, a third of each used.)
// XCD_ORDER: contiguous z-slab per XCD (workgroups are dealt round-robin to the 8 XCDs; the grid is a multiple of 8): the
// gathered planes of neighbouring rows then come through one L2 instead of being fetched into all eight.
// Returns the lane's first voxel; the wave has none when first - lane >= n.  (block_threads: blockDim.x, read by the kernel
// itself -- only there does the compiler fold it to the launch's uniform block size.)
template <int NV, bool XCD_ORDER>
__device__ __forceinline__ int lane_first(unsigned block_threads, int lane) {
  const unsigned per_xcd = gridDim.x / 8;
  const unsigned lb = XCD_ORDER ? (blockIdx.x % 8) * per_xcd + blockIdx.x / 8 : blockIdx.x;
  return (lb * block_threads + (threadIdx.x - lane)) * NV + lane;
}
// ... and its position (z, h, w), clamped into the volume; walk64 steps on from there
__device__ __forceinline__ void lane_start(int first, int n, int H, int W, int& w, int& h, int& z) {
  const int f0 = min(first, n - 1);
  w = f0 % W;
  const int t2 = f0 / W;
  h = t2 % H; z = t2 / H;
}

// ---- the reference stencil in 2-D (x0 = floor, x1 = x0 + 1, both clipped to [0, n-1], weight dx = x - float(clipped x0)) ----
struct Bilinear {
  int o00, o01, o10, o11;       // o[p][q]: corner p along H, q along W
  float wy0, wy1, wx0, wx1;
};
// Bit-identity with nfs_advect2d_fwd / _bwd (C = 1) needs the very roundings of warp2d.hip's kernels.  Those are compiled
// with floating-point contraction on, and which products the compiler fused there is not visible in their source: for
// C = 1 the forward sum is four plain products and three plain additions; the adjoint forms each axis' bracket as ONE
// fused multiply-add onto ONE plain product (the fused term is the (1 - dx) one along H and the dx one along W) and adds
// it to its channel sum by an FMA; lin_coord is an FMA in both.  So the arithmetic below is written out with contraction
// OFF and explicit fmaf() where those kernels fuse; tests/test_grid2d_kernels_gpu.py holds the two together bit for bit.
__device__ __forceinline__ Axis axis2d(int i, int n, float vel) {
#pragma clang fp contract(off)
  const float step = 2.f / (float)(n - 1);                        // (n >= 2)
  const float c = fmaf(step, (float)i, -1.f) - vel;               // lin_coord(i, n) - vel
  const float x = (c + 1.f) * (float)(n - 1) * 0.5f;
  float f = floorf(x);
  f = fminf(fmaxf(f, -1.f), (float)n);                            // keeps the int conversion defined (also for NaN)
  const int k = (int)f;
  Axis a;
  a.i0 = min(max(k, 0), n - 1);
  a.i1 = min(max(k + 1, 0), n - 1);
  a.w1 = x - (float)a.i0;
  return a;
}
__device__ __forceinline__ Bilinear bilinear_setup(int y, int x, int H, int W, float v0, float v1) {
#pragma clang fp contract(off)
  const Axis ay = axis2d(y, H, v0), ax = axis2d(x, W, v1);
  return Bilinear{ay.i0 * W + ax.i0, ay.i0 * W + ax.i1, ay.i1 * W + ax.i0, ay.i1 * W + ax.i1,
                  1.f - ay.w1, ay.w1, 1.f - ax.w1, ax.w1};
}
// add_n order of the reference: w00 I00 + w01 I01 + w10 I10 + w11 I11
__device__ __forceinline__ float advect2d_sample(const float* __restrict__ d, const Bilinear& b) {
#pragma clang fp contract(off)
  const float w00 = b.wy0 * b.wx0, w01 = b.wy0 * b.wx1, w10 = b.wy1 * b.wx0, w11 = b.wy1 * b.wx1;
  return ((w00 * d[b.o00] + w01 * d[b.o01]) + w10 * d[b.o10]) + w11 * d[b.o11];
}
// g_vel of one pixel: minus the sample's derivative along each axis in normalised units, times g
__device__ __forceinline__ F2u advect2d_grad(const float* __restrict__ d, const Bilinear& b, float g, int H, int W) {
#pragma clang fp contract(off)
  const float v00 = d[b.o00], v01 = d[b.o01], v10 = d[b.o10], v11 = d[b.o11];
  float gy = fmaf(g, fmaf(b.wx0, v10 - v00, b.wx1 * (v11 - v01)), 0.f);
  float gx = fmaf(g, fmaf(b.wy1, v11 - v10, b.wy0 * (v01 - v00)), 0.f);
  gy *= (float)(H - 1) * 0.5f;
  gx *= (float)(W - 1) * 0.5f;
  return F2u{-gy, -gx};
}

// ---- the reference stencil in 3-D, scalar field: the sample of nfs_advect_fwd's generic kernel ------------------------------
// warp_fwd_kernel<COORD_ADVECT> takes the volumes the lean kernel does not (a voxel count that is no multiple of 4).  It is
// compiled with contraction on; for C = 1 its compiled code is: lin_coord an FMA, the coordinate exactly axis2d's (its
// weight x - float(i0) is there fma(t, 0.5, -i0), the same number: halving is exact), every corner weight the plain
// products (wz * wy) * wx, every term a plain product weight * value, and the eight terms added one by one onto 0.f in
// the order z, y, x (x innermost).  Written out here with contraction off; tests/test_descent_kernels_gpu.py holds the two
// together bit for bit.  D, H, W >= 2; every index comes out of axis2d (clamped into [0, n), NaN included), the 8-byte
// row load starts at min(i0, W - 2).
__device__ __forceinline__ float advect3d_ref_sample(const float* __restrict__ d, int z, int h, int w, int D, int H, int W,
                                                     const F3u& v) {
#pragma clang fp contract(off)
  const Axis az = axis2d(z, D, v.x), ay = axis2d(h, H, v.y), ax = axis2d(w, W, v.z);
  const int xb = min(ax.i0, W - 2);
  const bool x0_lo = ax.i0 == xb, x1_lo = ax.i1 == xb;
  const float wz[2] = {1.f - az.w1, az.w1}, wy[2] = {1.f - ay.w1, ay.w1}, wx[2] = {1.f - ax.w1, ax.w1};
  const int iz[2] = {az.i0, az.i1}, iy[2] = {ay.i0, ay.i1};
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const F2u p = *reinterpret_cast<const F2u*>(d + ((int64_t)iz[a] * H + iy[b]) * W + xb);
      const float v0 = x0_lo ? p.x : p.y, v1 = x1_lo ? p.x : p.y;
      const float wzy = wz[a] * wy[b];
      const float t0 = (wzy * wx[0]) * v0, t1 = (wzy * wx[1]) * v1;
      s = s + t0;
      s = s + t1;
    }
  return s;
}

}  // namespace nfs
