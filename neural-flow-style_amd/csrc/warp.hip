// A2/A3/A11: border-replicating trilinear resampling family (transform.py:238-269,
// 343-433, 557-569, 611-628).  One thread per output voxel, W fastest => coalesced
// stores and near-coalesced gathers; coordinates are generated in registers (the
// reference materialises 3 coordinate volumes + 8 index/weight/gather tensors).
// HBM-bound: algorithmic bytes = read volume once + write output once.
#include "advect_stencil.h"
#include <stdlib.h>

namespace nfs {

typedef float f32x2 __attribute__((ext_vector_type(2)));

enum CoordKind { COORD_EXPLICIT = 0, COORD_ROTATE = 1, COORD_ADVECT = 2 };

struct WarpArgs {
  const float* src;     // fwd: source volume(s); bwd: as fwd (may be null when unused)
  const float* coords;  // explicit [B,3,X,Y,Z] | rot [B,9] | vel [X,Y,Z,3]
  int B, X, Y, Z, C;
  int src_batched;      // 1: src has a batch dim (explicit), 0: one shared volume (rotate/advect)
};

template <int KIND>
__device__ __forceinline__ void coords_at(const WarpArgs& a, int b, int x, int y, int z, int64_t vox,
                                          float& cx, float& cy, float& cz) {
  if (KIND == COORD_EXPLICIT) {
    const int64_t n = (int64_t)a.X * a.Y * a.Z;
    const float* c = a.coords + (int64_t)b * 3 * n;
    cx = c[vox];
    cy = c[n + vox];
    cz = c[2 * n + vox];
  } else if (KIND == COORD_ROTATE) {
    const float* r = a.coords + b * 9;
    const float gx = lin_coord(x, a.X), gy = lin_coord(y, a.Y), gz = lin_coord(z, a.Z);
    cx = r[0] * gx + r[1] * gy + r[2] * gz;
    cy = r[3] * gx + r[4] * gy + r[5] * gz;
    cz = r[6] * gx + r[7] * gy + r[8] * gz;
  } else {
    const float* v = a.coords + vox * 3;
    cx = lin_coord(x, a.X) - v[0];
    cy = lin_coord(y, a.Y) - v[1];
    cz = lin_coord(z, a.Z) - v[2];
  }
}

template <int KIND>
__global__ void __launch_bounds__(256) warp_fwd_kernel(WarpArgs a, float* __restrict__ out) {
  const int64_t n = (int64_t)a.X * a.Y * a.Z;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n * a.B) return;
  const int b = (int)(gid / n);
  const int64_t vox = gid - (int64_t)b * n;
  const int z = (int)(vox % a.Z);
  const int y = (int)((vox / a.Z) % a.Y);
  const int x = (int)(vox / ((int64_t)a.Z * a.Y));
  float cx, cy, cz;
  coords_at<KIND>(a, b, x, y, z, vox, cx, cy, cz);
  Tri t; Axis ax, ay, az;
  tri_setup(cx, cy, cz, a.X, a.Y, a.Z, t, ax, ay, az);
  const float* src = a.src + (a.src_batched ? (int64_t)b * n * a.C : 0);
  float* o = out + gid * a.C;
  if (a.C == 1 && a.Z >= 2) {   // scalar volume: x-corner pairs from 8-byte loads
    o[0] = tri_sample_pairs(src, a.Y, a.Z, ax, ay, az);
    return;
  }
  for (int c = 0; c < a.C; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += t.w[k] * src[t.o[k] * a.C + c];
    o[c] = s;
  }
}

// adjoint: g_src += scatter(g_out) (float atomics), g_coord written (explicit: [B,3,X,Y,Z];
// advect: g_vel [X,Y,Z,3] = -g_coord).
template <int KIND>
__global__ void __launch_bounds__(256) warp_bwd_kernel(WarpArgs a, const float* __restrict__ g_out,
                                                       float* __restrict__ g_src, float* __restrict__ g_coord) {
  const int64_t n = (int64_t)a.X * a.Y * a.Z;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= n * a.B) return;
  const int b = (int)(gid / n);
  const int64_t vox = gid - (int64_t)b * n;
  const int z = (int)(vox % a.Z);
  const int y = (int)((vox / a.Z) % a.Y);
  const int x = (int)(vox / ((int64_t)a.Z * a.Y));
  float cx, cy, cz;
  coords_at<KIND>(a, b, x, y, z, vox, cx, cy, cz);
  Tri t; Axis ax, ay, az;
  tri_setup(cx, cy, cz, a.X, a.Y, a.Z, t, ax, ay, az);
  const int64_t boff = a.src_batched ? (int64_t)b * n * a.C : 0;
  const float* go = g_out + gid * a.C;
  float gx = 0.f, gy = 0.f, gz = 0.f;
  const float wx[2] = {1.f - ax.w1, ax.w1}, wy[2] = {1.f - ay.w1, ay.w1}, wz[2] = {1.f - az.w1, az.w1};
  for (int c = 0; c < a.C; ++c) {
    const float g = go[c];
    if (g_src) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float contrib = t.w[k] * g;
        if (contrib != 0.f) atomicAdd(g_src + boff + t.o[k] * a.C + c, contrib);
      }
    }
    if (g_coord) {
      const float* src = a.src + boff;
      float v[8];
      if (a.C == 1 && a.Z >= 2) {
        tri_gather_pairs(src, a.Y, a.Z, ax, ay, az, v);
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = src[t.o[k] * a.C + c];
      }
      // k = a*4 + b*2 + c  (x,y,z bits)
      const float dx = wy[0] * wz[0] * (v[4] - v[0]) + wy[0] * wz[1] * (v[5] - v[1]) +
                       wy[1] * wz[0] * (v[6] - v[2]) + wy[1] * wz[1] * (v[7] - v[3]);
      const float dy = wx[0] * wz[0] * (v[2] - v[0]) + wx[0] * wz[1] * (v[3] - v[1]) +
                       wx[1] * wz[0] * (v[6] - v[4]) + wx[1] * wz[1] * (v[7] - v[5]);
      const float dz = wx[0] * wy[0] * (v[1] - v[0]) + wx[0] * wy[1] * (v[3] - v[2]) +
                       wx[1] * wy[0] * (v[5] - v[4]) + wx[1] * wy[1] * (v[7] - v[6]);
      gx += g * dx;
      gy += g * dy;
      gz += g * dz;
    }
  }
  if (g_coord) {
    gx *= (float)(a.X - 1) * 0.5f;
    gy *= (float)(a.Y - 1) * 0.5f;
    gz *= (float)(a.Z - 1) * 0.5f;
    if (KIND == COORD_ADVECT) {
      float* gv = g_coord + vox * 3;
      gv[0] = -gx; gv[1] = -gy; gv[2] = -gz;
    } else {
      float* gc = g_coord + (int64_t)b * 3 * n;
      gc[vox] = gx; gc[n + vox] = gy; gc[2 * n + vox] = gz;
    }
  }
}


// ---- advect, scalar field (the hot case) --------------------------------------------------------
// The generic kernel keeps one voxel per thread in flight and is bound by latency x occupancy
// (~1.9 TB/s).  Here a thread owns 4 W-consecutive voxels: the 12 velocity floats arrive as three
// float4 loads, the 16 x-corner pairs as 8-byte loads, all issued before use, 32-bit indexing.
// Scalar-field advect, 4 W-consecutive voxels per thread, lean stencil: the back-traced voxel coordinate is
// x_a = index_a - vel_a * (n_a - 1)/2 (one FMA; lin_coord(i) - vel mapped to voxel space), border replication by
// clamping it to [0, n-1], base cell min(floor, n-2), weight in [0,1]; the four row-pairs of the stencil are
// dword-aligned 8-byte loads.  D, H, W >= 2.  The first form (per-corner index clamps, two runtime integer
// divisions per voxel) spent ~150 VALU instructions per voxel on a 20-byte-per-voxel stream.
// adv_next (nullable, MODE 2): advect(d, UPDATED vel) of the same voxels -- the next iteration's forward sample, formed
// while the new velocity is still in registers (advect reads the velocity of its own voxel only; the gathered density is
// constant): the forward advect launch of the next iteration and its 96 MB velocity read disappear.  Same arithmetic
// as MODE 0 on the stored velocity: bit-identical to running nfs_advect_fwd afterwards.
struct AdamFused { float* m; float* v; float lr_t, b1, b2, eps; float* adv_next = nullptr;
                   unsigned long long* live = nullptr; unsigned long long* ever = nullptr; };

// (the lean stencil -- corners_differ, lean_dims / lean_cell / lean_gather / lean_sample / lean_grad -- and the lane
// layout -- walk64, lane_first, lane_start -- are advect_stencil.h: libnfs_descent.so forms the same samples from them)

// MODE 0: forward; 1: velocity gradient -> out; 2: velocity gradient consumed on the spot by the TF-Adam update of
// the velocity itself (vel, m, v updated in place: every thread reads and writes only its own 4 voxels of them;
// the 96 MB gradient never goes to HBM)
// Slab form (zoff, Dfull): vel / g_out / out / the moments hold only the D planes [zoff, zoff + D) of a volume of Dfull
// planes, d is the WHOLE density (the back-traced points leave the slab); zoff = 0, Dfull = D is the whole volume.
// EVER (MODE 2 + LIVE, volumes below 2^31 / 12 voxels): ad.ever is set and the streamed accesses are predicated per lane
// SRC (other than SRC_VEL: MODE 0 / 1, whole volumes): vel is a stream function [D,H,W,3], a potential [D,H,W] or a
// Helmholtz variable [D,H,W,4] and the velocity is source_velocity<SRC>() of it (source_ops.h), formed in registers and never
// stored; everything after the fetch is the same code
template <int MODE, bool LIVE = false, bool EVER = false, int SRC = SRC_VEL>   // LIVE: ad.live is set (a compile-time switch: the mask code out of the plain kernels)
__global__ void __launch_bounds__(256) advect1_kernel(const float* __restrict__ d, const float* vel,
                                                      const float* __restrict__ g_out, float* out,
                                                      int D, int H, int W, AdamFused ad, int zoff, int Dfull) {
  constexpr bool BWD = MODE != 0;
  const int n = D * H * W;
  // a wave owns 256 consecutive voxels: lane l takes l, l+64, l+128, l+192 (768- or 256-byte runs per instruction).
  // Per-XCD order not for the fused Adam variant: it is dominated by the streamed moments, and eight distant streams
  // measured slower than one front, 0.128 vs 0.112 ms.
  const int lane = threadIdx.x & 63, first = lane_first<4, MODE != 2>(blockDim.x, lane);
  if (first - lane >= n) return;
  [[maybe_unused]] unsigned long long ew[4] = {~0ull, ~0ull, ~0ull, ~0ull};
  if constexpr (MODE == 2 && LIVE) {
    // `ever` (nullable): bit i = voxel i has been live in SOME iteration since the Adam moments were zeroed.  Where it never
    // was, every velocity gradient so far was an exact zero: m = v = +0, and this iteration's is zero again when the
    // CURRENT mask (`live` on entry: the mask of the forward sample this gradient belongs to) has the bit clear too --
    // ApplyAdam then leaves m, v and the velocity exactly as they are (b1 0 + (1 - b1) (+-0) = +0, x - lr 0 / (0 + eps) = x),
    // so the next forward sample and its mask bit do not change either.  A wave whose 256 voxels are all like that has
    // nothing to read and nothing to write: it returns here.  (Everything else runs the unchanged path: bit-identical.)
    if (ad.ever) {
      const int wbase = __builtin_amdgcn_readfirstlane(first - lane);
      unsigned long long any = 0ull;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = wbase + 64 * j;
        ew[j] = 0ull;
        if (b < n) {
          const unsigned long long e0 = ad.ever[b >> 6], e = e0 | ad.live[b >> 6];
          if (e != e0 && lane == 0) ad.ever[b >> 6] = e;
          any |= e;
          ew[j] = e;
        }
      }
      if (any == 0ull) return;
    }
  }
  // EVER: in a wave that runs, the lanes whose voxel never was live take part in nothing either -- their streamed loads
  // get an offset beyond the buffer (the hardware answers zeros without touching memory: exactly what m and v hold
  // there), their stores likewise, their mask bit stays clear.  Traffic then follows the ever-live cache lines, not the
  // ever-live waves.
  [[maybe_unused]] bool act[4] = {true, true, true, true};
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t vel_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(vel), 0, EVER ? (uint32_t)n * 12u : 0u, 0x00020000);
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t m_rs = __builtin_amdgcn_make_buffer_rsrc(ad.m, 0, EVER ? (uint32_t)n * 12u : 0u, 0x00020000);
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t u_rs = __builtin_amdgcn_make_buffer_rsrc(ad.v, 0, EVER ? (uint32_t)n * 12u : 0u, 0x00020000);
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t g_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g_out), 0, EVER ? (uint32_t)n * 4u : 0u, 0x00020000);
  [[maybe_unused]] const __amdgpu_buffer_rsrc_t adv_rs = __builtin_amdgcn_make_buffer_rsrc(ad.adv_next, 0, EVER ? (uint32_t)n * 4u : 0u, 0x00020000);
  typedef unsigned u32x3_t __attribute__((ext_vector_type(3)));
  [[maybe_unused]] auto ld3 = [](__amdgpu_buffer_rsrc_t r, uint32_t o) {
    const u32x3_t q = __builtin_amdgcn_raw_buffer_load_b96(r, o, 0, 0);
    return F3u{__uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z)};
  };
  [[maybe_unused]] auto st3 = [](F3u f, __amdgpu_buffer_rsrc_t r, uint32_t o) {
    const u32x3_t q = {__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z)};
    __builtin_amdgcn_raw_buffer_store_b96(q, r, o, 0, 0);
  };
  const F3u* v3 = reinterpret_cast<const F3u*>(vel);
  const F3u* m3 = reinterpret_cast<const F3u*>(ad.m);
  const F3u* u3 = reinterpret_cast<const F3u*>(ad.v);
  F3u vv[4], mm[4], uu[4];
  float gg[4];
  bool ok[4];
  [[maybe_unused]] int ws, hs, zs;   // SRC: the voxel positions, walked here as well (walk64 keeps them inside the volume)
  if constexpr (SRC != SRC_VEL) lane_start(first, n, H, W, ws, hs, zs);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = first + 64 * j;
    ok[j] = idx < n;
    const int ic = ok[j] ? idx : n - 1;
    if constexpr (SRC != SRC_VEL) {
      static_assert(SRC == SRC_VEL || MODE != 2, "the updates are nfs_stream_bwd_adam / nfs_potential_bwd_adam / nfs_helmholtz_bwd_adam");
      vv[j] = source_velocity<SRC>(vel, (size_t)(unsigned)(zs * H + hs) * (unsigned)W + (unsigned)ws, zs, hs, ws, D, H, W);
      if (BWD) gg[j] = g_out[ic];
      walk64(ws, hs, zs, W, H, D - 1);
      continue;
    }
    if constexpr (EVER) {
      act[j] = ok[j] && ((ew[j] >> lane) & 1ull);
      const uint32_t o12 = act[j] ? (uint32_t)idx * 12u : 0x80000000u, o4 = act[j] ? (uint32_t)idx * 4u : 0x80000000u;
      vv[j] = ld3(vel_rs, o12);
      gg[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(g_rs, o4, 0, 0));
      mm[j] = ld3(m_rs, o12);
      uu[j] = ld3(u_rs, o12);
      continue;
    }
    vv[j] = v3[ic];
    if (BWD) gg[j] = g_out[ic];
    if (MODE == 2) {   // the Adam moments are streamed: ask for them with the velocity, before the gather
      mm[j] = m3[ic];
      uu[j] = u3[ic];
    }
  }
  const LeanDims dm = lean_dims(Dfull, H, W);
  int w, h, z;
  lane_start(first, n, H, W, w, h, z);
  z += zoff;
  const int zlast = zoff + D - 1;
  F2u p[4][4];
  float wz[4], wy[4], wx[4], mz[4], my[4], mx[4];
  [[maybe_unused]] const int w0 = w, h0 = h, z0 = z;   // MODE 2 with adv_next: the walk is repeated for the second sample
  [[maybe_unused]] unsigned ob[4];                    // ... and the base cell of the first sample is remembered
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const LeanCell c = lean_cell(vv[j], z, h, w, dm);
    wz[j] = c.wz; wy[j] = c.wy; wx[j] = c.wx;
    if (BWD) {   // outside the volume both clipped corners coincide: no dependence on the coordinate
      mz[j] = (c.xz >= 0.f && c.xz < dm.nz1) ? dm.hz : 0.f;
      my[j] = (c.xy >= 0.f && c.xy < dm.ny1) ? dm.hy : 0.f;
      mx[j] = (c.xx >= 0.f && c.xx < dm.nx1) ? dm.hx : 0.f;
    }
    if (MODE == 2) ob[j] = c.o;
    lean_gather(d, c.o, dm, p[j]);
    walk64(w, h, z, W, H, zlast);
  }
  if (!BWD) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ok[j]) out[first + 64 * j] = lean_sample(p[j], wx[j], wy[j], wz[j]);
      if constexpr (LIVE) {
        const unsigned long long lv = __ballot(ok[j] && corners_differ(p[j]));
        if (lane == 0 && first + 64 * j < n) ad.live[(first + 64 * j) >> 6] = lv;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float e[4], a[4];
      lean_rows(p[j], wx[j], e, a);
      // d(sample)/d(coordinate) along each axis: difference of the two faces, interpolated in the other two
      const float f0 = fmaf(wy[j], e[1] - e[0], e[0]), f1 = fmaf(wy[j], e[3] - e[2], e[2]);
      const float dx = fmaf(wz[j], f1 - f0, f0);
      const float g0 = a[1] - a[0], g1 = a[3] - a[2];
      const float dy = fmaf(wz[j], g1 - g0, g0);
      const float b0 = fmaf(wy[j], g0, a[0]), b1 = fmaf(wy[j], g1, a[2]);
      const float dz = b1 - b0;
      // coordinate = index - vel * (n-1)/2  =>  d/dvel = -(n-1)/2 * d/dcoordinate (mz/my/mx carry the factor)
      const float gv[3] = {-gg[j] * dz * mz[j], -gg[j] * dy * my[j], -gg[j] * dx * mx[j]};
      const int idx = first + 64 * j;
      if (MODE == 1) {
        if (ok[j]) reinterpret_cast<F3u*>(out)[idx] = F3u{gv[0], gv[1], gv[2]};
      } else {
        // TF ApplyAdam, same arithmetic as adam_kernel (field.hip); out == vel
        float xs[3] = {vv[j].x, vv[j].y, vv[j].z}, ms[3] = {mm[j].x, mm[j].y, mm[j].z},
              us[3] = {uu[j].x, uu[j].y, uu[j].z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          ms[c] = ad.b1 * ms[c] + (1.f - ad.b1) * gv[c];
          us[c] = ad.b2 * us[c] + (1.f - ad.b2) * gv[c] * gv[c];
          xs[c] -= ad.lr_t * ms[c] / (sqrtf(us[c]) + ad.eps);
        }
        vv[j] = F3u{xs[0], xs[1], xs[2]};
        if constexpr (EVER) {
          const uint32_t o12 = act[j] ? (uint32_t)idx * 12u : 0x80000000u;
          st3(vv[j], vel_rs, o12);
          st3(F3u{ms[0], ms[1], ms[2]}, m_rs, o12);
          st3(F3u{us[0], us[1], us[2]}, u_rs, o12);
        } else if (ok[j]) {
          reinterpret_cast<F3u*>(out)[idx] = vv[j];
          reinterpret_cast<F3u*>(ad.m)[idx] = F3u{ms[0], ms[1], ms[2]};
          reinterpret_cast<F3u*>(ad.v)[idx] = F3u{us[0], us[1], us[2]};
        }
      }
    }
    if (MODE == 2 && ad.adv_next) {
      // the next iteration's forward sample from the updated velocity (MODE 0's on it; the voxel indices are walked
      // again rather than kept: twelve registers more cost the kernel a wave per SIMD)
      w = w0; h = h0; z = z0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const LeanCell c = lean_cell(vv[j], z, h, w, dm);
        wz[j] = c.wz; wy[j] = c.wy; wx[j] = c.wx;
        // One Adam step moves the back-traced point by a fraction of a cell: its base cell is almost always the one the
        // adjoint just gathered, whose eight corners are still in registers -- only the weights change.  The second
        // gather (a further memory round trip in every wave's life: 0.128 -> 0.166 ms when it was unconditional) is
        // taken only by the lanes whose point crossed a cell face.
        if (c.o != ob[j]) lean_gather(d, c.o, dm, p[j]);
        walk64(w, h, z, W, H, zlast);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float s = lean_sample(p[j], wx[j], wy[j], wz[j]);
        if constexpr (EVER)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, s), adv_rs,
                                                act[j] ? (uint32_t)(first + 64 * j) * 4u : 0x80000000u, 0, 0);
        else if (ok[j]) ad.adv_next[first + 64 * j] = s;
        if constexpr (LIVE) {
          const unsigned long long lv = __ballot(ok[j] && (!EVER || act[j]) && corners_differ(p[j]));
          if (lane == 0 && first + 64 * j < n) ad.live[(first + 64 * j) >> 6] = lv;
        }
      }
    }
  }
}


// ---- one step of _transport (styler_base.py:59-89) fused with the temporal filter's accumulation -------------------
// out = w_g * advect(g, scale * u) + w_add * addend   for a C-channel grid field g [D,H,W,C] (C = 3: the stylisation
// velocity, C = 1: a density), u [D,H,W,3] the simulation velocity of the frame being crossed (scale = +1 forwards,
// -1 backwards, +-|b-a| for the one-step form).  HBM-bound: reads u (12 B), gathers g (4C B compulsory), reads the
// addend (4C B), writes out (4C B) per voxel.  A wave owns 128 consecutive voxels, lane l takes l and l+64 (every
// streamed 12-byte vector access is one contiguous run per instruction); lean stencil as in advect1_kernel; the two
// W-adjacent corners of a row come from one 8C-byte access (dword-aligned dwordx2 / two dwordx3).
template <int C> struct __attribute__((packed, aligned(4))) Vec { float v[C]; };

template <int C>
__global__ void __launch_bounds__(256) transport_step_kernel(const float* __restrict__ g, const float* __restrict__ u,
                                                             const float* __restrict__ addend, float* __restrict__ out,
                                                             int D, int H, int W, float scale, float w_g, float w_add) {
  constexpr int NV = 2;
  const int n = D * H * W;
  const int lane = threadIdx.x & 63, first = lane_first<NV, true>(blockDim.x, lane);
  if (first - lane >= n) return;
  const F3u* u3 = reinterpret_cast<const F3u*>(u);
  const Vec<C>* gC = reinterpret_cast<const Vec<C>*>(g);
  F3u vv[NV];
  Vec<C> add[NV];
  bool ok[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int idx = first + 64 * j;
    ok[j] = idx < n;
    const int ic = ok[j] ? idx : n - 1;
    vv[j] = u3[ic];
    if (addend) add[j] = reinterpret_cast<const Vec<C>*>(addend)[ic];
  }
  LeanDims dm = lean_dims(D, H, W);
  dm.hz *= scale; dm.hy *= scale; dm.hx *= scale;     // the back-trace runs along scale * u
  int w, h, z;
  lane_start(first, n, H, W, w, h, z);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const LeanCell cell = lean_cell(vv[j], z, h, w, dm);
    Vec<C> lo[4], hi[4];
    lean_gather(gC, cell.o, dm, lo, hi);
    Vec<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const F2u p[4] = {{lo[0].v[c], hi[0].v[c]}, {lo[1].v[c], hi[1].v[c]}, {lo[2].v[c], hi[2].v[c]}, {lo[3].v[c], hi[3].v[c]}};
      float s = w_g * lean_sample(p, cell.wx, cell.wy, cell.wz);
      if (addend) s = fmaf(w_add, add[j].v[c], s);
      r.v[c] = s;
    }
    if (ok[j]) reinterpret_cast<Vec<C>*>(out)[first + 64 * j] = r;
    walk64(w, h, z, W, H, D - 1);
  }
}

// generic channel count (and degenerate volumes): one thread per voxel on the exact reference stencil
__global__ void __launch_bounds__(256) transport_step_generic_kernel(const float* __restrict__ g,
                                                                     const float* __restrict__ u,
                                                                     const float* __restrict__ addend,
                                                                     float* __restrict__ out, int D, int H, int W, int C,
                                                                     float scale, float w_g, float w_add) {
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  const float* v = u + vox * 3;
  Tri t; Axis az, ay, ax;
  tri_setup(lin_coord(z, D) - scale * v[0], lin_coord(y, H) - scale * v[1], lin_coord(x, W) - scale * v[2], D, H, W, t,
            az, ay, ax);
  for (int c = 0; c < C; ++c) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += t.w[k] * g[t.o[k] * C + c];
    s *= w_g;
    if (addend) s = fmaf(w_add, addend[vox * C + c], s);
    out[vox * C + c] = s;
  }
}

// ---- output-stationary adjoint of rotate for C = 1 -------------------------------------------
// Global float atomics cap the scatter at ~90 G atomics/s (5.6 ms for 8 views of 200^3), and LDS float
// atomics are no better: measured on gfx950 (tools/lds_atomic_bench.hip) ds_add_f32 sustains 0.33
// lanes/clk/CU while ds_add_u64 runs at 9.4.  So the tile accumulates in 64-bit FIXED POINT:
// contributions are scaled by 2^k, with k chosen from max|g_out| (a streaming pre-pass) so that no voxel
// sum can overflow; with ~49 bits below the largest value this is more accurate than f32 accumulation and,
// integer adds being associative, bit-reproducible.
// A block owns RT_TZ x RT_TY x RT_TX voxels of g_d and keeps them, plus a one-cell halo on every side, in
// LDS as 64-bit fixed-point accumulators (LDS float atomics run at 1/40 of the integer rate on gfx950).
// It walks, view by view, the output-lattice rows that cross its catchment (the samples whose base cell
// lies in [tile_lo - 1, tile_hi]), each row clipped to the exact x-interval; a sample in the catchment adds
// all 8 corners with compile-time LDS offsets and no per-corner tests (the halo absorbs the corners that
// belong to neighbouring tiles; only the owned cells are written back).  No global atomics; the integer
// sums make the result independent of the traversal order.
#ifndef NFS_RT_TZ
// (tile shape x lanes per lattice row swept on 8 views of 200^3, tools/rot_tile_sweep.sh: 14x12x40 x 8 0.331 ms, x 4 0.305,
// x 2 0.357, x 16 0.42; 14x14x34 x 4 0.296; 16x12x34 x 4 0.307; 10x10x40 x 4 0.324; 12x12x48 x 4 0.41 (240-wide for 200);
// the lattice rows of one (tile, view) are ~20 samples long on average and many are much shorter, so narrow groups
// idle less in the row tails)
#define NFS_RT_TZ 14
#define NFS_RT_TY 14
#define NFS_RT_TX 34
#define NFS_RT_GROUP 4
#endif
constexpr int RT_TZ = NFS_RT_TZ, RT_TY = NFS_RT_TY, RT_TX = NFS_RT_TX;
constexpr int RT_LZ = RT_TZ + 2, RT_LY = RT_TY + 2, RT_LX = RT_TX + 2;
#ifndef NFS_RT_THREADS
#define NFS_RT_THREADS 1024
#endif
constexpr int RT_THREADS = NFS_RT_THREADS;
constexpr int RT_GROUP = NFS_RT_GROUP;   // lanes that share one lattice row
constexpr int RT_VMAX = 32;   // views per launch (host loops over chunks)
static_assert(RT_THREADS / 2 >= RT_VMAX, "the per-view weight check runs on lanes RT_THREADS / 2 + v");

struct ViewRows {             // per (block, view), in LDS
  // voxel-space sample coordinate of axis a at lattice point (oz,oy,ox): c + a0*oz + a1*oy + s*ox
  float a0[3], a1[3], s[3], inv_s[3], c[3];
  float lo[3], hi[3];         // catchment (padded) in voxel space
  float wextra;               // weight bound of this view beyond the launcher's 4*nmax (0 for a rotation)
  int z_lo, y_lo, x_lo, x_hi, ey, rows;
  unsigned my;                // ceil(2^32 / ey)
};

// max |x| over n floats -> *out (as float bits; non-negative floats order like unsigned ints)
__global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ x, int64_t n, unsigned* out) {
  __shared__ float red[16];
  float m = 0.f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(x + i);
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    } else {
      for (int64_t j = i; j < n; ++j) m = fmaxf(m, fabsf(x[j]));
    }
  }
  m = block_max(m, red);
  if (threadIdx.x == 0 && m > 0.f) atomicMax(out, __float_as_uint(fminf(m, 3.0e38f)));
}

// catchment of one (tile, view).  One lane per view runs this while the other 1023 threads of the block wait, so its
// latency is a fixed cost of every block (measured in round 4, tools/render_family_by_views.py: the kernel took
// 42 us + 30 us per view at 200^3 -- the first version of this function, 21 double-precision divisions and 148 bytes of
// scratch under the kernel's 64-register cap, was most of the 42).  Now: double precision where it sets the floats the
// sample loop reads (A, c, 1 / A[a][2]: bit-identical to before), one reciprocal of the determinant for the lattice box
// (a bound, padded by 0.05 cells), every array fully unrolled and the outputs stored as soon as they are final: inlined
// it fits the 64 registers without scratch (out of line the ABI's callee-saved registers alone cost 16 scratch round
// trips).  200^3: 71.8 -> 62.6 us at one view, 278.7 -> 271.5 at eight, bit-identical; with the sample loop compiled out
// the kernel (zero fill of the accumulators, this function, write-back) takes 16.7 us, of which this function 1.3.
__device__ __forceinline__ void rotate_tile_catchment(const float* r, int D, int H, int W, int z0, int y0,
                                                                 int x0, int z1, int y1, int x1, ViewRows* out) {
  const int n[3] = {D, H, W};
  const int tlo[3] = {z0, y0, x0}, thi[3] = {z1, y1, x1};
  float rr[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) rr[i] = r[i];
  double sb[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) sb[b] = n[b] > 1 ? 2.0 / (n[b] - 1) : 0.0;
  // cmin/cmax: the range the (unclamped) sample coordinate of axis a takes over the whole output lattice;
  // a border tile also catches the samples clamped onto it, so its catchment extends to that range
  double A[3][3], mid[3], half[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double ha = 0.5 * (n[a] - 1);
    double rs = 0.0, mn = 0.0, mx = 0.0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      A[a][b] = (double)rr[a * 3 + b] * sb[b] * ha;
      rs += (double)rr[a * 3 + b];
      mn += fmin(A[a][b] * (n[b] - 1), 0.0);
      mx += fmax(A[a][b] * (n[b] - 1), 0.0);
    }
    const double c = (1.0 - rs) * ha;
    // base cell floor(u) in [tlo-1, thi]  <=>  u in [tlo-1, thi+1); 0.05-cell pad covers the float evaluation
    const double xl = (tlo[a] == 0) ? fmin(c + mn - 0.5, -1.05) : tlo[a] - 1.05;
    const double xh = (thi[a] == n[a] - 1) ? fmax(c + mx + 0.5, n[a] + 0.05) : thi[a] + 1.05;
    mid[a] = 0.5 * (xl + xh) - c;
    half[a] = 0.5 * (xh - xl);
    out->a0[a] = (float)A[a][0];
    out->a1[a] = (float)A[a][1];
    out->s[a] = (float)A[a][2];
    out->inv_s[a] = fabs(A[a][2]) > 1e-6 ? (float)(1.0 / A[a][2]) : 0.f;
    out->c[a] = (float)c;
    out->lo[a] = (float)xl;
    out->hi[a] = (float)xh;
  }
  const double k00 = A[1][1] * A[2][2] - A[1][2] * A[2][1], k01 = A[0][2] * A[2][1] - A[0][1] * A[2][2],
               k02 = A[0][1] * A[1][2] - A[0][2] * A[1][1];
  const double det = A[0][0] * k00 + A[1][0] * k01 + A[2][0] * k02;
  int lo[3] = {0, 0, 0}, hi[3] = {D - 1, H - 1, W - 1};
  if (fabs(det) > 1e-9) {
    const double rd = 1.0 / det;
    // row b of the inverse = cofactors / det; box centre / half widths in voxel space -> centre / half extents in
    // lattice space (the reciprocal instead of nine divisions moves the box by ~1e-13 cells: it is a padded bound)
    double iv[3][3];
    iv[0][0] = k00; iv[0][1] = k01; iv[0][2] = k02;
    iv[1][0] = A[1][2] * A[2][0] - A[1][0] * A[2][2];
    iv[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0];
    iv[1][2] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    iv[2][0] = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    iv[2][1] = A[0][1] * A[2][0] - A[0][0] * A[2][1];
    iv[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double oc = (iv[b][0] * mid[0] + iv[b][1] * mid[1] + iv[b][2] * mid[2]) * rd;
      const double oe = (fabs(iv[b][0]) * half[0] + fabs(iv[b][1]) * half[1] + fabs(iv[b][2]) * half[2]) * fabs(rd) + 1e-9;
      lo[b] = (int)fmin(fmax(floor(oc - oe), 0.0), (double)n[b]);
      hi[b] = (int)fmax(fmin(ceil(oc + oe), (double)(n[b] - 1)), -1.0);
    }
  }
  const int ez = max(hi[0] - lo[0] + 1, 0), ey = max(hi[1] - lo[1] + 1, 0);
  out->z_lo = lo[0]; out->y_lo = lo[1]; out->x_lo = lo[2]; out->x_hi = hi[2];
  out->ey = ey;
  out->rows = hi[2] >= lo[2] ? ez * ey : 0;
  out->my = ey > 1 ? 0xFFFFFFFFu / (unsigned)ey + 1u : 0u;     // ceil(2^32 / ey), ey >= 2
}

// The launcher's fixed-point bound allows 4*nmax summed weight per view on one voxel, which holds for a rotation.  Any
// other matrix may put more there (a scale clamps a whole corner region onto one voxel, a shrink stacks samples), up to
// one unit per sample of the view: such a view adds D*H*W.  R^T R is formed from the floats the kernel reads.  (Run by
// other lanes than the catchment's: inside rotate_tile_catchment it pushes that function into scratch.)
__device__ __forceinline__ float rotate_view_extra_weight(const float* r, int D, int H, int W) {
  bool rigid = true;
#pragma unroll
  for (int b = 0; b < 3; ++b)
#pragma unroll
    for (int c = b; c < 3; ++c) {
      const double e = (double)r[b] * r[c] + (double)r[3 + b] * r[3 + c] + (double)r[6 + b] * r[6 + c];
      rigid = rigid && fabs(e - (b == c ? 1.0 : 0.0)) <= 1e-4;
    }
  return rigid ? 0.f : (float)((double)D * H * W);
}

// ---- which tiles, and how much of each, a live-mask launch accumulates ------------------------------------------------
// live (nfs_advect_*_live): bit (z H + y) W + x set = the velocity gradient of voxel (z, y, x) can be non-zero.  The
// linear stencil between the rotate adjoint's g_d and the advect adjoint (the smoothing) reads g_d within `dil` cells of
// such a voxel, and nothing else of g_d is ever multiplied by a non-zero: a tile needs the sums of the bounding box of
// its voxels within `dil` of a live voxel, no more.  One wave per tile finds that box; a second, one-block launch sorts
// the tiles by decreasing work into `order` -- the hardware starts blocks in index order, and with boxes of very
// different sizes (and two fifths of the tiles empty on a smoke density) the long ones must not start last.
// Workspace (ints): [LWS_BOXES + 8 t ...] box of tile t = (z0, z1, y0, y1, x0, x1, work, -), [LWS_ORDER(ntiles) + i] the
// tile block i of the adjoint takes.
constexpr int LWS_BOXES = 8;
#define LWS_ORDER(ntiles) (nfs::LWS_BOXES + 8 * (ntiles))
constexpr int LB_THREADS = 1024, LB_WAVES = LB_THREADS / 64, LB_CLASSES = 64;

// a WAVE per tile, four (z, y) rows of the tile's dilated box per lane
__global__ void __launch_bounds__(LB_THREADS) rotate_live_boxes_kernel(const unsigned long long* __restrict__ live, int D,
                                                                       int H, int W, int tiles_y, int tiles_x, int dil,
                                                                       int ntiles, int* __restrict__ ws) {
  const int t = threadIdx.x, lane = t & 63;
  const int tile = blockIdx.x * LB_WAVES + (t >> 6);
  if (tile < ntiles) {
    const int bx = tile % tiles_x, by = (tile / tiles_x) % tiles_y, bz = tile / (tiles_x * tiles_y);
    const int Tz0 = bz * RT_TZ, Ty0 = by * RT_TY, Tx0 = bx * RT_TX;
    const int Tz1 = min(Tz0 + RT_TZ, D) - 1, Ty1 = min(Ty0 + RT_TY, H) - 1, Tx1 = min(Tx0 + RT_TX, W) - 1;
    const int ez0 = max(Tz0 - dil, 0), ez1 = min(Tz1 + dil, D - 1), ey0 = max(Ty0 - dil, 0), ey1 = min(Ty1 + dil, H - 1);
    const int ex0 = max(Tx0 - dil, 0), ex1 = min(Tx1 + dil, W - 1);
    const int nry = ey1 - ey0 + 1, len = ex1 - ex0 + 1, nrows = (ez1 - ez0 + 1) * nry;   // len <= RT_TX + 2 dil <= 63
    int b0 = 0x7fffffff, b1 = -1, b2 = 0x7fffffff, b3 = -1, b4 = 0x7fffffff, b5 = -1;
    for (int r = lane; r < nrows; r += 64) {
      const int rz = ez0 + r / nry, ry = ey0 + r % nry;
      const int64_t bit0 = ((int64_t)rz * H + ry) * W + ex0;
      const int sh = (int)(bit0 & 63);
      unsigned long long bits = live[bit0 >> 6] >> sh;
      if (sh + len > 64) bits |= live[(bit0 >> 6) + 1] << (64 - sh);
      bits &= (1ull << len) - 1ull;
      if (bits) {
        b0 = min(b0, rz); b1 = max(b1, rz); b2 = min(b2, ry); b3 = max(b3, ry);
        b4 = min(b4, ex0 + (int)__builtin_ctzll(bits)); b5 = max(b5, ex0 + 63 - (int)__builtin_clzll(bits));
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      b0 = min(b0, __shfl_xor(b0, o, 64)); b1 = max(b1, __shfl_xor(b1, o, 64));
      b2 = min(b2, __shfl_xor(b2, o, 64)); b3 = max(b3, __shfl_xor(b3, o, 64));
      b4 = min(b4, __shfl_xor(b4, o, 64)); b5 = max(b5, __shfl_xor(b5, o, 64));
    }
    if (lane == 0) {
      int* b = ws + LWS_BOXES + tile * 8;
      int work = 0;
      int z0 = Tz0, z1 = Tz1, y0 = Ty0, y1 = Ty1, x0 = Tx0, x1 = Tx1;
      if (b1 >= 0) {
        z0 = max(Tz0, b0 - dil); z1 = min(Tz1, b1 + dil);
        y0 = max(Ty0, b2 - dil); y1 = min(Ty1, b3 + dil);
        x0 = max(Tx0, b4 - dil); x1 = min(Tx1, b5 + dil);
        // samples whose base cell lies in [lo - 1, hi] per axis; a box on the volume's border also catches the samples
        // clamped onto it (a few cells' worth at these view angles)
        const int cz = z1 - z0 + 2 + (z0 == 0 ? 6 : 0) + (z1 == D - 1 ? 6 : 0);
        const int cy = y1 - y0 + 2 + (y0 == 0 ? 6 : 0) + (y1 == H - 1 ? 6 : 0);
        const int cx = x1 - x0 + 2 + (x0 == 0 ? 6 : 0) + (x1 == W - 1 ? 6 : 0);
        work = cz * cy * cx;
      }
      b[0] = z0; b[1] = z1; b[2] = y0; b[3] = y1; b[4] = x0; b[5] = x1; b[6] = work; b[7] = 0;
    }
  }
}

// ... and the tiles by decreasing work: one block, counting sort by work class (a launch of its own: the boxes come from
// 85 blocks on all XCDs, and a ticket + __threadfence() in their kernel -- the "last block sorts" form this replaced --
// cost 30 us of cache maintenance; a kernel boundary costs 3)
__global__ void __launch_bounds__(LB_THREADS) rotate_live_order_kernel(int ntiles, int* __restrict__ ws) {
  __shared__ int hist[LB_CLASSES + 1];
  const int t = threadIdx.x;
  const int* boxes = ws + LWS_BOXES;
  constexpr int WMAX = (RT_TZ + 13) * (RT_TY + 13) * (RT_TX + 13);
  for (int i = t; i <= LB_CLASSES; i += LB_THREADS) hist[i] = 0;
  __syncthreads();
  auto cls = [](int work) {   // 0 = most work ... LB_CLASSES - 1 = least, LB_CLASSES = none
    return work == 0 ? LB_CLASSES : LB_CLASSES - 1 - min((int)(((int64_t)work * LB_CLASSES) / (WMAX + 1)), LB_CLASSES - 1);
  };
  constexpr int PER = 4;                                   // tiles per thread and round (4096 per round)
  int* order = ws + LWS_ORDER(ntiles);
  int done = 0;                                            // tiles placed by earlier rounds (volumes of > 4096 tiles)
  for (int base = 0; base < ntiles; base += PER * LB_THREADS) {
    int c[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = base + j * LB_THREADS + t;
      c[j] = i < ntiles ? cls(boxes[i * 8 + 6]) : -1;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) if (c[j] >= 0) atomicAdd(&hist[c[j]], 1);
    __syncthreads();
    if (t == 0) {
      int run = done;
      for (int k = 0; k <= LB_CLASSES; ++k) { const int n = hist[k]; hist[k] = run; run += n; }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PER; ++j) if (c[j] >= 0) order[atomicAdd(&hist[c[j]], 1)] = base + j * LB_THREADS + t;
    __syncthreads();
    done = min(base + PER * LB_THREADS, ntiles);
    for (int i = t; i <= LB_CLASSES; i += LB_THREADS) hist[i] = 0;
  }
}

// COEF: g_out holds, per sample, the render's u (nfs_rotate_render_fwd with u_rot) and `ab` the per-(view, depth
// segment, ray) pair (A, B) of nfs_render_ray_coef: the sample's gradient is A u - B, formed here instead of by a
// render-adjoint pass over the whole rotated volume (K4a: 512 MB of traffic and a launch at eight views)
template <bool COEF>
__global__ void __launch_bounds__(RT_THREADS, 8) rotate_bwd_tiled_kernel(const float* __restrict__ g_out,
                                                                         const float* __restrict__ rot,
                                                                         float* __restrict__ g_d,
                                                                         const unsigned* __restrict__ gmax_bits,
                                                                         float bound_factor, int V, int D, int H,
                                                                         int W, int tiles_y, int tiles_x, int overwrite,
                                                                         int order, const float2* __restrict__ ab,
                                                                         int nseg, int seg_len, int nbounds,
                                                                         const int* __restrict__ lws) {
  __shared__ unsigned long long acc[RT_LZ * RT_LY * RT_LX];
  __shared__ ViewRows vrows[RT_VMAX];
  [[maybe_unused]] __shared__ float gred[RT_THREADS / 64];
  const int t = threadIdx.x;
  // Which tile a block takes.  order 0 (round 1-3): x-border tiles first, then z-border, then the interior (border tiles
  // also collect the clamped out-of-volume samples and run longest; starting them first keeps them off the tail), dealt
  // round-robin to the XCDs by the hardware -- neighbouring tiles, whose catchments overlap by a third, then sit on
  // different L2s and every XCD fetches its own copy of the shared rows (PMC: 608 MB fetched for 320 MB algorithmic).
  // order 1 / 2 (NFS_RT_XCD; measured in round 4, tools/rot_xcd_ab.sh, NOT the default): every XCD owns a contiguous range
  // of (z, y) tile columns (1: z-major, 2: y-major) with all their x tiles, x-border tiles first inside the XCD, so that
  // shared catchment rows are L2 hits: FETCH_SIZE 340 -> 308 / 290 MB (raw counter) but 0.297 -> 0.308 ms -- the kernel is
  // bound by its VALU + LDS-atomic stream, not by the fetch, and the round-robin deal balances the slow border tiles better.
  int bz, by, bx;
  const int* lbox = nullptr;
  if (lws) {
    // live-mask launch: rotate_live_boxes_kernel has left, per tile, the box to accumulate and, in `order`, the tiles by
    // decreasing work -- the longest blocks start first, the tiles nothing reads come last and return at once
    const int ntiles = gridDim.x;
    const int tile = lws[LWS_ORDER(ntiles) + blockIdx.x];
    lbox = lws + LWS_BOXES + tile * 8;
    bx = tile % tiles_x;
    by = (tile / tiles_x) % tiles_y;
    bz = tile / (tiles_x * tiles_y);
  } else if (order == 0) {
    const int tiles_z = gridDim.x / (tiles_x * tiles_y);
    by = blockIdx.x % tiles_y;
    const int oz_ = (blockIdx.x / tiles_y) % tiles_z;
    const int ox_ = blockIdx.x / (tiles_y * tiles_z);
    bz = oz_ == 0 ? 0 : (oz_ == 1 ? tiles_z - 1 : oz_ - 1);
    bx = ox_ == 0 ? 0 : (ox_ == 1 ? tiles_x - 1 : ox_ - 1);
  } else {
    const int tiles_z = (D + RT_TZ - 1) / RT_TZ;
    const int cols = tiles_z * tiles_y, cpx = (cols + 7) / 8;
    const int xcd = blockIdx.x % 8, i = blockIdx.x / 8;
    const int c0 = xcd * cpx, nc = min(cpx, cols - c0);
    if (nc <= 0 || i >= nc * tiles_x) return;
    const int ox_ = i / nc, col = c0 + i % nc;
    bx = ox_ == 0 ? 0 : (ox_ == 1 ? tiles_x - 1 : ox_ - 1);
    if (order == 1) { bz = col / tiles_y; by = col % tiles_y; } else { by = col / tiles_z; bz = col % tiles_z; }
  }
  // the tile (T*) and the box of it this block accumulates (z0 ... x1, inclusive): the whole tile, or -- with a live
  // mask -- the bounding box of the voxels whose gradient anything downstream reads.  What is written outside that box
  // (zeros) meets an exact zero factor downstream; inside it every sample that touches a voxel is still visited and the
  // integer sums do not depend on the order: the velocity gradient is bit-identical to the unmasked launch
  // (tests/test_dead_skip_gpu.py).
  const int Tz0 = bz * RT_TZ, Ty0 = by * RT_TY, Tx0 = bx * RT_TX;
  const int Tz1 = min(Tz0 + RT_TZ, D) - 1, Ty1 = min(Ty0 + RT_TY, H) - 1, Tx1 = min(Tx0 + RT_TX, W) - 1;
  int z0 = Tz0, y0 = Ty0, x0 = Tx0, z1 = Tz1, y1 = Ty1, x1 = Tx1;
  bool dead = false;
  if (lbox) {
    z0 = lbox[0]; z1 = lbox[1]; y0 = lbox[2]; y1 = lbox[3]; x0 = lbox[4]; x1 = lbox[5];   // (scalar loads: uniform address)
    dead = lbox[6] == 0;
  }
  if (!dead)
    for (int i = t; i < RT_LZ * RT_LY * RT_LX; i += RT_THREADS) acc[i] = 0ull;
  // fixed-point scale 2^k: |any voxel sum| <= bound_factor * max|g_out| must stay below 2^62
  float gmax = 0.f;
  if (dead) {                                     // (uniform over the block)
  } else if (COEF) {                              // the maximum of the coefficient kernel's per-block bounds
    const float* bounds = reinterpret_cast<const float*>(gmax_bits);
    float m = 0.f;
    for (int i = t; i < nbounds; i += RT_THREADS) m = fmaxf(m, bounds[i]);
    m = wave_max(m);
    if ((t & 63) == 0) gred[t >> 6] = m;
    __syncthreads();
    gmax = gred[0];
#pragma unroll
    for (int i = 1; i < RT_THREADS / 64; ++i) gmax = fmaxf(gmax, gred[i]);
  } else {
    gmax = __uint_as_float(*gmax_bits);
  }
  if (dead || !(gmax > 0.f)) {                    // nothing downstream reads this tile / all-zero gradient
    if (overwrite)
      for (int i = t; i < RT_TZ * RT_TY * RT_TX; i += RT_THREADS) {
        const int lx_ = i % RT_TX, ly_ = (i / RT_TX) % RT_TY, lz_ = i / (RT_TX * RT_TY);
        const int z = Tz0 + lz_, y = Ty0 + ly_, x = Tx0 + lx_;
        if (z < D && y < H && x < W) g_d[((int64_t)z * H + y) * W + x] = 0.f;
      }
    return;
  }
  if (t < V) rotate_tile_catchment(rot + t * 9, D, H, W, z0, y0, x0, z1, y1, x1, &vrows[t]);
  else if (t >= RT_THREADS / 2 && t < RT_THREADS / 2 + V)
    vrows[t - RT_THREADS / 2].wextra = rotate_view_extra_weight(rot + (t - RT_THREADS / 2) * 9, D, H, W);
  __syncthreads();

  // bound on the summed weight of any voxel: the launcher's 4*nmax per view + 8, and more for a view that is no rotation
  // (for rotations this is the launcher's float, so their scale and sums stay what they were)
  float bf = bound_factor;
  for (int v = 0; v < V; ++v) bf += vrows[v].wextra;
  int ebound;
  frexpf(gmax * bf, &ebound);                     // gmax*bf < 2^ebound
  const int kexp = 62 - ebound;
  // samples are scaled by 2^(k-32): the integer part of a product is the high word, the fraction the low word
  const int ks = kexp - 32;
  const float fscale = ldexpf(1.f, min(max(ks, -120), 120));
  const float fscale2 = ldexpf(1.f, ks - min(max(ks, -120), 120));  // split: 2^ks may exceed the float range

  const int grp = t / RT_GROUP, gl = t % RT_GROUP;
  constexpr int NGRP = RT_THREADS / RT_GROUP;
  const unsigned nz = (unsigned)(z1 - z0 + 1), ny = (unsigned)(y1 - y0 + 1), nx = (unsigned)(x1 - x0 + 1);
  const float3 dm1 = make_float3((float)(D - 1), (float)(H - 1), (float)(W - 1));
  const float oz1 = (float)(1 - z0), oy1 = (float)(1 - y0), ox1 = (float)(1 - x0);
  for (int v = 0; v < V; ++v) {
    const ViewRows& vr = vrows[v];
    const int rows = vr.rows;
    if (rows <= 0) continue;
    const float* gv = g_out + (int64_t)v * D * H * W;
    for (int row = grp; row < rows; row += NGRP) {
      const int zi = vr.ey > 1 ? (int)__umulhi((unsigned)row, vr.my) : row;
      const int oy = vr.y_lo + (row - zi * vr.ey), oz = vr.z_lo + zi;
      // exact x-interval of this row inside the catchment slab of every axis
      float ta = (float)vr.x_lo, tb = (float)vr.x_hi;
      const float fz = (float)oz, fy = (float)oy;
      float pv[3];                 // voxel coordinate of the row's sample ox = 0, per axis
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float p = vr.c[a] + vr.a0[a] * fz + vr.a1[a] * fy;
        pv[a] = p;
        if (vr.inv_s[a] != 0.f) {
          const float u0 = (vr.lo[a] - p) * vr.inv_s[a], u1 = (vr.hi[a] - p) * vr.inv_s[a];
          ta = fmaxf(ta, fminf(u0, u1) - 0.01f);
          tb = fminf(tb, fmaxf(u0, u1) + 0.01f);
        } else if (p < vr.lo[a] || p > vr.hi[a]) {
          tb = ta - 2.f;
        }
      }
      const int xa = (int)ceilf(ta), xb = (int)floorf(tb);
      if (xb < xa) continue;
      float sz = vr.s[0], sy = vr.s[1], sx = vr.s[2];
      // COEF: settle the three LDS reads HERE -- left to the compiler, their first use inside the sample loop puts an
      // s_waitcnt lgkmcnt(0) into every iteration, which also waits for the previous sample's eight LDS atomics.
      // Measured on one box (8 views of 200^3): COEF 324 -> 311 us with it, the plain instance 271 -> 278: that one keeps
      // the compiler's waits.
      if constexpr (COEF) asm volatile("" : "+v"(sz), "+v"(sy), "+v"(sx));
      const float* grow = gv + ((int64_t)oz * H + oy) * W;
      // (COEF: the ray of a sample is its (oy, ox); its depth segment, far end first, is wave-uniform per row)
      [[maybe_unused]] const float2* abrow =
          COEF ? ab + (((int64_t)v * nseg + (D - 1 - oz) / seg_len) * H + oy) * W : nullptr;
      // the next sample's operands are loaded one iteration ahead and stay RAW until they are used (forming A u - B at
      // load time would put a full wait behind every load)
      int ox = xa + gl;
      float g = 0.f;
      [[maybe_unused]] float2 cab = make_float2(0.f, 0.f);
      if (ox <= xb) {
        g = grow[ox];
        if (COEF) cab = abrow[ox];
      }
      while (ox <= xb) {
        const int oxn = ox + RT_GROUP;
        float gn = 0.f;
        [[maybe_unused]] float2 cabn = make_float2(0.f, 0.f);
        if (oxn <= xb) {                       // (one exec-mask block around both loads)
          gn = grow[oxn];
          if (COEF) cabn = abrow[oxn];
        }
        if (COEF) g = fmaf(cab.x, g, -cab.y);
        if (g != 0.f) {
          // lean stencil (same form as the ray march): the sample's voxel coordinate is affine in ox; border
          // replication = clamp the coordinate; base cell floor(c), weights (1-w, w).  A sample clamped onto the far
          // border has base cell n-1 and w = 0: the whole weight on voxel n-1 and an exact zero into the halo cell
          // beyond it (adding zero changes nothing in the fixed-point sum).
          const float fx = (float)ox;
          const float cz = __builtin_amdgcn_fmed3f(fmaf(sz, fx, pv[0]), 0.f, dm1.x);
          const float cy = __builtin_amdgcn_fmed3f(fmaf(sy, fx, pv[1]), 0.f, dm1.y);
          const float cx = __builtin_amdgcn_fmed3f(fmaf(sx, fx, pv[2]), 0.f, dm1.z);
          const float bz = floorf(cz), by_ = floorf(cy), bx_ = floorf(cx);
          const float wz = cz - bz, wy = cy - by_, wx = cx - bx_;
          // halo'd local base cell (small integers: exact in float)
          const int lz = (int)(bz + oz1), ly = (int)(by_ + oy1), lx = (int)(bx_ + ox1);
          if ((unsigned)lz <= nz && (unsigned)ly <= ny && (unsigned)lx <= nx) {
            const float gs = g * fscale * fscale2;
            const float wz1 = gs * wz, wz0 = gs - wz1;
            // packed f32 (v_pk_*_f32, two results per instruction): (w01, w11) = (wz0, wz1) * wy; (w00, w10) = rest
            const f32x2 wzp = {wz0, wz1};
            const f32x2 wy1 = wzp * wy, wy0 = wzp - wy1;
            const f32x2 ax = {1.f - wx, wx};
            f32x2 c00, c01, c10, c11;      // (x, x+1) corner pairs of the rows (z,y), (z,y+1), (z+1,y), (z+1,y+1)
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(c00) : "v"(wy0), "v"(ax));
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]" : "=v"(c01) : "v"(wy1), "v"(ax));
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(c10) : "v"(wy0), "v"(ax));
            asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(c11) : "v"(wy1), "v"(ax));
            // LDS byte address of the base cell: two full-rate 24-bit multiply-adds (the compiler's own choice for
            // this expression is a quarter-rate v_mad_u64_u32)
            unsigned zy, cell_b;
            asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(zy) : "v"(lz), "n"(RT_LY), "v"(ly));
            asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(cell_b) : "v"(zy), "s"(RT_LX * 8), "v"(lx * 8));
            unsigned long long* cell = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(acc) + cell_b);
// float -> 64-bit two's-complement fixed point: high word = floor (v_cvt_flr_i32_f32), low word = fract * 2^32
// (v_fract_f32 is < 1 by construction; the scaling is one packed multiply per corner pair; v_cvt_u32_f32 saturates)
#define NFS_RT_ADD2(off_, c_)                                                                      \
  {                                                                                                \
    unsigned lo0_, hi0_, lo1_, hi1_;                                                               \
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(hi0_) : "v"((c_).x));                                    \
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(hi1_) : "v"((c_).y));                                    \
    f32x2 fr_ = {__builtin_amdgcn_fractf((c_).x), __builtin_amdgcn_fractf((c_).y)};                \
    fr_ = fr_ * 4294967296.f;                                                                      \
    asm("v_cvt_u32_f32 %0, %1" : "=v"(lo0_) : "v"(fr_.x));                                         \
    asm("v_cvt_u32_f32 %0, %1" : "=v"(lo1_) : "v"(fr_.y));                                         \
    atomicAdd(cell + (off_), ((unsigned long long)hi0_ << 32) | lo0_);                             \
    atomicAdd(cell + (off_) + 1, ((unsigned long long)hi1_ << 32) | lo1_);                         \
  }
            NFS_RT_ADD2(0, c00)
            NFS_RT_ADD2(RT_LX, c01)
            NFS_RT_ADD2(RT_LY * RT_LX, c10)
            NFS_RT_ADD2(RT_LY * RT_LX + RT_LX, c11)
#undef NFS_RT_ADD2
          }
        }
        g = gn;
        if (COEF) cab = cabn;
        ox = oxn;
      }
    }
  }
  __syncthreads();
  for (int i = t; i < RT_TZ * RT_TY * RT_TX; i += RT_THREADS) {
    const int lx_ = i % RT_TX, ly_ = (i / RT_TX) % RT_TY, lz_ = i / (RT_TX * RT_TY);
    const int z = Tz0 + lz_, y = Ty0 + ly_, x = Tx0 + lx_;
    if (z < D && y < H && x < W) {
      // (the accumulators are indexed from the box's origin; the tile's voxels outside the box hold no sum)
      const bool in = z >= z0 && z <= z1 && y >= y0 && y <= y1 && x >= x0 && x <= x1;
      const long long q = in ? (long long)acc[((z - z0 + 1) * RT_LY + (y - y0) + 1) * RT_LX + (x - x0) + 1] : 0ll;
      // the tiles partition the volume: with `overwrite` every voxel is written exactly once (no zero fill before)
      if (overwrite) g_d[((int64_t)z * H + y) * W + x] = q != 0 ? (float)ldexp((double)q, -kexp) : 0.f;
      else if (q != 0) g_d[((int64_t)z * H + y) * W + x] += (float)ldexp((double)q, -kexp);
    }
  }
}

// ---- adjoint of MacCormack advection (nfs_advect_maccormack_bwd) ----------------------------------------------------------
// The scheme (warp2d.hip, maccormack_kernel): F = SL(d, x - v), B = SL(F, x + v), A = F + (d - B)/2, out = keep ? F : A with
// keep the limiter's decision, a comparison (no gradient through it).  Given g = dL/d out and the forward's own keep mask:
//   gA = keep ? 0 : g,  gB = -gA/2,  gF = g + SL^T(gB; x + v),  g_d = gA/2 + SL^T(gF; x - v),
//   g_vel = +(n-1)/2 gB grad F(x + v) - (n-1)/2 gF grad d(x - v)
// i.e. the order-1 adjoint twice: pass 1 on (F, -v, gB), pass 2 on (d, v, gF).  gF is a scattered sum that g_vel depends
// on, and g_vel has to come out the same bits in every run (view-sharded ranks apply "the identical step"), so pass 1
// scatters into 64-bit fixed-point accumulators (integer adds are associative), one per element of the field.  Scale
// 2^k from max|g| (absmax_kernel, on the device): every element may trace into one cell, so an accumulator holds at most
// max|g|/2 * D H W C in magnitude; k is the largest power with that bound below 2^62 (a quantum of ~2^-39 max|g| at
// 200^3).  A clamped axis (trace outside the volume: both clipped corners coincide) scatters with weight 1 onto the one
// cell it sampled -- the real-number adjoint of (1 - w) f + w f -- so every weight lies in [0, 1] whatever the velocity.
__device__ __forceinline__ double mc_fixed_scale(const unsigned* gmax_bits, float nelem) {
  const float m = fminf(__uint_as_float(*gmax_bits) * 0.5f * nelem, 3.0e38f);     // > any accumulator's |sum|
  if (!(m > 0.f)) return 1.0;
  int e;
  frexpf(m, &e);                                                                     // m < 2^e
  return ldexp(1.0, 62 - e);
}
__device__ __forceinline__ void mc_fixed_add(long long* acc, int64_t o, double scaled) {
  atomicAdd(reinterpret_cast<unsigned long long*>(acc) + o, (unsigned long long)__double2ll_rn(scaled));
}

// one axis of the stencil tri_setup builds, corners merged where they coincide
struct McAxis { int i[2]; float w[2]; };
__device__ __forceinline__ McAxis mc_axis(float c, int n) {
  const Axis a = axis_setup(c, n);
  const bool two = a.i0 != a.i1;
  return {{a.i0, a.i1}, {two ? 1.f - a.w1 : 1.f, two ? a.w1 : 0.f}};
}
// gradient of the trilinear sample along (z, y, x) in cells: difference of the two faces, interpolated in the other two
// axes (f[a*4 + b*2 + c]: corner (z_a, y_b, x_c))
__device__ __forceinline__ void mc_grad(const float (&f)[8], const McAxis& az, const McAxis& ay, const McAxis& ax, float& dz,
                                        float& dy, float& dx) {
  dz = ay.w[0] * (ax.w[0] * (f[4] - f[0]) + ax.w[1] * (f[5] - f[1])) + ay.w[1] * (ax.w[0] * (f[6] - f[2]) + ax.w[1] * (f[7] - f[3]));
  dy = az.w[0] * (ax.w[0] * (f[2] - f[0]) + ax.w[1] * (f[3] - f[1])) + az.w[1] * (ax.w[0] * (f[6] - f[4]) + ax.w[1] * (f[7] - f[5]));
  dx = az.w[0] * (ay.w[0] * (f[1] - f[0]) + ay.w[1] * (f[3] - f[2])) + az.w[1] * (ay.w[0] * (f[5] - f[4]) + ay.w[1] * (f[7] - f[6]));
}

// pass 1, one thread per voxel (any C, 2-D as D == 1): gB from g and the keep mask; g_vel (nullable) = the B half;
// g_d_acc (nullable) += gA/2 on the element itself; acc += SL^T(gB; x + v) in fixed point.  Stencil: tri_setup at x + v,
// as maccormack_kernel sampled d_fwd.
__global__ void __launch_bounds__(256) maccormack_bwd1_kernel(const float* __restrict__ g_out, const float* __restrict__ vel,
                                                              const float* __restrict__ d_fwd,
                                                              const unsigned long long* __restrict__ keep,
                                                              float* __restrict__ g_vel, float* __restrict__ g_d_acc,
                                                              long long* acc, const unsigned* __restrict__ gmax_bits, int D,
                                                              int H, int W, int C, int nd) {
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  const float* v = vel + vox * nd;
  const float vz = nd == 3 ? v[0] : 0.f, vy = v[nd - 2], vx = v[nd - 1];
  const McAxis az = mc_axis(lin_coord(z, D) + vz, D), ay = mc_axis(lin_coord(y, H) + vy, H),
               ax = mc_axis(lin_coord(x, W) + vx, W);
  const double scale = mc_fixed_scale(gmax_bits, (float)n * (float)C);
  float sz = 0.f, sy = 0.f, sx = 0.f;
  for (int c = 0; c < C; ++c) {
    const int64_t e = vox * C + c;
    const float g = g_out[e];
    const float gA = ((keep[e >> 6] >> (e & 63)) & 1ull) ? 0.f : g, gB = -0.5f * gA;
    if (gA == 0.f) continue;
    if (g_d_acc) g_d_acc[e] += 0.5f * gA;
    int64_t o[8];
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      o[k] = (((int64_t)az.i[k >> 2] * H + ay.i[(k >> 1) & 1]) * W + ax.i[k & 1]) * C + c;
      f[k] = d_fwd[o[k]];
    }
    if (g_vel) {
      float dz, dy, dx;
      mc_grad(f, az, ay, ax, dz, dy, dx);
      sz += gB * dz; sy += gB * dy; sx += gB * dx;
    }
    const double gs = (double)gB * scale;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double w = (double)az.w[k >> 2] * (double)ay.w[(k >> 1) & 1] * (double)ax.w[k & 1];
      if (w != 0.0) mc_fixed_add(acc, o[k], w * gs);
    }
  }
  if (g_vel) {   // coordinate = index + vel (n-1)/2
    float* gv = g_vel + vox * nd;
    if (nd == 3) gv[0] = sz * (0.5f * (float)(D - 1));
    gv[nd - 2] = sy * (0.5f * (float)(H - 1));
    gv[nd - 1] = sx * (0.5f * (float)(W - 1));
  }
}

// pass 1 for the scalar 3-D field: a block owns MT_Z x MT_Y x MT_X voxels and sums what their traces scatter in LDS, in
// the same 64-bit fixed point, over the tile and a halo of MT_R cells (a trace of up to MT_R - 1 cells per axis stays
// inside); the few contributions that land further away go to the global accumulator directly.  The tile is then added
// to the global accumulators row by row (contiguous 8-byte atomics, zeros skipped): about 3.6 global atomics per voxel in
// runs instead of 8 scattered ones (global atomics bound the one-thread-per-voxel form: 0.52 ms at 200^3 for 32 B of
// streamed traffic per cell; this form 0.16 ms, profiles/maccormack_adjoint.txt).  Integer adds in LDS and in memory: the
// sums do not depend on the order.
constexpr int MT_Z = 8, MT_Y = 8, MT_X = 32, MT_R = 3, MT_THREADS = 512;
constexpr int MT_LZ = MT_Z + 2 * MT_R, MT_LY = MT_Y + 2 * MT_R, MT_LX = MT_X + 2 * MT_R, MT_CELLS = MT_LZ * MT_LY * MT_LX;
static_assert(MT_CELLS * 8 <= 64 * 1024, "the tile's accumulators fit the LDS a launch gets without an opt-in");
__global__ void __launch_bounds__(MT_THREADS) maccormack_bwd1_tiled_kernel(const float* __restrict__ g_out,
                                                                           const float* __restrict__ vel,
                                                                           const float* __restrict__ d_fwd,
                                                                           const unsigned long long* __restrict__ keep,
                                                                           float* __restrict__ g_vel, float* __restrict__ g_d_acc,
                                                                           long long* acc, const unsigned* __restrict__ gmax_bits,
                                                                           int D, int H, int W, int ntx, int nty) {
  __shared__ unsigned long long tile[MT_CELLS];
  const int tid = threadIdx.x;
  for (int i = tid; i < MT_CELLS; i += MT_THREADS) tile[i] = 0ull;
  const int bx = blockIdx.x % ntx, by = (blockIdx.x / ntx) % nty, bz = blockIdx.x / (ntx * nty);
  const int z0 = bz * MT_Z, y0 = by * MT_Y, x0 = bx * MT_X;
  const double scale = mc_fixed_scale(gmax_bits, (float)D * (float)H * (float)W);
  __syncthreads();
  for (int l = tid; l < MT_Z * MT_Y * MT_X; l += MT_THREADS) {
    const int x = x0 + l % MT_X, y = y0 + (l / MT_X) % MT_Y, z = z0 + l / (MT_X * MT_Y);
    if (x >= W || y >= H || z >= D) continue;
    const int64_t vox = ((int64_t)z * H + y) * W + x;
    const F3u v = reinterpret_cast<const F3u*>(vel)[vox];
    const float g = g_out[vox];
    const float gA = ((keep[vox >> 6] >> (vox & 63)) & 1ull) ? 0.f : g, gB = -0.5f * gA;
    if (gA == 0.f) {
      if (g_vel) reinterpret_cast<F3u*>(g_vel)[vox] = F3u{0.f, 0.f, 0.f};
      continue;
    }
    if (g_d_acc) g_d_acc[vox] += 0.5f * gA;
    const McAxis az = mc_axis(lin_coord(z, D) + v.x, D), ay = mc_axis(lin_coord(y, H) + v.y, H),
                 ax = mc_axis(lin_coord(x, W) + v.z, W);
    if (g_vel) {
      float f[8];
      tri_gather_pairs(d_fwd, H, W, Axis{az.i[0], az.i[1], 0.f}, Axis{ay.i[0], ay.i[1], 0.f}, Axis{ax.i[0], ax.i[1], 0.f}, f);
      float dz, dy, dx;
      mc_grad(f, az, ay, ax, dz, dy, dx);      // coordinate = index + vel (n-1)/2
      reinterpret_cast<F3u*>(g_vel)[vox] = F3u{gB * dz * (0.5f * (float)(D - 1)), gB * dy * (0.5f * (float)(H - 1)),
                                               gB * dx * (0.5f * (float)(W - 1))};
    }
    const double gs = (double)gB * scale;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double wk = (double)az.w[k >> 2] * (double)ay.w[(k >> 1) & 1] * (double)ax.w[k & 1];
      if (wk == 0.0) continue;
      const int cz = az.i[k >> 2], cy = ay.i[(k >> 1) & 1], cx = ax.i[k & 1];
      const unsigned rz = (unsigned)(cz - z0 + MT_R), ry = (unsigned)(cy - y0 + MT_R), rx = (unsigned)(cx - x0 + MT_R);
      const unsigned long long q = (unsigned long long)__double2ll_rn(wk * gs);
      if (rz < (unsigned)MT_LZ && ry < (unsigned)MT_LY && rx < (unsigned)MT_LX)
        atomicAdd(&tile[(rz * MT_LY + ry) * MT_LX + rx], q);
      else
        atomicAdd(reinterpret_cast<unsigned long long*>(acc) + ((int64_t)cz * H + cy) * W + cx, q);
    }
  }
  __syncthreads();
  for (int i = tid; i < MT_CELLS; i += MT_THREADS) {
    const unsigned long long q = tile[i];
    if (q == 0ull) continue;     // (only cells inside the volume ever receive anything)
    const int cx = x0 - MT_R + i % MT_LX, cy = y0 - MT_R + (i / MT_LX) % MT_LY, cz = z0 - MT_R + i / (MT_LX * MT_LY);
    atomicAdd(reinterpret_cast<unsigned long long*>(acc) + ((int64_t)cz * H + cy) * W + cx, q);
  }
}

// pass 2: gF = g + acc / scale; g_vel (nullable, holds pass 1's half) -= (n-1)/2 gF grad d(x - v); g_d_acc (nullable) +=
// SL^T(gF; x - v) (float atomics, as nfs_advect_bwd).  Stencil: the one d_fwd was sampled with.
// Scalar 3-D fields the four-voxel forward takes (advect1_takes): the lean stencil in advect1_kernel's layout -- a wave
// owns 256 consecutive voxels, lane l takes l, l + 64, ...; g, the accumulators, the velocity and pass 1's half of g_vel
// are streamed in contiguous runs, all requested before the gathers; per-XCD z-slabs.
__global__ void __launch_bounds__(256) maccormack_bwd2x4_kernel(const float* __restrict__ d, const float* __restrict__ vel,
                                                                const float* __restrict__ g_out,
                                                                const long long* __restrict__ acc,
                                                                const unsigned* __restrict__ gmax_bits, float* g_vel,
                                                                float* g_d_acc, int D, int H, int W) {
  const int n = D * H * W;
  const int lane = threadIdx.x & 63, first = lane_first<4, true>(blockDim.x, lane);
  if (first - lane >= n) return;
  const double inv = 1.0 / mc_fixed_scale(gmax_bits, (float)n);
  const F3u* v3 = reinterpret_cast<const F3u*>(vel);
  F3u* gv3 = reinterpret_cast<F3u*>(g_vel);
  F3u vv[4], hh[4];
  float gg[4];
  long long aa[4];
  bool ok[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = first + 64 * j;
    ok[j] = idx < n;
    const int ic = ok[j] ? idx : n - 1;
    vv[j] = v3[ic];
    gg[j] = g_out[ic];
    aa[j] = acc[ic];
    if (g_vel) hh[j] = gv3[ic];
  }
  const LeanDims dm = lean_dims(D, H, W);
  int w, h, z;
  lane_start(first, n, H, W, w, h, z);
  F2u p[4][4];
  float wz[4], wy[4], wx[4], mz[4], my[4], mx[4];
  unsigned ob[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const LeanCell c = lean_cell(vv[j], z, h, w, dm);
    wz[j] = c.wz; wy[j] = c.wy; wx[j] = c.wx; ob[j] = c.o;
    // outside the volume both clipped corners coincide: no dependence on the coordinate
    mz[j] = (c.xz >= 0.f && c.xz < dm.nz1) ? dm.hz : 0.f;
    my[j] = (c.xy >= 0.f && c.xy < dm.ny1) ? dm.hy : 0.f;
    mx[j] = (c.xx >= 0.f && c.xx < dm.nx1) ? dm.hx : 0.f;
    lean_gather(d, c.o, dm, p[j]);
    walk64(w, h, z, W, H, D - 1);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!ok[j]) continue;
    const float gF = (float)((double)gg[j] + (double)aa[j] * inv);
    if (g_vel) {
      float dz, dy, dx;
      lean_grad(p[j], wx[j], wy[j], wz[j], dz, dy, dx);
      gv3[first + 64 * j] = F3u{hh[j].x - gF * dz * mz[j], hh[j].y - gF * dy * my[j], hh[j].z - gF * dx * mx[j]};
    }
    if (g_d_acc && gF != 0.f) {
      const float cz[2] = {1.f - wz[j], wz[j]}, cy[2] = {1.f - wy[j], wy[j]}, cx[2] = {1.f - wx[j], wx[j]};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float contrib = cz[k >> 2] * cy[(k >> 1) & 1] * cx[k & 1] * gF;
        if (contrib != 0.f) atomicAdd(g_d_acc + ob[j] + (k >> 2) * dm.uHW + ((k >> 1) & 1) * dm.uW + (k & 1), contrib);
      }
    }
  }
}

// ... and every other shape (any C, 2-D as D == 1, thin sides), one thread per voxel: tri_setup at x - v
__global__ void __launch_bounds__(256) maccormack_bwd2_kernel(const float* __restrict__ d, const float* __restrict__ vel,
                                                              const float* __restrict__ g_out, const long long* __restrict__ acc,
                                                              const unsigned* __restrict__ gmax_bits, float* __restrict__ g_vel,
                                                              float* __restrict__ g_d_acc, int D, int H, int W, int C, int nd) {
  const int64_t n = (int64_t)D * H * W;
  const int64_t vox = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vox >= n) return;
  const int x = (int)(vox % W), y = (int)((vox / W) % H), z = (int)(vox / ((int64_t)W * H));
  const double inv = 1.0 / mc_fixed_scale(gmax_bits, (float)n * (float)C);
  const float* v = vel + vox * nd;
  const float vz = nd == 3 ? v[0] : 0.f, vy = v[nd - 2], vx = v[nd - 1];
  const McAxis az = mc_axis(lin_coord(z, D) - vz, D), ay = mc_axis(lin_coord(y, H) - vy, H),
               ax = mc_axis(lin_coord(x, W) - vx, W);
  float sz = 0.f, sy = 0.f, sx = 0.f;
  for (int c = 0; c < C; ++c) {
    const int64_t e = vox * C + c;
    const float gF = (float)((double)g_out[e] + (double)acc[e] * inv);
    if (gF == 0.f) continue;
    int64_t o[8];
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      o[k] = (((int64_t)az.i[k >> 2] * H + ay.i[(k >> 1) & 1]) * W + ax.i[k & 1]) * C + c;
      if (g_vel) f[k] = d[o[k]];
    }
    if (g_vel) {
      float dz, dy, dx;
      mc_grad(f, az, ay, ax, dz, dy, dx);
      sz += gF * dz; sy += gF * dy; sx += gF * dx;
    }
    if (g_d_acc) {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float contrib = az.w[k >> 2] * ay.w[(k >> 1) & 1] * ax.w[k & 1] * gF;
        if (contrib != 0.f) atomicAdd(g_d_acc + o[k], contrib);
      }
    }
  }
  if (g_vel) {   // coordinate = index - vel (n-1)/2
    float* gv = g_vel + vox * nd;
    if (nd == 3) gv[0] -= sz * (0.5f * (float)(D - 1));
    gv[nd - 2] -= sy * (0.5f * (float)(H - 1));
    gv[nd - 1] -= sx * (0.5f * (float)(W - 1));
  }
}

static int check_dims(int B, int X, int Y, int Z, int C) {
  NFS_REQUIRE(B > 0 && X > 0 && Y > 0 && Z > 0 && C > 0, "warp: non-positive dimension");
  NFS_REQUIRE((int64_t)B * X * Y * Z * C < (int64_t)1 << 40, "warp: tensor too large");
  return NFS_OK;
}

// ---- the one launch path of rotate_bwd_tiled_kernel -------------------------------------------------------------------
// src: g_out [V,D,H,W], or with COEF (ab set: per-(view, segment, ray) coefficients) the render's u volume; scale_bits:
// max |sample gradient| (COEF: nbounds per-block bounds on it); live + lws (COEF, nullable): the tiles' live boxes are
// formed first and the blocks take the tiles by that order
static void rotate_bwd_tiled_launch(const float* src, const float* rot, float* g_d, const unsigned* scale_bits, int V,
                                    int D, int H, int W, int overwrite, const float2* ab, int nseg, int seg_len,
                                    int nbounds, const unsigned long long* live, int dilate, int* lws, hipStream_t s) {
  const int tz = (D + RT_TZ - 1) / RT_TZ, ty = (H + RT_TY - 1) / RT_TY, tx = (W + RT_TX - 1) / RT_TX;
  // a voxel collects, per rotation view, unit total weight from interior samples and at most ~max(D,H,W)
  // clamped samples per face direction; 4*nmax per view is a safe bound on the summed weights (the kernel
  // raises it for any view whose matrix is no rotation: rotate_view_extra_weight)
  const int nmax = D > H ? (D > W ? D : W) : (H > W ? H : W);
  const float bound_factor = 4.f * (float)nmax * (float)V + 8.f;
  // (0, 1 or 2; anything else is the default order, not a third decomposition the kernel does not have)
  static const int order = [] { const char* e = getenv("NFS_RT_XCD"); const int v = e ? atoi(e) : 0; return v == 1 || v == 2 ? v : 0; }();
  const int grid = (live || order == 0) ? tz * ty * tx : 8 * ((tz * ty + 7) / 8) * tx;
  if (live) {
    hipLaunchKernelGGL(rotate_live_boxes_kernel, dim3((tz * ty * tx + LB_WAVES - 1) / LB_WAVES), dim3(LB_THREADS), 0, s,
                       live, D, H, W, ty, tx, dilate, tz * ty * tx, lws);
    hipLaunchKernelGGL(rotate_live_order_kernel, dim3(1), dim3(LB_THREADS), 0, s, tz * ty * tx, lws);
  }
  const auto kernel = ab ? rotate_bwd_tiled_kernel<true> : rotate_bwd_tiled_kernel<false>;
  for (int v0 = 0; v0 < V; v0 += RT_VMAX) {
    const int vn = V - v0 < RT_VMAX ? V - v0 : RT_VMAX;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(RT_THREADS), 0, s, src + (int64_t)v0 * D * H * W, rot + v0 * 9, g_d,
                       scale_bits, bound_factor, vn, D, H, W, ty, tx, (overwrite && v0 == 0) ? 1 : 0, order,
                       ab ? ab + (int64_t)v0 * nseg * H * W : ab, nseg, seg_len, nbounds, live ? (const int*)lws : nullptr);
  }
}

// ---- the one launch path of advect1_kernel -----------------------------------------------------------------------------
// the shapes it takes: nz planes of a [D,H,W] volume (nz = D: all of it)
static bool advect1_takes(int D, int H, int W, int nz) {
  return W >= 2 && H >= 2 && D >= 2 && (int64_t)nz * H * W % 4 == 0 && (int64_t)D * H * W < ((int64_t)1 << 30);
}

// mode: advect1_kernel's MODE; LIVE follows ad.live, EVER ad.ever (and NFS_EVER_LANES); the planes [z0, z0 + nz) of the
// volume (vel / g_out / out / the moments hold those only; z0 = 0, nz = D: the whole-volume forms).  The callers have
// checked their pointers for null.
// src: what vel is (advect1_kernel's SRC; other than SRC_VEL: mode 0 / 1 on whole volumes).
template <int SRC>
static auto advect1_from(int mode, bool live) {
  return mode == 1 ? advect1_kernel<1, false, false, SRC>
                   : live ? advect1_kernel<0, true, false, SRC> : advect1_kernel<0, false, false, SRC>;
}

static int advect1_launch(const char* who, int mode, const float* d, const float* vel, const float* g_out, float* out,
                          int D, int H, int W, int z0, int nz, const AdamFused& ad, nfs_stream_t stream, int src = SRC_VEL) {
  NFS_REQUIRE(!ad.adv_next || (ad.adv_next != d && ad.adv_next != g_out), "%s: adv_next must not alias d or g_out", who);
  if (int e = check_dims(1, D, H, W, 1)) return e;
  NFS_REQUIRE(z0 >= 0 && nz >= 1 && z0 + nz <= D, "%s: slab outside the volume", who);
  NFS_REQUIRE(advect1_takes(D, H, W, nz),
              "%s: needs D, H, W >= 2, D*H*W < 2^30 and a multiple of 4 voxels (nz*H*W for a slab)", who);
  const int64_t n = (int64_t)nz * H * W;
  auto kernel = ad.live ? advect1_kernel<0, true> : advect1_kernel<0>;
  if (src != SRC_VEL) {
    NFS_REQUIRE(mode != 2 && z0 == 0 && nz == D,
                "%s: a stream function or potential takes the forward and the gradient of a whole volume", who);
    kernel = src == SRC_STREAM ? advect1_from<SRC_STREAM>(mode, ad.live)
             : src == SRC_POTENTIAL ? advect1_from<SRC_POTENTIAL>(mode, ad.live) : advect1_from<SRC_HELMHOLTZ>(mode, ad.live);
  } else if (mode == 1) {
    kernel = advect1_kernel<1>;
  } else if (mode == 2 && !ad.live) {
    kernel = advect1_kernel<2>;
  } else if (mode == 2) {
    // (per-lane predication goes through buffer descriptors: 32-bit byte offsets, 12 n < 2^31; larger volumes skip by waves only)
    static const bool lanes = [] { const char* e = getenv("NFS_EVER_LANES"); return !(e && atoi(e) == 0); }();
    kernel = (ad.ever && lanes && n * 12 < ((int64_t)1 << 31)) ? advect1_kernel<2, true, true> : advect1_kernel<2, true>;
  }
  // 256 threads x 4 voxels; whole rounds of the 8 XCDs
  hipLaunchKernelGGL(kernel, dim3((blocks_for(n, 1024) + 7) / 8 * 8), dim3(256), 0, as_stream(stream), d, vel, g_out, out,
                     nz, H, W, ad, z0, D);
  return check_launch(who);
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_warp3d_fwd(const float* imgs, const float* coords, float* out, int B, int X, int Y, int Z, int C,
                   nfs_stream_t stream) {
  NFS_REQUIRE(imgs && coords && out, "nfs_warp3d_fwd: null pointer");
  if (int e = check_dims(B, X, Y, Z, C)) return e;
  WarpArgs a{imgs, coords, B, X, Y, Z, C, 1};
  const int64_t n = (int64_t)B * X * Y * Z;
  hipLaunchKernelGGL(warp_fwd_kernel<COORD_EXPLICIT>, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), a, out);
  return check_launch("nfs_warp3d_fwd");
}

int nfs_warp3d_bwd(const float* imgs, const float* coords, const float* g_out, float* g_imgs_acc, float* g_coords,
                   int B, int X, int Y, int Z, int C, nfs_stream_t stream) {
  NFS_REQUIRE(coords && g_out, "nfs_warp3d_bwd: null pointer");
  NFS_REQUIRE(!g_coords || imgs, "nfs_warp3d_bwd: g_coords needs imgs");
  if (int e = check_dims(B, X, Y, Z, C)) return e;
  WarpArgs a{imgs, coords, B, X, Y, Z, C, 1};
  const int64_t n = (int64_t)B * X * Y * Z;
  hipLaunchKernelGGL(warp_bwd_kernel<COORD_EXPLICIT>, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), a,
                     g_out, g_imgs_acc, g_coords);
  return check_launch("nfs_warp3d_bwd");
}

int nfs_rotate_fwd(const float* d, const float* rot, float* out, int V, int D, int H, int W, int C,
                   nfs_stream_t stream) {
  NFS_REQUIRE(d && rot && out, "nfs_rotate_fwd: null pointer");
  if (int e = check_dims(V, D, H, W, C)) return e;
  WarpArgs a{d, rot, V, D, H, W, C, 0};
  const int64_t n = (int64_t)V * D * H * W;
  hipLaunchKernelGGL(warp_fwd_kernel<COORD_ROTATE>, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), a, out);
  return check_launch("nfs_rotate_fwd");
}

int nfs_rotate_bwd(const float* g_out, const float* rot, float* g_d_acc, int V, int D, int H, int W, int C,
                   float* workspace, const float* g_max, int overwrite, nfs_stream_t stream) {
  NFS_REQUIRE(g_out && rot && g_d_acc, "nfs_rotate_bwd: null pointer");
  if (int e = check_dims(V, D, H, W, C)) return e;
  if (C == 1 && workspace) {
    const unsigned* gmax_bits = reinterpret_cast<const unsigned*>(g_max);
    if (!gmax_bits) {                       // no max |g_out| supplied: streaming pre-pass
      unsigned* wb = reinterpret_cast<unsigned*>(workspace);
      zero_words(wb, 1, as_stream(stream));                              // (a kernel, not a memset node: common.h)
      const int64_t n = (int64_t)V * D * H * W;
      hipLaunchKernelGGL(absmax_kernel, dim3(2048), dim3(256), 0, as_stream(stream), g_out, n, wb);
      gmax_bits = wb;
    }
    rotate_bwd_tiled_launch(g_out, rot, g_d_acc, gmax_bits, V, D, H, W, overwrite, nullptr, 1, D, 0, nullptr, 0, nullptr,
                            as_stream(stream));
    return check_launch("nfs_rotate_bwd(tiled)");
  }
  NFS_REQUIRE(!overwrite, "nfs_rotate_bwd: overwrite needs the tiled adjoint (C == 1 and a workspace)");
  WarpArgs a{nullptr, rot, V, D, H, W, C, 0};
  const int64_t n = (int64_t)V * D * H * W;
  hipLaunchKernelGGL(warp_bwd_kernel<COORD_ROTATE>, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), a,
                     g_out, g_d_acc, (float*)nullptr);
  return check_launch("nfs_rotate_bwd");
}

// the tiled adjoint on the render's u volume and per-(view, segment, ray) coefficients: sample gradient = A u - B
// (nfs_rotate_render_fwd_coef / nfs_render_ray_coef); bounds [nbounds]: per-block bounds on max |sample gradient|, whose
// maximum sets the fixed-point scale
static int rotate_bwd_coef_impl(const char* who, const float* u_rot, const float* ab, const float* rot, float* g_d_acc, int V,
                                int D, int H, int W, int nseg, int seg_len, const float* bounds, int nbounds, int overwrite,
                                const unsigned long long* live, int dilate, int* lws, nfs_stream_t stream) {
  NFS_REQUIRE(u_rot && ab && rot && g_d_acc && bounds, "nfs_rotate_bwd_coef: null pointer");
  NFS_REQUIRE(nbounds > 0, "nfs_rotate_bwd_coef: no bounds");
  if (int e = check_dims(V, D, H, W, 1)) return e;
  NFS_REQUIRE(nseg > 0 && seg_len > 0 && (int64_t)nseg * seg_len >= D, "nfs_rotate_bwd_coef: the segments do not cover D");
  NFS_REQUIRE(!live || (dilate >= 0 && RT_TX + 2 * dilate <= 63), "nfs_rotate_bwd_coef_live: dilate out of range");
  rotate_bwd_tiled_launch(u_rot, rot, g_d_acc, reinterpret_cast<const unsigned*>(bounds), V, D, H, W, overwrite,
                          reinterpret_cast<const float2*>(ab), nseg, seg_len, nbounds, live, dilate, lws, as_stream(stream));
  return check_launch(who);
}

int nfs_rotate_bwd_coef(const float* u_rot, const float* ab, const float* rot, float* g_d_acc, int V, int D, int H, int W,
                        int nseg, int seg_len, const float* bounds, int nbounds, int overwrite, nfs_stream_t stream) {
  return rotate_bwd_coef_impl("nfs_rotate_bwd_coef", u_rot, ab, rot, g_d_acc, V, D, H, W, nseg, seg_len, bounds, nbounds,
                              overwrite, nullptr, 0, nullptr, stream);
}

// ... restricted to what a velocity variable can use: `live` is the mask nfs_advect_fwd_live / nfs_advect_bwd_adam_fwd_live
// wrote for the CURRENT velocity ([nfs_live_mask_words] 64-bit words, bit = linear voxel index), `dilate` the reach of
// the linear stencil between g_d and the advect adjoint (1 for the 3x3x3 smoothing, 0 without it).  Inside a tile's box
// (the bounding box of its voxels within `dilate` of a live voxel) g_d is bit-identical to nfs_rotate_bwd_coef; outside
// the boxes it is written as zeros (overwrite) or left alone (accumulate) -- values that only ever meet a zero factor.
// A tile without a box returns before its sample loop; the others run longest first.
int nfs_rotate_bwd_coef_live(const float* u_rot, const float* ab, const float* rot, float* g_d_acc, int V, int D, int H,
                             int W, int nseg, int seg_len, const float* bounds, int nbounds, int overwrite,
                             const unsigned long long* live, int dilate, int* workspace, nfs_stream_t stream) {
  NFS_REQUIRE(live && workspace, "nfs_rotate_bwd_coef_live: null mask / workspace");
  return rotate_bwd_coef_impl("nfs_rotate_bwd_coef_live", u_rot, ab, rot, g_d_acc, V, D, H, W, nseg, seg_len, bounds,
                              nbounds, overwrite, live, dilate, workspace, stream);
}

// ints of that workspace: a box per tile, the tiles in the order the adjoint's blocks take them (written by every launch
// before it is read: no initialisation needed)
int nfs_rotate_live_workspace_ints(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  const int nt = ((D + RT_TZ - 1) / RT_TZ) * ((H + RT_TY - 1) / RT_TY) * ((W + RT_TX - 1) / RT_TX);
  return LWS_ORDER(nt) + nt;
}

// 64-bit words of the live mask of a [D,H,W] volume (one bit per voxel, rounded up to whole waves of 256 voxels)
int nfs_live_mask_words(int D, int H, int W) {
  const int64_t n = (int64_t)D * H * W;
  return (D > 0 && H > 0 && W > 0 && n < ((int64_t)1 << 30)) ? (int)((n + 255) / 256 * 4) : 0;
}

int nfs_advect_fwd(const float* d, const float* vel, float* out, int D, int H, int W, int C, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && out, "nfs_advect_fwd: null pointer");
  if (int e = check_dims(1, D, H, W, C)) return e;
  if (C == 1 && advect1_takes(D, H, W, D))
    return advect1_launch("nfs_advect_fwd(x4)", 0, d, vel, nullptr, out, D, H, W, 0, D, AdamFused{}, stream);
  WarpArgs a{d, vel, 1, D, H, W, C, 0};
  const int64_t n = (int64_t)D * H * W;
  hipLaunchKernelGGL(warp_fwd_kernel<COORD_ADVECT>, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), a, out);
  return check_launch("nfs_advect_fwd");
}

// nfs_advect_fwd for a scalar field + the live mask of the back-traced stencils (see AdamFused::live): refuses the shapes
// the four-voxel kernel does not take (NFS_EINVAL; callers then run without a mask)
int nfs_advect_fwd_live(const float* d, const float* vel, float* out, unsigned long long* live, int D, int H, int W,
                        nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && out && live, "nfs_advect_fwd_live: null pointer");
  AdamFused ad{};
  ad.live = live;
  return advect1_launch("nfs_advect_fwd_live", 0, d, vel, nullptr, out, D, H, W, 0, D, ad, stream);
}

int nfs_advect_bwd(const float* d, const float* vel, const float* g_out, float* g_d_acc, float* g_vel, int D, int H,
                   int W, int C, nfs_stream_t stream) {
  NFS_REQUIRE(vel && g_out, "nfs_advect_bwd: null pointer");
  NFS_REQUIRE(!g_vel || d, "nfs_advect_bwd: g_vel needs d");
  NFS_REQUIRE(g_d_acc || g_vel, "nfs_advect_bwd: nothing to compute");
  if (int e = check_dims(1, D, H, W, C)) return e;
  if (C == 1 && !g_d_acc && advect1_takes(D, H, W, D))   // velocity gradient only: no atomics
    return advect1_launch("nfs_advect_bwd(x4)", 1, d, vel, g_out, g_vel, D, H, W, 0, D, AdamFused{}, stream);
  WarpArgs a{d, vel, 1, D, H, W, C, 0};
  const int64_t n = (int64_t)D * H * W;
  hipLaunchKernelGGL(warp_bwd_kernel<COORD_ADVECT>, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), a,
                     g_out, g_d_acc, g_vel);
  return check_launch("nfs_advect_bwd");
}

// advect along the velocity a variable stands for (source_velocity<SRC>(), source_ops.h: s [D,H,W,3], phi [D,H,W] or
// a [D,H,W,4]), the velocity never stored; live (nullable): the mask nfs_advect_fwd_live writes.  Bit-identical to
// nfs_curl_fwd / nfs_grad_fwd (reversed; for a: both, added once) followed by nfs_advect_fwd / _live on the stored velocity
static int advect_from_fwd(const char* who, int src, const float* d, const float* var, float* out, unsigned long long* live,
                           int D, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(d && var && out, "%s: null pointer", who);
  NFS_REQUIRE(out != d && out != var, "%s: out must not alias d or %s", who, source_name(src));
  NFS_REQUIRE(src != SRC_HELMHOLTZ || aligned16(var), "%s: the Helmholtz variable must be 16-byte aligned", who);
  AdamFused ad{};
  ad.live = live;
  return advect1_launch(who, 0, d, var, nullptr, out, D, H, W, 0, D, ad, stream, src);
}

// ... and its velocity gradient g_vel [D,H,W,3] (advect's channel order), the velocity recomputed from the variable:
// bit-identical to nfs_advect_bwd (g_vel only) on the stored velocity
static int advect_from_bwd(const char* who, int src, const float* d, const float* var, const float* g_out, float* g_vel,
                           int D, int H, int W, nfs_stream_t stream) {
  NFS_REQUIRE(d && var && g_out && g_vel, "%s: null pointer", who);
  NFS_REQUIRE(g_vel != d && g_vel != var && g_vel != g_out, "%s: g_vel must not alias d, %s or g_out", who, source_name(src));
  NFS_REQUIRE(src != SRC_HELMHOLTZ || aligned16(var), "%s: the Helmholtz variable must be 16-byte aligned", who);
  return advect1_launch(who, 1, d, var, g_out, g_vel, D, H, W, 0, D, AdamFused{}, stream, src);
}

int nfs_advect_stream_fwd(const float* d, const float* s, float* out, unsigned long long* live, int D, int H, int W,
                          nfs_stream_t stream) {
  return advect_from_fwd("nfs_advect_stream_fwd", SRC_STREAM, d, s, out, live, D, H, W, stream);
}

int nfs_advect_stream_bwd(const float* d, const float* s, const float* g_out, float* g_vel, int D, int H, int W,
                          nfs_stream_t stream) {
  return advect_from_bwd("nfs_advect_stream_bwd", SRC_STREAM, d, s, g_out, g_vel, D, H, W, stream);
}

int nfs_advect_potential_fwd(const float* d, const float* phi, float* out, unsigned long long* live, int D, int H, int W,
                             nfs_stream_t stream) {
  return advect_from_fwd("nfs_advect_potential_fwd", SRC_POTENTIAL, d, phi, out, live, D, H, W, stream);
}

int nfs_advect_potential_bwd(const float* d, const float* phi, const float* g_out, float* g_vel, int D, int H, int W,
                             nfs_stream_t stream) {
  return advect_from_bwd("nfs_advect_potential_bwd", SRC_POTENTIAL, d, phi, g_out, g_vel, D, H, W, stream);
}

int nfs_advect_helmholtz_fwd(const float* d, const float* a, float* out, unsigned long long* live, int D, int H, int W,
                             nfs_stream_t stream) {
  return advect_from_fwd("nfs_advect_helmholtz_fwd", SRC_HELMHOLTZ, d, a, out, live, D, H, W, stream);
}

int nfs_advect_helmholtz_bwd(const float* d, const float* a, const float* g_out, float* g_vel, int D, int H, int W,
                             nfs_stream_t stream) {
  return advect_from_bwd("nfs_advect_helmholtz_bwd", SRC_HELMHOLTZ, d, a, g_out, g_vel, D, H, W, stream);
}

// ---- adjoint of nfs_advect_maccormack_keep (transform.py:570-582, 590-607; the kernels above) ----------------------------
static bool mc_dims_ok(int D, int H, int W, int C, int nd) {
  return D > 0 && H > 0 && W > 0 && C > 0 && (nd == 2 || nd == 3) && (nd == 3 || D == 1) &&
         (int64_t)D * H * W * C < ((int64_t)1 << 40);
}
// workspace: the 64-bit accumulators (one per element), then 64 floats whose first word holds max|g_out|
int64_t nfs_advect_maccormack_bwd_workspace_floats(int D, int H, int W, int C, int nd) {
  return mc_dims_ok(D, H, W, C, nd) ? 2 * (int64_t)D * H * W * C + 64 : -1;
}

int nfs_advect_maccormack_bwd(const float* d, const float* vel, const float* d_fwd, const unsigned long long* keep,
                              const float* g_out, float* g_d_acc, float* g_vel, float* workspace, int64_t workspace_floats,
                              int D, int H, int W, int C, int nd, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && d_fwd && keep && g_out && workspace, "nfs_advect_maccormack_bwd: null pointer");
  NFS_REQUIRE(g_d_acc || g_vel, "nfs_advect_maccormack_bwd: nothing to compute");
  NFS_REQUIRE(mc_dims_ok(D, H, W, C, nd),
              "nfs_advect_maccormack_bwd: needs positive dimensions, nd 2 (with D == 1) or 3, fewer than 2^40 elements");
  const int64_t ne = (int64_t)D * H * W * C, nv = (int64_t)D * H * W;
  NFS_REQUIRE(workspace_floats >= 2 * ne + 64 && ((uintptr_t)workspace & 7) == 0,
              "nfs_advect_maccormack_bwd: workspace smaller than nfs_advect_maccormack_bwd_workspace_floats() or not 8-byte "
              "aligned");
  NFS_REQUIRE(g_vel != g_out && g_d_acc != g_out, "nfs_advect_maccormack_bwd: the gradients must not alias g_out");
  hipStream_t s = as_stream(stream);
  long long* acc = reinterpret_cast<long long*>(workspace);
  unsigned* gmax = reinterpret_cast<unsigned*>(workspace + 2 * ne);
  zero_words(workspace, 2 * ne + 64, s);
  const unsigned mb = blocks_for(ne, 1024);
  hipLaunchKernelGGL(absmax_kernel, dim3(mb < 2048 ? mb : 2048), dim3(256), 0, s, g_out, ne, gmax);
  // the scalar 3-D fields the four-voxel forward takes (nfs_advect_fwd's choice of stencil for d_fwd) have kernels of
  // their own in both passes
  const bool hot = C == 1 && nd == 3 && advect1_takes(D, H, W, D);
  if (hot) {
    const int ntx = (W + MT_X - 1) / MT_X, nty = (H + MT_Y - 1) / MT_Y, ntz = (D + MT_Z - 1) / MT_Z;
    hipLaunchKernelGGL(maccormack_bwd1_tiled_kernel, dim3(ntx * nty * ntz), dim3(MT_THREADS), 0, s, g_out, vel, d_fwd, keep,
                       g_vel, g_d_acc, acc, gmax, D, H, W, ntx, nty);
  } else {
    hipLaunchKernelGGL(maccormack_bwd1_kernel, dim3(blocks_for(nv, 256)), dim3(256), 0, s, g_out, vel, d_fwd, keep, g_vel,
                       g_d_acc, acc, gmax, D, H, W, C, nd);
  }
  if (hot)                                                    // 256 threads x 4 voxels; whole rounds of the 8 XCDs
    hipLaunchKernelGGL(maccormack_bwd2x4_kernel, dim3((blocks_for(nv, 1024) + 7) / 8 * 8), dim3(256), 0, s, d, vel, g_out,
                       acc, gmax, g_vel, g_d_acc, D, H, W);
  else
    hipLaunchKernelGGL(maccormack_bwd2_kernel, dim3(blocks_for(nv, 256)), dim3(256), 0, s, d, vel, g_out, acc, gmax, g_vel,
                       g_d_acc, D, H, W, C, nd);
  return check_launch("nfs_advect_maccormack_bwd");
}

// velocity gradient of advect + TF ApplyAdam on the velocity in one pass (scalar field, C = 1; the shapes the four-voxel
// kernel does not take: nfs_advect_bwd + nfs_adam_tf_step)
int nfs_advect_bwd_adam(const float* d, float* vel, const float* g_out, float* m, float* v, int D, int H, int W,
                        float lr_t, float beta1, float beta2, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && g_out && m && v, "nfs_advect_bwd_adam: null pointer");
  return advect1_launch("nfs_advect_bwd_adam", 2, d, vel, g_out, vel, D, H, W, 0, D,
                        AdamFused{m, v, lr_t, beta1, beta2, eps}, stream);
}

// ... and the NEXT iteration's forward advect of the updated velocity in the same pass (adv_next [D,H,W], see AdamFused)
int nfs_advect_bwd_adam_fwd(const float* d, float* vel, const float* g_out, float* m, float* v, float* adv_next, int D, int H,
                            int W, float lr_t, float beta1, float beta2, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && g_out && m && v && adv_next, "nfs_advect_bwd_adam_fwd: null pointer");
  return advect1_launch("nfs_advect_bwd_adam_fwd", 2, d, vel, g_out, vel, D, H, W, 0, D,
                        AdamFused{m, v, lr_t, beta1, beta2, eps, adv_next}, stream);
}

// ... and the live mask of that next forward sample (for the next iteration's nfs_rotate_bwd_coef_live)
int nfs_advect_bwd_adam_fwd_live(const float* d, float* vel, const float* g_out, float* m, float* v, float* adv_next,
                                 unsigned long long* live_next, int D, int H, int W, float lr_t, float beta1, float beta2,
                                 float eps, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && g_out && m && v && adv_next && live_next, "nfs_advect_bwd_adam_fwd_live: null pointer");
  return advect1_launch("nfs_advect_bwd_adam_fwd_live", 2, d, vel, g_out, vel, D, H, W, 0, D,
                        AdamFused{m, v, lr_t, beta1, beta2, eps, adv_next, live_next}, stream);
}

// ... skipping the waves whose voxels have never been live (see `ever` in advect1_kernel): `live` holds the mask of the
// CURRENT forward sample on entry and that of the next one on return, `ever` [nfs_live_mask_words] is the OR of every mask
// since m and v were zeroed (zero it with them; the caller must not use it once anything else has written m or v).
// Bit-identical to nfs_advect_bwd_adam_fwd_live.
int nfs_advect_bwd_adam_fwd_live_ever(const float* d, float* vel, const float* g_out, float* m, float* v, float* adv_next,
                                      unsigned long long* live, unsigned long long* ever, int D, int H, int W, float lr_t,
                                      float beta1, float beta2, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && g_out && m && v && adv_next && live && ever, "nfs_advect_bwd_adam_fwd_live_ever: null pointer");
  return advect1_launch("nfs_advect_bwd_adam_fwd_live_ever", 2, d, vel, g_out, vel, D, H, W, 0, D,
                        AdamFused{m, v, lr_t, beta1, beta2, eps, adv_next, live, ever}, stream);
}

// Slab forms (view-sharded runs shard the replicated field work over D-slabs, engine.GridStylizer): d is the whole
// [D,H,W] density, vel / out / g_out / m / v hold the nz planes [z0, z0 + nz) only.  Same arithmetic per voxel as the
// whole-volume entry points (the same kernel with a plane offset).
int nfs_advect_fwd_slab(const float* d, const float* vel, float* out, int D, int H, int W, int z0, int nz,
                        nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && out, "nfs_advect_fwd_slab: null pointer");
  return advect1_launch("nfs_advect_fwd_slab", 0, d, vel, nullptr, out, D, H, W, z0, nz, AdamFused{}, stream);
}

int nfs_advect_bwd_adam_slab(const float* d, float* vel, const float* g_out, float* m, float* v, int D, int H, int W,
                             int z0, int nz, float lr_t, float beta1, float beta2, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && g_out && m && v, "nfs_advect_bwd_adam_slab: null pointer");
  return advect1_launch("nfs_advect_bwd_adam_slab", 2, d, vel, g_out, vel, D, H, W, z0, nz,
                        AdamFused{m, v, lr_t, beta1, beta2, eps}, stream);
}

int nfs_advect_bwd_adam_fwd_slab(const float* d, float* vel, const float* g_out, float* m, float* v, float* adv_next, int D,
                                 int H, int W, int z0, int nz, float lr_t, float beta1, float beta2, float eps,
                                 nfs_stream_t stream) {
  NFS_REQUIRE(d && vel && g_out && m && v && adv_next, "nfs_advect_bwd_adam_fwd_slab: null pointer");
  return advect1_launch("nfs_advect_bwd_adam_fwd_slab", 2, d, vel, g_out, vel, D, H, W, z0, nz,
                        AdamFused{m, v, lr_t, beta1, beta2, eps, adv_next}, stream);
}

// one step of StylerBase._transport (styler_base.py:59-89) with the temporal filter's weighted accumulation fused in
int nfs_transport_step(const float* g, const float* u, float scale, float w_g, const float* addend, float w_addend,
                       float* out, int D, int H, int W, int C, nfs_stream_t stream) {
  NFS_REQUIRE(g && u && out, "nfs_transport_step: null pointer");
  NFS_REQUIRE(g != out, "nfs_transport_step: out must not alias g (it is a gather)");
  if (int e = check_dims(1, D, H, W, C)) return e;
  const int64_t n = (int64_t)D * H * W;
  if ((C == 1 || C == 3) && W >= 2 && H >= 2 && D >= 2 && n < ((int64_t)1 << 29)) {
    const unsigned blocks = (blocks_for(n, 512) + 7) / 8 * 8;
    if (C == 3)
      hipLaunchKernelGGL(transport_step_kernel<3>, dim3(blocks), dim3(256), 0, as_stream(stream), g, u, addend, out, D, H,
                         W, scale, w_g, w_addend);
    else
      hipLaunchKernelGGL(transport_step_kernel<1>, dim3(blocks), dim3(256), 0, as_stream(stream), g, u, addend, out, D, H,
                         W, scale, w_g, w_addend);
    return check_launch("nfs_transport_step");
  }
  hipLaunchKernelGGL(transport_step_generic_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), g, u,
                     addend, out, D, H, W, C, scale, w_g, w_addend);
  return check_launch("nfs_transport_step(generic)");
}

}  // extern "C"
