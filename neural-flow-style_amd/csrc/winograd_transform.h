// What the transform kernels of the three-kernel Winograd convolutions, F(4x4) (winograd.hip) and F(5x5) (winograd5.hip),
// must agree on to the last bit, written once.  Each family has two schedules of the same arithmetic -- one thread per
// (tile, channel[-pair]) and one wave per patch column ("six / seven waves") -- and a data gradient reads the ReLU bit
// cache that a forward pass wrote, possibly in the other schedule:
//
//   the Cook-Toom passes        wg4_bt / wg4_at (winograd_math.h), w5_bt / w5_at
//   the layer epilogue          NFS_WG_EPILOGUE over wg_add / wg_relu / wg_keep / wg_keep_positive (float or float2)
//   the bit-cache layouts       NFS_WG4_BIT_SHIFT, wg4_bit_pair, NFS_WG4_NB_TILE / NFS_WG4_NB_POS (the pooled gradient's
//                               neighbour lookup); w5_bit_shift, w5_bits_store (pair merge + store), w5_bits_at / w5_bits_mask
//   indexing                    NFS_WG_TILE (tile -> b, ty, tx), wg_xcd_block (XCD-contiguous block order)
//
// Functions where the kernels' instruction streams stayed those of the expressions written in place, statement or
// expression macros where they did not (each says so; profiles/winograd_transform_refactor.txt has the comparison).  The
// column and row passes around these pieces stay written out per kernel: as shared functions they changed every stream.
#pragma once
#include "common.h"
#include "winograd_math.h"

namespace nfs {

// ---- indexing ----------------------------------------------------------------------------------------------------------
// tile -> image b, tile row ty, tile column tx, declared in place (a statement macro: through a function that returns the
// three, two of the six-wave F(4x4) kernels scheduled one compare differently from the parent's written-out line)
#define NFS_WG_TILE(tile, TH, TW) \
  const int tx = (int)((tile) % (TW)), ty = (int)(((tile) / (TW)) % (TH)), b = (int)((tile) / ((int64_t)(TW) * (TH)))
// Patches of neighbouring tiles overlap by two pixels: give each XCD a contiguous range of blocks (workgroups are dealt
// round-robin to the 8 XCDs; the grid is a multiple of 8), or every shared pixel is fetched from HBM into two L2s
// (PMC: 2.0x / 2.5x the compulsory read bytes with the plain order)
__device__ __forceinline__ unsigned wg_xcd_block(unsigned block, unsigned blocks) {
  const unsigned per_xcd = blocks / 8;
  return (block % 8) * per_xcd + block / 8;
}

// ---- the layer epilogue ---------------------------------------------------------------------------------------------------
// Written once for a value V of one channel (float, F(5x5)) or of a channel pair (float2, F(4x4)); the overloads below are
// what it does per component.  keep: one channel's mask bit (bool) or a pair's two (bits 0 and 1 of a word).
__device__ __forceinline__ void wg_add(float& v, float b) { v += b; }
__device__ __forceinline__ void wg_add(float2& v, float2 b) { v.x += b.x; v.y += b.y; }
__device__ __forceinline__ void wg_relu(float& v) { v = fmaxf(v, 0.f); }
__device__ __forceinline__ void wg_relu(float2& v) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); }
__device__ __forceinline__ void wg_keep(float& v, bool keep) { v = keep ? v : 0.f; }
__device__ __forceinline__ void wg_keep(float2& v, uint32_t keep) { v.x = (keep & 1u) ? v.x : 0.f; v.y = (keep & 2u) ? v.y : 0.f; }
__device__ __forceinline__ void wg_keep_positive(float& v, float x) { v = x > 0.f ? v : 0.f; }
__device__ __forceinline__ void wg_keep_positive(float2& v, float2 x) { v.x = x.x > 0.f ? v.x : 0.f; v.y = x.y > 0.f ? v.y : 0.f; }
// MODE 0 (forward):       v = relu?(v + bias)
// MODE 1 (data gradient): v = (v [+ ad if relu]) * mask [+ ad if !relu];  mask = keep if bits, else aux0[idx] > 0 if aux0, else 1.
// relu != 0 in MODE 1: the addend has NOT been through the ReLU mask yet (same mask: both are gradients wrt the output of
// the layer below), so it is added first and masked with the rest.  ad is the value loaded from aux1 (or from anywhere, if
// aux1 is null: the callers request the addend row up front, without a branch around the load).
// (a statement macro: as a function, by value, the data gradient's instances kept the parent's instruction counts but not
// their order -- profiles/winograd_transform_refactor.txt.)  v: the value, updated in place; V: its type.
#define NFS_WG_EPILOGUE(MODE, V, zero, v, bias, relu, aux1, ad, bits, keep, aux0, idx)          \
  do {                                                                                           \
    if (MODE == 0) {                                                                             \
      wg_add(v, bias);                                                                           \
      if (relu) wg_relu(v);                                                                      \
    } else {                                                                                     \
      const V adv_ = aux1 ? ad : V(zero);                                                        \
      if (relu) wg_add(v, adv_);                                                                 \
      if (bits) wg_keep(v, keep);                                                                \
      else if (aux0) wg_keep_positive(v, *reinterpret_cast<const V*>(aux0 + idx));               \
      if (!relu) wg_add(v, adv_);                                                                \
    }                                                                                            \
  } while (0)

// ==== F(4x4): 6 x 6 patches, 4 x 4 tiles, a float2 channel pair per thread ===================================================
// ReLU bit cache: one word per (4 x 4 tile, channel pair), bit NFS_WG4_BIT_SHIFT(row, col) + channel = (value > 0)
#define NFS_WG4_BIT_SHIFT(a, c) (((a) * 4 + (c)) * 2)
__device__ __forceinline__ uint32_t wg4_bit_pair(float2 v) { return (v.x > 0.f ? 1u : 0u) | (v.y > 0.f ? 2u : 0u); }
// Pooled data gradient: patch row / column p of 0..5 lies in neighbour tile NFS_WG4_NB_TILE(p) of three (0 the one before, 1 the
// tile itself, 2 the one after), at row / column NFS_WG4_NB_POS(p) inside it
// (macros: the six-wave kernel calls them with its run-time column, and as functions, simplified on their own before they
// are inlined, they left it another instruction order than the expressions written in place)
#define NFS_WG4_NB_TILE(p) ((p) == 0 ? 0 : ((p) == 5 ? 2 : 1))
#define NFS_WG4_NB_POS(p) ((p) == 0 ? 3 : ((p) == 5 ? 0 : (p) - 1))
// ==== F(5x5): 7 x 7 patches, 5 x 5 tiles, one channel per thread ==============================================================
// B^T (7 x 7) = {-2,4,5/2,-5,-1/2,1,0} {0,2,-2,-9/2,1/2,1,0} {0,-2,6,-7/2,-3/2,1,0} {0,1,-3/2,-2,3/2,1,0}
//               {0,-1,5/2,0,-5/2,1,0} {0,4,0,-5,0,1,0} {0,-2,4,5/2,-5,-1/2,1}
// A^T (5 x 7) = {1,1,1,1,1,1,0} {0,1,-1,2,-2,1/2,0} {0,1,1,4,4,1/4,0} {0,1,-1,8,-8,1/8,0} {0,1,1,16,16,1/16,1}
// (written for one float; a thread owns ONE channel of a tile: the deep layers have few tiles -- 200 at 25 x 25 and 8 views --
// and two channels per thread, as in the F(4x4) transforms, leave the chip with less than one wave per SIMD)
// (no FMA contraction in the two transforms, as in wg4_bt / wg4_at: every kernel that inlines them rounds alike)
__device__ __forceinline__ void w5_bt(const float* d, float* o) {
#pragma clang fp contract(off)
  o[0] = -2.f * d[0] + 4.f * d[1] + 2.5f * d[2] - 5.f * d[3] - 0.5f * d[4] + d[5];
  o[1] = 2.f * d[1] - 2.f * d[2] - 4.5f * d[3] + 0.5f * d[4] + d[5];
  o[2] = -2.f * d[1] + 6.f * d[2] - 3.5f * d[3] - 1.5f * d[4] + d[5];
  o[3] = d[1] - 1.5f * d[2] - 2.f * d[3] + 1.5f * d[4] + d[5];
  o[4] = -d[1] + 2.5f * d[2] - 2.5f * d[4] + d[5];
  o[5] = 4.f * d[1] - 5.f * d[3] + d[5];
  o[6] = -2.f * d[1] + 4.f * d[2] + 2.5f * d[3] - 5.f * d[4] - 0.5f * d[5] + d[6];
}
__device__ __forceinline__ void w5_at(const float* m, float* o) {
#pragma clang fp contract(off)
  const float s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
  o[0] = m[0] + s12 + s34 + m[5];
  o[1] = d12 + 2.f * d34 + 0.5f * m[5];
  o[2] = s12 + 4.f * s34 + 0.25f * m[5];
  o[3] = d12 + 8.f * d34 + 0.125f * m[5];
  o[4] = s12 + 16.f * s34 + 0.0625f * m[5] + m[6];
}

// ReLU bit cache: two words per (5 x 5 tile, channel PAIR), bit w5_bit_shift(row, col) + (channel & 1) of the 64 = (x > 0).
// A thread holds one channel: it collects its 25 bits at the even positions, and the two lanes of a pair merge theirs.
__device__ __forceinline__ int w5_bit_shift(int a, int c) { return 2 * (a * 5 + c); }
// gid = tile * channels + c; every lane of the wave calls this (one __shfl_xor per word), the even channel stores
__device__ __forceinline__ void w5_bits_store(uint32_t* bits, int64_t gid, int c, unsigned long long mask) {
  const uint32_t lo = (uint32_t)mask, hi = (uint32_t)(mask >> 32);
  const uint32_t plo = __shfl_xor(lo, 1, 64), phi = __shfl_xor(hi, 1, 64);       // the odd channel of the pair
  if (!(c & 1)) *reinterpret_cast<uint2*>(bits + gid) = make_uint2(lo | (plo << 1), hi | (phi << 1));   // 2 * (gid / 2)
}
// where the pair's two words are (one 8-byte load), and from them this channel's bits at the even positions
__device__ __forceinline__ const uint2* w5_bits_at(const uint32_t* bits, int64_t gid) {
  return reinterpret_cast<const uint2*>(bits + (gid & ~(int64_t)1));
}
__device__ __forceinline__ unsigned long long w5_bits_mask(uint2 mw, int c) {
  return (((unsigned long long)mw.y << 32) | mw.x) >> (c & 1);
}

// ---- filters: U_z[ci][co] = (G g G^T)[z], z = S r + q, packed [S * S][K/32][N][32]; S = 6 for F(4x4), 7 for F(5x5) ------------
// kind 0: GEMM K = Ci, N = Co, g = w[:, :, ci, co];  kind 1 (data gradient): K = Co, N = Ci, taps flipped
template <int S> __device__ __forceinline__ void wg_g(const float g0, const float g1, const float g2, float* u);
// G = [[1/4,0,0],[-1/6,-1/6,-1/6],[-1/6,1/6,-1/6],[1/24,1/12,1/6],[1/24,-1/12,1/6],[0,0,1]]
template <> __device__ __forceinline__ void wg_g<6>(const float g0, const float g1, const float g2, float* u) {
  u[0] = 0.25f * g0;
  u[1] = (-1.f / 6.f) * (g0 + g1 + g2);
  u[2] = (-1.f / 6.f) * (g0 - g1 + g2);
  u[3] = (1.f / 24.f) * g0 + (1.f / 12.f) * g1 + (1.f / 6.f) * g2;
  u[4] = (1.f / 24.f) * g0 - (1.f / 12.f) * g1 + (1.f / 6.f) * g2;
  u[5] = g2;
}
// G (7 x 3) = {-1/2,0,0} {-1/3,-1/3,-1/3} {1/9,-1/9,1/9} {1/36,1/18,1/9} {-1/60,1/30,-1/15} {32/45,16/45,8/45} {0,0,1}
template <> __device__ __forceinline__ void wg_g<7>(const float g0, const float g1, const float g2, float* u) {
  u[0] = -0.5f * g0;
  u[1] = (-1.f / 3.f) * (g0 + g1 + g2);
  u[2] = (1.f / 9.f) * (g0 - g1 + g2);
  u[3] = (1.f / 36.f) * g0 + (1.f / 18.f) * g1 + (1.f / 9.f) * g2;
  u[4] = (-1.f / 60.f) * g0 + (1.f / 30.f) * g1 - (1.f / 15.f) * g2;
  u[5] = (32.f / 45.f) * g0 + (16.f / 45.f) * g1 + (8.f / 45.f) * g2;
  u[6] = g2;
}

template <int S>
__global__ void __launch_bounds__(256) winograd_pack_tile_kernel(const float* __restrict__ w, float* __restrict__ up, int Ci,
                                                                 int Co, int kind) {
  const int Kc = kind == 0 ? Ci : Co, Nc = kind == 0 ? Co : Ci;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (int64_t)Kc * Nc) return;
  const int n = (int)(gid % Nc), k = (int)(gid / Nc);
  float g[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (kind == 0) g[r][s] = w[((int64_t)(r * 3 + s) * Ci + k) * Co + n];
      else g[r][s] = w[((int64_t)((2 - r) * 3 + (2 - s)) * Ci + n) * Co + k];
    }
  float t[S][3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    float u[S];
    wg_g<S>(g[0][s], g[1][s], g[2][s], u);
#pragma unroll
    for (int r = 0; r < S; ++r) t[r][s] = u[r];
  }
#pragma unroll
  for (int r = 0; r < S; ++r) {
    float u[S];
    wg_g<S>(t[r][0], t[r][1], t[r][2], u);
#pragma unroll
    for (int q = 0; q < S; ++q) up[(((int64_t)(r * S + q) * (Kc / 32) + k / 32) * Nc + n) * 32 + (k & 31)] = u[q];
  }
}

}  // namespace nfs
