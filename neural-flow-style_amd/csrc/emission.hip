// libnfs_emission.so (include/nfs_emission.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and the other three libraries' alone.
// The emission model of a colour grid: a colour field c [n,C] (channels last) seen through a grey volume e [n]:
//   emission_fwd_*        q   = clamp01(c) * e                       (the expression of colour_clamp_gather_kernel, field.hip)
//   emission_bwd_*        g_c = g_q * e where 0 <= c <= 1, else +0   (the mask of clamp01_bwd_kernel)
//   emission_bwd_adam_*   the same g_c in registers, consumed by TF ApplyAdam on (c, m, v) in place (adam_tf_placed below)
// Memory-bound, one rounding per output.  Two forms of each:
//   *_vec<C>     a lane owns four consecutive floats of the flat [n * C] arrays (16-byte loads and stores: every array must
//                be 16-byte aligned) and reads e at flat / C -- one 64-bit division per lane, then a counter; the lane that
//                holds the last n * C % 4 floats finishes them one by one
//   *_scalar     a lane owns one float: any alignment of 4 (a view offset by one element)
// Bytes per voxel at C = 3: forward 12 (c) + 4 (e) + 12 (q) = 28; adjoint 40; fused update 4 + 4 * 12 read, 36 written
// against 40 + 84 of the adjoint followed by nfs_adam_tf_step.  No LDS, no atomics.
// Every index: n < 2^36 (checked), so n * C < 2^38 fits 64 bits with room and the grid stays below 2^31 blocks; e is read
// only at flat / C of a flat index below n * C.
#include "common.h"
#include "../../include/nfs_emission.h"

namespace nfs {

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float emission_adj(float g, float c, float e) { return (c >= 0.f && c <= 1.f) ? g * e : 0.f; }

// TF ApplyAdam of one element, bit for bit what nfs_adam_tf_step writes at that element's place.  adam_tf (source_ops.h)
// is the plain expression, and so is adam_kernel (field.hip); but that kernel is compiled with the compiler's default
// contraction, and its one expression came out three ways (read off its code object):
//   PLACE_BODY   the float4 body, flat index below n & ~3:       m = fma(b1, m, (1 - b1) g)     u = fma((1 - b2) g, g, b2 u)
//   PLACE_PAIR   the first two of a tail of two or three:        m = fma(1 - b1, g, b1 m)       u = fma((1 - b2) g, g, b2 u)
//   PLACE_LAST   the odd last element (a tail of one or three):  m = b1 m + (1 - b1) g          u = ((1 - b2) g) g + b2 u
// The plain expression here would be contracted by this kernel's own surroundings (it came out as PLACE_PAIR everywhere
// in the float4 form and as PLACE_LAST in the scalar form) and differ from the composition in the last bit of m from the
// second step on.  So the three forms are stated, with contraction off, and chosen by the element's place: the fused update
// equals nfs_emission_bwd + nfs_adam_tf_step at every length and alignment (tests/test_emission_kernels_gpu.py holds it
// there; a library whose adam_kernel contracts otherwise fails that test).  The update of x cannot contract: a quotient.
enum { PLACE_BODY = 0, PLACE_PAIR = 1, PLACE_LAST = 2 };
__device__ __forceinline__ int adam_place(int64_t i, int64_t total) {
  const int64_t body = total & ~(int64_t)3;
  if (i < body) return PLACE_BODY;
  return ((total & 3) >= 2 && i - body < 2) ? PLACE_PAIR : PLACE_LAST;
}
__device__ __forceinline__ void adam_tf_placed(float& x, float& m, float& u, float g, float lr_t, float b1, float b2,
                                               float eps, int place) {
#pragma clang fp contract(off)
  const float t1 = (1.f - b1) * g, t2 = (1.f - b2) * g, bu = b2 * u;
  if (place == PLACE_BODY) m = __builtin_fmaf(b1, m, t1);
  else if (place == PLACE_PAIR) m = __builtin_fmaf(1.f - b1, g, b1 * m);
  else m = b1 * m + t1;
  if (place == PLACE_LAST) u = t2 * g + bu;
  else u = __builtin_fmaf(t2, g, bu);
  x -= lr_t * m / (sqrtf(u) + eps);
}

// e at the (up to four) consecutive flat indices i4 .. i4 + cnt - 1
template <int C>
__device__ __forceinline__ void lane_e(const float* __restrict__ e, int64_t i4, int cnt, float ev[4]) {
  int64_t vox = i4 / C;
  int r = (int)(i4 - vox * C);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    ev[j] = j < cnt ? e[vox] : 0.f;
    if (++r == C) { r = 0; ++vox; }
  }
}

template <int C>
__global__ void __launch_bounds__(256) emission_fwd_vec(const float* __restrict__ c, const float* __restrict__ e,
                                                        float* __restrict__ q, int64_t total) {
  const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= total) return;
  const int cnt = total - i4 >= 4 ? 4 : (int)(total - i4);
  float ev[4];
  lane_e<C>(e, i4, cnt, ev);
  if (cnt == 4) {
    const float4 cv = *reinterpret_cast<const float4*>(c + i4);
    float4 o;
    o.x = clamp01(cv.x) * ev[0]; o.y = clamp01(cv.y) * ev[1]; o.z = clamp01(cv.z) * ev[2]; o.w = clamp01(cv.w) * ev[3];
    *reinterpret_cast<float4*>(q + i4) = o;
  } else {
    for (int j = 0; j < cnt; ++j) q[i4 + j] = clamp01(c[i4 + j]) * ev[j];
  }
}

__global__ void __launch_bounds__(256) emission_fwd_scalar(const float* __restrict__ c, const float* __restrict__ e,
                                                           float* __restrict__ q, int64_t total, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) q[i] = clamp01(c[i]) * e[i / C];
}

template <int C>
__global__ void __launch_bounds__(256) emission_bwd_vec(const float* __restrict__ g_q, const float* __restrict__ c,
                                                        const float* __restrict__ e, float* __restrict__ g_c,
                                                        int64_t total) {
  const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= total) return;
  const int cnt = total - i4 >= 4 ? 4 : (int)(total - i4);
  float ev[4];
  lane_e<C>(e, i4, cnt, ev);
  if (cnt == 4) {
    const float4 gv = *reinterpret_cast<const float4*>(g_q + i4);
    const float4 cv = *reinterpret_cast<const float4*>(c + i4);
    float4 o;
    o.x = emission_adj(gv.x, cv.x, ev[0]); o.y = emission_adj(gv.y, cv.y, ev[1]);
    o.z = emission_adj(gv.z, cv.z, ev[2]); o.w = emission_adj(gv.w, cv.w, ev[3]);
    *reinterpret_cast<float4*>(g_c + i4) = o;
  } else {
    for (int j = 0; j < cnt; ++j) g_c[i4 + j] = emission_adj(g_q[i4 + j], c[i4 + j], ev[j]);
  }
}

__global__ void __launch_bounds__(256) emission_bwd_scalar(const float* __restrict__ g_q, const float* __restrict__ c,
                                                           const float* __restrict__ e, float* __restrict__ g_c,
                                                           int64_t total, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) g_c[i] = emission_adj(g_q[i], c[i], e[i / C]);
}

template <int C>
__global__ void __launch_bounds__(256) emission_bwd_adam_vec(const float* __restrict__ g_q, float* __restrict__ c,
                                                             const float* __restrict__ e, float* __restrict__ m,
                                                             float* __restrict__ v, int64_t total, float lr_t, float b1,
                                                             float b2, float eps) {
  const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= total) return;
  const int cnt = total - i4 >= 4 ? 4 : (int)(total - i4);
  float ev[4];
  lane_e<C>(e, i4, cnt, ev);
  if (cnt == 4) {
    const float4 gv = *reinterpret_cast<const float4*>(g_q + i4);
    float4 cv = *reinterpret_cast<const float4*>(c + i4);
    float4 mv = *reinterpret_cast<const float4*>(m + i4);
    float4 uv = *reinterpret_cast<const float4*>(v + i4);
    adam_tf_placed(cv.x, mv.x, uv.x, emission_adj(gv.x, cv.x, ev[0]), lr_t, b1, b2, eps, PLACE_BODY);
    adam_tf_placed(cv.y, mv.y, uv.y, emission_adj(gv.y, cv.y, ev[1]), lr_t, b1, b2, eps, PLACE_BODY);
    adam_tf_placed(cv.z, mv.z, uv.z, emission_adj(gv.z, cv.z, ev[2]), lr_t, b1, b2, eps, PLACE_BODY);
    adam_tf_placed(cv.w, mv.w, uv.w, emission_adj(gv.w, cv.w, ev[3]), lr_t, b1, b2, eps, PLACE_BODY);
    *reinterpret_cast<float4*>(c + i4) = cv;
    *reinterpret_cast<float4*>(m + i4) = mv;
    *reinterpret_cast<float4*>(v + i4) = uv;
  } else {
    for (int j = 0; j < cnt; ++j) {
      float x = c[i4 + j], mi = m[i4 + j], ui = v[i4 + j];
      adam_tf_placed(x, mi, ui, emission_adj(g_q[i4 + j], x, ev[j]), lr_t, b1, b2, eps, adam_place(i4 + j, total));
      c[i4 + j] = x; m[i4 + j] = mi; v[i4 + j] = ui;
    }
  }
}

__global__ void __launch_bounds__(256) emission_bwd_adam_scalar(const float* __restrict__ g_q, float* __restrict__ c,
                                                                const float* __restrict__ e, float* __restrict__ m,
                                                                float* __restrict__ v, int64_t total, int C, float lr_t,
                                                                float b1, float b2, float eps) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  float x = c[i], mi = m[i], ui = v[i];
  adam_tf_placed(x, mi, ui, emission_adj(g_q[i], x, e[i / C]), lr_t, b1, b2, eps, adam_place(i, total));
  c[i] = x; m[i] = mi; v[i] = ui;
}

static int check_emission(const char* who, int64_t n, int C) {
  NFS_REQUIRE(n >= 1, "%s: n must be at least 1 (got %lld)", who, (long long)n);
  NFS_REQUIRE(n < ((int64_t)1 << 36), "%s: n must be below 2^36 voxels", who);
  NFS_REQUIRE(C >= 1 && C <= 4, "%s: C must be 1..4 (got %d)", who, C);
  return NFS_OK;
}

static bool aligned16(const void* a, const void* b, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

}  // namespace nfs

using namespace nfs;

// one launch of KERNEL<C> for the runtime C in 1..4
#define NFS_EMISSION_BY_C(KERNEL, grid, s, ...)                                                         \
  switch (C) {                                                                                          \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(256), 0, s, __VA_ARGS__); break;                   \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(256), 0, s, __VA_ARGS__); break;                   \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(256), 0, s, __VA_ARGS__); break;                   \
    default: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(256), 0, s, __VA_ARGS__); break;                  \
  }

extern "C" {

int nfs_emission_version(void) { return NFS_EMISSION_ABI_VERSION; }

int nfs_emission_fwd(const float* c, const float* e, float* q, int64_t n, int C, nfs_stream_t stream) {
  NFS_REQUIRE(c && e && q, "nfs_emission_fwd: null pointer");
  if (int err = check_emission("nfs_emission_fwd", n, C)) return err;
  NFS_REQUIRE((const float*)q != c && (const float*)q != e, "nfs_emission_fwd: q must not alias c or e");
  const int64_t total = n * C;
  hipStream_t s = as_stream(stream);
  if (aligned16(c, q)) {
    const dim3 grid(blocks_for((total + 3) / 4, 256));
    NFS_EMISSION_BY_C(emission_fwd_vec, grid, s, c, e, q, total)
  } else {
    hipLaunchKernelGGL(emission_fwd_scalar, dim3(blocks_for(total, 256)), dim3(256), 0, s, c, e, q, total, C);
  }
  return check_launch("nfs_emission_fwd");
}

int nfs_emission_bwd(const float* g_q, const float* c, const float* e, float* g_c, int64_t n, int C, nfs_stream_t stream) {
  NFS_REQUIRE(g_q && c && e && g_c, "nfs_emission_bwd: null pointer");
  if (int err = check_emission("nfs_emission_bwd", n, C)) return err;
  NFS_REQUIRE((const float*)g_c != g_q && (const float*)g_c != c && (const float*)g_c != e,
              "nfs_emission_bwd: g_c must not alias g_q, c or e");
  const int64_t total = n * C;
  hipStream_t s = as_stream(stream);
  if (aligned16(g_q, c, g_c)) {
    const dim3 grid(blocks_for((total + 3) / 4, 256));
    NFS_EMISSION_BY_C(emission_bwd_vec, grid, s, g_q, c, e, g_c, total)
  } else {
    hipLaunchKernelGGL(emission_bwd_scalar, dim3(blocks_for(total, 256)), dim3(256), 0, s, g_q, c, e, g_c, total, C);
  }
  return check_launch("nfs_emission_bwd");
}

int nfs_emission_bwd_adam(const float* g_q, float* c, const float* e, float* m, float* v, int64_t n, int C, float lr_t,
                          float beta1, float beta2, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(g_q && c && e && m && v, "nfs_emission_bwd_adam: null pointer");
  if (int err = check_emission("nfs_emission_bwd_adam", n, C)) return err;
  NFS_REQUIRE(c != m && c != v && m != v, "nfs_emission_bwd_adam: c, m and v must not alias one another");
  NFS_REQUIRE((const float*)c != g_q && (const float*)m != g_q && (const float*)v != g_q && (const float*)c != e &&
                  (const float*)m != e && (const float*)v != e,
              "nfs_emission_bwd_adam: c, m and v must not alias g_q or e");
  const int64_t total = n * C;
  hipStream_t s = as_stream(stream);
  if (aligned16(g_q, c, m, v)) {
    const dim3 grid(blocks_for((total + 3) / 4, 256));
    NFS_EMISSION_BY_C(emission_bwd_adam_vec, grid, s, g_q, c, e, m, v, total, lr_t, beta1, beta2, eps)
  } else {
    hipLaunchKernelGGL(emission_bwd_adam_scalar, dim3(blocks_for(total, 256)), dim3(256), 0, s, g_q, c, e, m, v, total, C,
                       lr_t, beta1, beta2, eps);
  }
  return check_launch("nfs_emission_bwd_adam");
}

}  // extern "C"
