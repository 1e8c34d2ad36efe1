// libnfs_flow.so (include/nfs_flow.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and the other nine libraries' alone.
// Particles carried along a flow of the carrier field in K Euler steps of h = 1 / K, and the sweep that carries a gradient
// back along the stored path:
//   flow_fwd_kernel   path[0] = p, path[k+1] = path[k] + h g2p(u, path[k]): one thread per particle walks its K steps with
//                     the position in registers.  The sample is carrier_displace_kernel's body (g2p_axis.h's stencil and
//                     gather with nd and cubic at run time, as nfs_g2p_fwd runs them: the same bits); the step is
//                     __fadd_rn(x, __fmul_rn(h, v)) kept apart by flow_step, so that no contraction fuses it.
//   flow_bwd_kernel   lam[K] = g_out, lam[k] = lam[k+1] + h J(path[k])^T lam[k+1]: one thread per particle walks k
//                     downward with lam in registers.  Per tap s = u[cell] . lam (nd products), and per axis a the tap adds
//                     (w'_a prod_{b != a} w_b) s to J_a, the weight formed as (f_0 f_1) f_2 with f_a = w'_a; then
//                     lam_a += h (n_a J_a).  A gather: no atomics, no LDS.
// The gradient in u is not formed here: it is nfs_carrier_bwd over path[0:K] and lam[1:K+1] (ops.flow_grad).
// The sweep is templated on <ND, CUBIC>: the tap loops unroll, and the index, weight and derivative arrays are registers
// (docs/kernels/particles.md has the compiler's counts per instance).  The forward kernel is not: see the note above it.
// Every index: g2p_axis clamps every tap into [0, n-1] whatever the position is (NaN included), so every address of u lies
// inside the grid; cell offsets, particle offsets and the step stride N nd are 64-bit; (K + 1) N nd < 2^62 is checked.
#include "common.h"
#include "g2p_axis.h"
#include "ray_gather.h"
#include "../../include/nfs_flow.h"

namespace nfs {

struct FlowFwdArgs {
  const float* u;
  const float* p;
  float* path;
  int nd, n[3], cubic, K;
  float h;                // 1.0f / K, formed on the host (IEEE division)
  int64_t N;
};

struct FlowBwdArgs {
  const float* u;
  const float* path;
  const float* g_out;
  float* lam;
  int n[3], K;
  float h;                // 1.0f / K, formed on the host (IEEE division)
  int64_t N;
};

// x + h v as the float32 product followed by the float32 sum.  The toolchain's __fmul_rn and __fadd_rn are a plain * and +
// that the optimiser contracts into one fused multiply-add once they are inlined, so the product is handed through an empty
// asm statement, which the optimiser cannot see through: two roundings, whatever the contraction mode is.
__device__ __forceinline__ float flow_step(float x, float h, float v) {
  float hv = __fmul_rn(h, v);
  asm volatile("" : "+v"(hv));
  return __fadd_rn(x, hv);
}

// NOT templated, unlike the sweep below: nd and cubic are run-time values exactly as in g2p_kernel (splat.hip) and
// carrier_displace_kernel, and the body is theirs (the stencil of g2p_axis.h per axis, g2p_gather).  Which products and sums
// of g2p_axis the compiler contracts depends on what it sees around them -- with cubic a compile-time constant it fuses
// x = p n into t = x - (idx + 0.5) and not into floor(x - 0.5), the other way round from those two kernels, and the sample
// differs in the last bits (by more where clipped weights cancel) -- so the kernel that promises THEIR bits keeps THEIR form.
__global__ void __launch_bounds__(256) flow_fwd_kernel(FlowFwdArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  const int nd = a.nd;
  const int64_t step = a.N * nd;
  float* out = a.path + i * nd;
  float x[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int d = 0; d < 3; ++d)
    if (d < nd) {
      x[d] = a.p[i * nd + d];
      out[d] = x[d];
    }
  for (int k = 0; k < a.K; ++k) {
    int ix[3][4];
    float wx[3][4];
#pragma unroll
    for (int d = 0; d < 3; ++d) {            // (g2p_stencil with the position in registers)
      if (d < nd) {
        g2p_axis(x[d] * (float)a.n[d], a.n[d], a.cubic, ix[d], wx[d]);
      } else {
        ix[d][0] = 0; wx[d][0] = 1.f;
      }
    }
    float v[3] = {0.f, 0.f, 0.f};
    g2p_gather(a.u, nd, a.n, nd, a.cubic, ix, wx, [&](int c, float s) {
      if (c == 0) v[0] = s;
      if (c == 1) v[1] = s;
      if (c == 2) v[2] = s;
    });
    out += step;
#pragma unroll
    for (int d = 0; d < 3; ++d)
      if (d < nd) {
        x[d] = flow_step(x[d], a.h, v[d]);
        out[d] = x[d];
      }
  }
}

template <int ND, bool CUBIC>
__global__ void __launch_bounds__(256) flow_bwd_kernel(FlowBwdArgs a) {
  constexpr int TAPS = CUBIC ? 4 : 2, T2 = ND >= 3 ? TAPS : 1;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  const int n[3] = {a.n[0], a.n[1], a.n[2]};
  const float h = a.h;
  const int64_t step = a.N * ND;
  float lam[ND];
#pragma unroll
  for (int d = 0; d < ND; ++d) {
    lam[d] = a.g_out[i * ND + d];
    a.lam[(int64_t)a.K * step + i * ND + d] = lam[d];
  }
  for (int k = a.K - 1; k >= 0; --k) {
    const float* xk = a.path + (int64_t)k * step + i * ND;
    int ix[3][4];
    float wx[3][4], dw[3][4];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (d < ND) {
        const float x = xk[d] * (float)n[d];
        g2p_axis(x, n[d], CUBIC ? 1 : 0, ix[d], wx[d]);
        g2p_axis_d(x, CUBIC ? 1 : 0, ix[d], dw[d]);
      } else {
        ix[d][0] = 0; wx[d][0] = 1.f; dw[d][0] = 0.f;
      }
    }
    float J[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int ka = 0; ka < TAPS; ++ka)
#pragma unroll
      for (int kb = 0; kb < TAPS; ++kb) {
        const float w01 = wx[0][ka] * wx[1][kb], d0 = dw[0][ka] * wx[1][kb], d1 = wx[0][ka] * dw[1][kb];
        const int64_t rowb = (int64_t)ix[0][ka] * n[1] + ix[1][kb];
#pragma unroll
        for (int kc = 0; kc < T2; ++kc) {
          const float* uc = a.u + (ND >= 3 ? rowb * n[2] + ix[2][kc] : rowb) * ND;
          float s = uc[0] * lam[0];
#pragma unroll
          for (int c = 1; c < ND; ++c) s += uc[c] * lam[c];
          J[0] += (d0 * wx[2][kc]) * s;
          J[1] += (d1 * wx[2][kc]) * s;
          if (ND >= 3) J[2] += (w01 * dw[2][kc]) * s;
        }
      }
    float* out = a.lam + (int64_t)k * step + i * ND;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      lam[d] = lam[d] + h * ((float)n[d] * J[d]);
      out[d] = lam[d];
    }
  }
}

// the checks both entry points share; -> the number of floats of a [K+1,N,nd] buffer through *total
static int flow_check(const char* who, int nd, int X, int Y, int Z, int64_t N, int K, int64_t* total) {
  NFS_REQUIRE(nd == 2 || nd == 3, "%s: nd must be 2 or 3 (got %d)", who, nd);
  NFS_REQUIRE(X >= 1 && Y >= 1 && (nd == 2 || Z >= 1) && N >= 0,
              "%s: the grid sizes must be at least 1 and N at least 0 (got %d x %d x %d, N %lld)", who, X, Y, Z, (long long)N);
  NFS_REQUIRE(K >= 1, "%s: K, the number of steps, must be at least 1 (got %d)", who, K);
  NFS_REQUIRE(N < (((int64_t)1 << 62) / nd) / ((int64_t)K + 1), "%s: (K + 1) * N * nd must be below 2^62", who);
  *total = ((int64_t)K + 1) * N * nd;
  return NFS_OK;
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_flow_version(void) { return NFS_FLOW_ABI_VERSION; }

int nfs_flow_fwd(const float* u, const float* p, float* path, int nd, int X, int Y, int Z, int64_t N, int K, int cubic,
                 nfs_stream_t stream) {
  NFS_REQUIRE(u && p && path, "nfs_flow_fwd: null pointer (u, p and path are required)");
  int64_t total;
  if (int rc = flow_check("nfs_flow_fwd", nd, X, Y, Z, N, K, &total)) return rc;
  if (nd == 2) Z = 1;
  const int64_t nu = (int64_t)X * Y * Z * nd, np = N * nd;
  NFS_REQUIRE(!overlaps(path, total, u, nu) && !overlaps(path, total, p, np), "nfs_flow_fwd: path must not alias u or p");
  if (N == 0) return NFS_OK;
  FlowFwdArgs a{u, p, path, nd, {X, Y, Z}, cubic ? 1 : 0, K, 1.0f / (float)K, N};
  hipLaunchKernelGGL(flow_fwd_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, as_stream(stream), a);
  return check_launch("nfs_flow_fwd");
}

int nfs_flow_bwd(const float* u, const float* path, const float* g_out, float* lam, int nd, int X, int Y, int Z, int64_t N,
                 int K, int cubic, nfs_stream_t stream) {
  NFS_REQUIRE(u && path && g_out && lam, "nfs_flow_bwd: null pointer (u, path, g_out and lam are required)");
  int64_t total;
  if (int rc = flow_check("nfs_flow_bwd", nd, X, Y, Z, N, K, &total)) return rc;
  if (nd == 2) Z = 1;
  const int64_t nu = (int64_t)X * Y * Z * nd, np = N * nd;
  NFS_REQUIRE(!overlaps(lam, total, u, nu) && !overlaps(lam, total, path, total) && !overlaps(lam, total, g_out, np),
              "nfs_flow_bwd: lam must not alias u, path or g_out");
  if (N == 0) return NFS_OK;
  FlowBwdArgs a{u, path, g_out, lam, {X, Y, Z}, K, 1.0f / (float)K, N};
  const dim3 grid(blocks_for(N, 256)), block(256);
  hipStream_t s = as_stream(stream);
#define NFS_FLOW_LAUNCH(ND_, CUBIC_) hipLaunchKernelGGL((flow_bwd_kernel<ND_, CUBIC_>), grid, block, 0, s, a)
  if (nd == 2) { if (cubic) NFS_FLOW_LAUNCH(2, true); else NFS_FLOW_LAUNCH(2, false); }
  else         { if (cubic) NFS_FLOW_LAUNCH(3, true); else NFS_FLOW_LAUNCH(3, false); }
#undef NFS_FLOW_LAUNCH
  return check_launch("nfs_flow_bwd");
}

}  // extern "C"
