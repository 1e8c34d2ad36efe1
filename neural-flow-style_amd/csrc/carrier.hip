// libnfs_carrier.so (include/nfs_carrier.h), a library of its own that links against libnfs_hip.so for the error channel
// (nfs::set_error, api.hip) and leaves that library's ABI and the other seven libraries' alone.
// Particles moved by a displacement field on a coarse carrier grid, and the transpose of that sampling in the grid:
//   carrier_displace_kernel   v = g2p(u, p) (nfs_g2p_fwd's kernel with C = nd: the stencil, the tap order and the gather
//                             are g2p_axis.h's, the text splat.hip's g2p_kernel runs), p_out = p + v; one thread per particle
//   carrier_bwd_kernel        g_u[cell,c] = sum_i sum_taps w g_v[i,c]: a scatter of 2^nd or 4^nd taps x C per particle
// The scatter is where the time is.  One global float atomic per tap would be N x taps x C adds onto X Y Z C addresses
// (5e5 x 64 x 3 onto 47 000 at the workload's size): two thousand adds per address, issued from lanes that hold neighbouring
// particles and therefore the SAME addresses.  So a block sums in LDS everything that shares a destination, as
// p2g_fwd_lds_kernel does: particles arrive in the order of the grid (transform.grid_order), the taps of a block's 256
// particles span a small box of carrier cells [lo, hi] per axis (a min / max reduction of each particle's lowest and highest
// cell: g2p_axis's indices are non-decreasing in the tap), the box times C is accumulated in 64-bit fixed-point LDS words
// (ds_add_u64; sums independent of the order of the adds) and flushed with ONE global atomic per touched (cell, channel), the
// slots of the box walked so that consecutive lanes hold consecutive channels of consecutive cells of the last axis: runs
// of ext[last] x C contiguous floats.  A block whose box does not fit, whose values have no finite scale, or that is told
// not to (route 1) issues the per-tap atomics.  The decision is per block.
// Fixed point: m_i = (prod_a sum_taps |w_a,tap|) max_c |g_v[i,c]| bounds what particle i adds to any one cell (its taps'
// weights, coinciding after clipping or not, sum to at most that), so a cell sum of the block is below 256 max_i m_i =
// bound < 2^ebound; contributions are scaled by 2^kexp, kexp = 62 - ebound, and truncated toward zero: the quantum 2^-kexp
// is at most 2^-53 of max_i m_i (include/nfs_carrier.h states 2^-52), and no sum reaches 2^62.
// Every index: X Y Z C < 2^31 (checked), so cell and slot indices are ints; particle offsets are 64-bit.  g2p_axis clamps
// every tap into [0, n-1] whatever the position is (NaN included), and lo / hi are reductions of those very taps, so every
// LDS slot lies inside the box and every global address inside g_u.
#include "common.h"
#include "g2p_axis.h"
#include "ray_gather.h"
#include "../../include/nfs_carrier.h"

#include <math.h>

namespace nfs {

struct CarrierFwdArgs {
  const float* u;
  const float* p;
  float* p_out;
  float* v_out;
  int nd, n[3], cubic;
  int64_t N;
};

__global__ void __launch_bounds__(256) carrier_displace_kernel(CarrierFwdArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  int ix[3][4];
  float wx[3][4];
  g2p_stencil(a.p, i, a.nd, a.n, a.cubic, ix, wx);
  g2p_gather(a.u, a.nd, a.n, a.nd, a.cubic, ix, wx, [&](int c, float v) {
    if (a.v_out) a.v_out[i * a.nd + c] = v;
    a.p_out[i * a.nd + c] = a.p[i * a.nd + c] + v;
  });
}

constexpr int CAR_BLOCK = NFS_CARRIER_BLOCK;
constexpr int CAR_LDS = 8192;      // 64-bit LDS accumulators (64 KB: two blocks per CU)

struct CarrierBwdArgs {
  const float* g_v;
  const float* p;
  float* g_u;
  unsigned* n_box;
  int n[3], C, route;
  int64_t N;
};

// one contribution scaled by 2^kexp = fs fs2 (two factors: 2^kexp may exceed the float range), truncated toward zero
__device__ __forceinline__ unsigned long long carrier_fix64(float c, float fs, float fs2) {
  return (unsigned long long)(long long)(c * fs * fs2);
}

template <int ND, bool CUBIC>
__global__ void __launch_bounds__(CAR_BLOCK) carrier_bwd_kernel(CarrierBwdArgs a) {
  constexpr int TAPS = CUBIC ? 4 : 2, T2 = ND >= 3 ? TAPS : 1;
  extern __shared__ unsigned long long acc[];
  __shared__ int red[7 * 4];
  const int t = threadIdx.x, C = a.C;
  const int64_t i = (int64_t)blockIdx.x * CAR_BLOCK + t;
  const bool live = i < a.N;
  int ix[3][4];
  float wx[3][4];
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int k = 0; k < 4; ++k) { ix[d][k] = 0; wx[d][k] = 0.f; }
  if (live) g2p_stencil(a.p, i, ND, a.n, CUBIC ? 1 : 0, ix, wx);
  const float* gi = a.g_v + i * C;
  // every tap of this thread's particle: f(cell, w) with cell the linear index in the grid
  auto each_tap = [&](auto&& f) {
#pragma unroll
    for (int ka = 0; ka < TAPS; ++ka)
#pragma unroll
      for (int kb = 0; kb < TAPS; ++kb) {
        const float wab = wx[0][ka] * wx[1][kb];
#pragma unroll
        for (int kc = 0; kc < T2; ++kc) f(ix[0][ka], ix[1][kb], ix[2][kc], wab * wx[2][kc]);
      }
  };
  auto per_tap = [&]() {
    if (!live) return;
    each_tap([&](int c0, int c1, int c2, float w) {
      float* dst = a.g_u + (int64_t)((c0 * a.n[1] + c1) * a.n[2] + c2) * C;
      for (int c = 0; c < C; ++c) atomicAdd(dst + c, w * gi[c]);
    });
  };
  if (a.route != 0) { per_tap(); return; }

  // the block's box and the largest m_i (NaN and infinities count as infinite: no scale)
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
  float m = 0.f;
  if (live) {
    float ws = 1.f, gm = 0.f;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      lo[d] = ix[d][0]; hi[d] = ix[d][TAPS - 1];
      float sd = 0.f;
#pragma unroll
      for (int k = 0; k < TAPS; ++k) sd += fabsf(wx[d][k]);
      ws *= sd;
    }
    for (int c = 0; c < C; ++c) {
      const float g = fabsf(gi[c]);
      gm = (g > gm || g != g) ? g : gm;
    }
    m = ws * gm;
    if (!(m < 3.0e38f)) m = INFINITY;
  }
#pragma unroll
  for (int d = 0; d < ND; ++d) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[d] = min(lo[d], __shfl_xor(lo[d], o, 64));
      hi[d] = max(hi[d], __shfl_xor(hi[d], o, 64));
    }
    if ((t & 63) == 0) { red[(2 * d) * 4 + (t >> 6)] = lo[d]; red[(2 * d + 1) * 4 + (t >> 6)] = hi[d]; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) red[6 * 4 + (t >> 6)] = __float_as_int(m);
  __syncthreads();
  int ext[3] = {1, 1, 1};
  int64_t vol = 1;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    if (d < ND) {
      const int* r0 = red + (2 * d) * 4;
      const int* r1 = red + (2 * d + 1) * 4;
      lo[d] = min(min(r0[0], r0[1]), min(r0[2], r0[3]));
      hi[d] = max(max(r1[0], r1[1]), max(r1[2], r1[3]));
      ext[d] = hi[d] - lo[d] + 1;
      vol *= ext[d];
    } else {
      lo[d] = 0; hi[d] = 0;
    }
  }
  m = fmaxf(fmaxf(__int_as_float(red[24]), __int_as_float(red[25])), fmaxf(__int_as_float(red[26]), __int_as_float(red[27])));
  if (m == 0.f) return;                                       // every contribution of the block is a zero
  const float bound = (float)CAR_BLOCK * m;
  if (!(bound < 3.0e38f) || vol * C > CAR_LDS) { per_tap(); return; }
  int ebound;
  frexpf(bound, &ebound);
  const int kexp = 62 - ebound, k1 = min(kexp, 120);
  const float fs = ldexpf(1.f, k1), fs2 = ldexpf(1.f, kexp - k1);
  const int nslot = (int)vol * C;
  for (int s = t; s < nslot; s += CAR_BLOCK) acc[s] = 0ull;
  __syncthreads();
  if (live) {
    for (int c0 = 0; c0 < C; c0 += 4) {
      const int cn = min(4, C - c0);
      float g[4] = {0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < cn; ++c) g[c] = gi[c0 + c];
      each_tap([&](int i0, int i1, int i2, float w) {
        unsigned long long* dst = acc + (((i0 - lo[0]) * ext[1] + (i1 - lo[1])) * ext[2] + (i2 - lo[2])) * C + c0;
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < cn) atomicAdd(dst + c, carrier_fix64(w * g[c], fs, fs2));
      });
    }
  }
  __syncthreads();
  for (int s = t; s < nslot; s += CAR_BLOCK) {
    const unsigned long long q = acc[s];
    if (q == 0ull) continue;
    const int cell = s / C, c = s - cell * C;
    const int r = cell / ext[2];
    const int c2 = lo[2] + (cell - r * ext[2]);
    const int r1 = r / ext[1];
    const int c1 = lo[1] + (r - r1 * ext[1]), c0 = lo[0] + r1;
    atomicAdd(a.g_u + (int64_t)((c0 * a.n[1] + c1) * a.n[2] + c2) * C + c, (float)ldexp((double)(long long)q, -kexp));
  }
  if (t == 0 && a.n_box) atomicAdd(a.n_box, 1u);
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_carrier_version(void) { return NFS_CARRIER_ABI_VERSION; }

int nfs_carrier_displace(const float* u, const float* p, float* p_out, float* v_out, int nd, int X, int Y, int Z, int64_t N,
                         int cubic, nfs_stream_t stream) {
  NFS_REQUIRE(u && p && p_out, "nfs_carrier_displace: null pointer (u, p and p_out are required; v_out may be null)");
  NFS_REQUIRE(nd == 2 || nd == 3, "nfs_carrier_displace: nd must be 2 or 3 (got %d)", nd);
  NFS_REQUIRE(X >= 1 && Y >= 1 && (nd == 2 || Z >= 1) && N >= 0,
              "nfs_carrier_displace: the grid sizes must be at least 1 and N at least 0 (got %d x %d x %d, N %lld)", X, Y, Z,
              (long long)N);
  if (nd == 2) Z = 1;
  const int64_t nu = (int64_t)X * Y * Z * nd, np = N * nd;
  NFS_REQUIRE(!overlaps(p_out, np, u, nu) && !overlaps(p_out, np, p, np) && !overlaps(v_out, np, u, nu) &&
                  !overlaps(v_out, np, p, np) && !overlaps(v_out, np, p_out, np),
              "nfs_carrier_displace: p_out and v_out must not alias u, p or one another");
  if (N == 0) return NFS_OK;
  CarrierFwdArgs a{u, p, p_out, v_out, nd, {X, Y, Z}, cubic ? 1 : 0, N};
  hipLaunchKernelGGL(carrier_displace_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, as_stream(stream), a);
  return check_launch("nfs_carrier_displace");
}

int nfs_carrier_bwd(const float* g_v, const float* p, float* g_u, uint32_t* n_box_blocks, int nd, int X, int Y, int Z, int C,
                    int64_t N, int cubic, int route, nfs_stream_t stream) {
  NFS_REQUIRE(g_v && p && g_u, "nfs_carrier_bwd: null pointer (g_v, p and g_u are required; n_box_blocks may be null)");
  NFS_REQUIRE(nd == 2 || nd == 3, "nfs_carrier_bwd: nd must be 2 or 3 (got %d)", nd);
  NFS_REQUIRE(X >= 1 && Y >= 1 && (nd == 2 || Z >= 1) && C >= 1 && N >= 0,
              "nfs_carrier_bwd: the grid sizes and C must be at least 1 and N at least 0 (got %d x %d x %d, C %d, N %lld)", X,
              Y, Z, C, (long long)N);
  NFS_REQUIRE(route == 0 || route == 1, "nfs_carrier_bwd: route must be 0 (per block) or 1 (per-tap atomics) (got %d)",
              route);
  if (nd == 2) Z = 1;
  const int64_t cells = (int64_t)X * Y * Z;
  NFS_REQUIRE(cells < ((int64_t)1 << 31) && cells * C < ((int64_t)1 << 31), "nfs_carrier_bwd: X * Y * Z * C must be below 2^31");
  const int64_t nu = cells * C, ng = N * C, np = N * nd;
  const float* nb = reinterpret_cast<const float*>(n_box_blocks);
  NFS_REQUIRE(!overlaps(g_u, nu, g_v, ng) && !overlaps(g_u, nu, p, np) && !overlaps(nb, 1, g_v, ng) &&
                  !overlaps(nb, 1, p, np) && !overlaps(nb, 1, g_u, nu),
              "nfs_carrier_bwd: g_u and n_box_blocks must not alias g_v, p or one another");
  hipStream_t s = as_stream(stream);
  zero_words(g_u, nu, s);
  if (n_box_blocks) zero_words(n_box_blocks, 1, s);
  if (N > 0) {
    CarrierBwdArgs a{g_v, p, g_u, n_box_blocks, {X, Y, Z}, C, route, N};
    const dim3 grid(blocks_for(N, CAR_BLOCK)), block(CAR_BLOCK);
    const size_t lds = CAR_LDS * sizeof(unsigned long long);
#define NFS_CARRIER_LAUNCH(ND_, CUBIC_) hipLaunchKernelGGL((carrier_bwd_kernel<ND_, CUBIC_>), grid, block, lds, s, a)
    if (nd == 2) { if (cubic) NFS_CARRIER_LAUNCH(2, true); else NFS_CARRIER_LAUNCH(2, false); }
    else         { if (cubic) NFS_CARRIER_LAUNCH(3, true); else NFS_CARRIER_LAUNCH(3, false); }
#undef NFS_CARRIER_LAUNCH
  }
  return check_launch("nfs_carrier_bwd");
}

}  // extern "C"
