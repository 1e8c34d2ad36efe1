// A8: SPH particle -> grid splat (transform.py:1233-1267 W, 1310-1453 p2g, 1577-1704
// p2g_wavg) and its adjoint.  The reference issues (2*nsize+1)^d separate ScatterNd ops
// with N x (d+1) index tensors each; here one thread owns a particle and evaluates the whole
// neighbourhood in registers.  Forward: the (nd, nsize) listed in with_instance have compile-time
// neighbourhoods and accumulate the cells of a block's 256 particles in 64-bit fixed-point LDS, one
// global float atomic per touched cell (p2g_fwd_lds_kernel); everything else scatters per cell with
// global float atomics (p2g_fwd_kernel).  Backward: a gather, no atomics -- from the block's box of
// the grid gradient staged in LDS for the instances (p2g_bwd_box_kernel), from global memory
// otherwise (p2g_bwd_kernel).  HBM-bound: N*(4*nd+4*C) B of particle data + the touched cells.
#include "common.h"
#include "g2p_axis.h"

#include <stdlib.h>

#include <type_traits>

namespace nfs {

// nfs_splat_cfg as the kernels read it: the kernel constants (support h, normalisation sigma, particle mass) worked out
// once on the host (make_dev_cfg)
struct SplatDev {
  int nd, mode, nsize, clip;
  int res[3];
  float dom[3];
  float cell, h, sigma, mass, rest_density;
};

__device__ __forceinline__ float cubic_w(float q, float sigma) {
  if (q > 1.f) return 0.f;
  if (q <= 0.5f) return sigma * (6.f * (q * q * q - q * q) + 1.f);
  const float t = 1.f - q;
  return sigma * 2.f * t * t * t;
}
__device__ __forceinline__ float cubic_dw(float q, float sigma) {
  if (q > 1.f) return 0.f;
  if (q <= 0.5f) return sigma * 6.f * (3.f * q * q - 2.f * q);
  const float t = 1.f - q;
  return -sigma * 6.f * t * t;
}

struct Particle {
  bool valid;
  int idx[3];
  float r[3];
  bool grad_ok[3];  // clip mode: gradient passes the clamp
};

__device__ __forceinline__ Particle load_particle(const SplatDev& s, const float* __restrict__ p, int64_t a) {
  Particle P;
  P.valid = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) { P.idx[k] = 0; P.r[k] = 0.f; P.grad_ok[k] = true; }
  for (int k = 0; k < s.nd; ++k) {
    float v = p[a * s.nd + k] * s.dom[k];
    if (s.clip) {
      const float hi = s.dom[k] - 1e-6f;
      P.grad_ok[k] = (v >= 0.f) && (v <= hi);
      v = fminf(fmaxf(v, 0.f), hi);
    } else if (!(v >= 0.f && v < s.dom[k])) {
      P.valid = false;
    }
    const float fl = floorf(v / s.cell);
    P.idx[k] = (int)fl;
    P.r[k] = v - (fl + 0.5f) * s.cell;
  }
  return P;
}

// linear cell index with the H flip of the reference (axis 0 in 2-D, axis 1 in 3-D), or -1
__device__ __forceinline__ int64_t cell_index(const SplatDev& s, const int* c) {
  int64_t lin = 0;
  const int hax = s.nd == 2 ? 0 : 1;
  for (int k = 0; k < s.nd; ++k) {
    if (c[k] < 0 || c[k] >= s.res[k]) return -1;
    const int ck = (k == hax) ? s.res[k] - 1 - c[k] : c[k];
    lin = lin * s.res[k] + ck;
  }
  return lin;
}

// coefficient of a particle's weights: mass (density), mass / density (colour), 1 (raw sums); pdv = the density a colour
// particle is divided by (the adjoint needs it again), 1 otherwise
__device__ __forceinline__ float mode_coef(const SplatDev& s, const float* __restrict__ pd, int64_t a, float& pdv) {
  pdv = (s.mode == 1) ? (pd ? pd[a] : s.rest_density) : 1.f;
  float coef = 1.f;
  if (s.mode == 0) coef = s.mass;
  if (s.mode == 1) coef = s.mass / pdv;
  return coef;
}

// The (2 nsize + 1)^nd neighbourhood of a particle with compile-time extents: the per-axis offsets r - n cell and their
// squares are formed once (3 x SP values instead of 3 per cell), the loops unroll, no integer division (hood_each
// below spends ~120 instructions per cell on o / span, o % span with a run-time span).  f(i0, i1, i2, d2) with
// i_k = n_k + NS in [0, SP); rr[k][i_k] = r_k - n_k cell.
template <int ND, int NS>
struct Hood {
  static constexpr int SP = 2 * NS + 1;
  float rr[3][SP];
  __device__ __forceinline__ void init(const SplatDev& s, const Particle& P) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int i = 0; i < SP; ++i) rr[k][i] = k < ND ? P.r[k] - (float)(i - NS) * s.cell : 0.f;
  }
  template <class F>
  __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
    for (int i0 = 0; i0 < SP; ++i0) {
      const float q0 = rr[0][i0] * rr[0][i0];
#pragma unroll
      for (int i1 = 0; i1 < SP; ++i1) {
        const float q01 = q0 + rr[1][i1] * rr[1][i1];
        if (ND == 2) {
          f(i0, i1, NS, q01);
        } else {
#pragma unroll
          for (int i2 = 0; i2 < SP; ++i2) f(i0, i1, i2, q01 + rr[2][i2] * rr[2][i2]);
        }
      }
    }
  }
};

// The same neighbourhood with run-time nd / nsize, for every (nd, nsize) without an instance and for grids of >= 2^31
// cells: f(c, rr, d2) with c the cell, rr[k] = r_k - n_k cell.  No early-out on d2: the callers form q = sqrtf(d2) / h.
template <class F>
__device__ __forceinline__ void hood_each(const SplatDev& s, const Particle& P, F&& f) {
  const int span = 2 * s.nsize + 1;
  const int total = s.nd == 2 ? span * span : span * span * span;
  for (int o = 0; o < total; ++o) {
    int n[3] = {0, 0, 0};
    if (s.nd == 2) { n[0] = o / span - s.nsize; n[1] = o % span - s.nsize; }
    else { n[0] = o / (span * span) - s.nsize; n[1] = (o / span) % span - s.nsize; n[2] = o % span - s.nsize; }
    float d2 = 0.f, rr[3] = {0.f, 0.f, 0.f};
    int c[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < s.nd) {
        rr[k] = P.r[k] - (float)n[k] * s.cell;
        d2 += rr[k] * rr[k];
        c[k] = P.idx[k] + n[k];
      }
    f(c, rr, d2);
  }
}

// The scatter with per-cell global atomics: any nd / nsize, 64-bit cell indices.
__global__ void __launch_bounds__(256) p2g_fwd_kernel(SplatDev s, const float* __restrict__ p,
                                                      const float* __restrict__ attr, const float* __restrict__ pd,
                                                      float* __restrict__ grid, float* __restrict__ wsum, int N,
                                                      int C) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const Particle P = load_particle(s, p, a);
  if (!P.valid) return;
  float pdv;
  const float coef = mode_coef(s, pd, a, pdv);
  hood_each(s, P, [&](const int* c, const float*, float d2) {
    const float w = cubic_w(sqrtf(d2) / s.h, s.sigma);
    if (w == 0.f) return;
    const int64_t ci = cell_index(s, c);
    if (ci < 0) return;
    if (s.mode == 0) {
      atomicAdd(grid + ci, coef * w);
    } else {
      for (int ch = 0; ch < C; ++ch) atomicAdd(grid + ci * C + ch, coef * w * attr[a * C + ch]);
      if (s.mode == 2) atomicAdd(wsum + ci, w);
    }
  });
}

// The box of cells the own cells of a block's 256 particles span, widened by NS and clipped to the grid: what the
// forward accumulates and the adjoint stages in LDS.  Written once, as statements that expand in the two kernels: behind
// a function call (a struct's members or free functions alike) the same lines moved the compiler's choice between fma
// and mul + add in Hood::each's d2 for the (2,1), (2,2), (2,3) adjoints and the (2,2) forward, and with it result bits.
// NFS_BOX_REDUCE: from each lane's lo / hi (its particle's cell, or 0x7fffffff / -1 without one) to the block's box:
// defines ext[3], vol (cells of the box) and any (the block has a live particle); red: 6 x 4 ints of LDS; t = threadIdx.x.
#define NFS_BOX_REDUCE(ND_, NS_)                                                                                         \
  _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                                       \
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) {                                                                \
      lo[k] = min(lo[k], __shfl_xor(lo[k], o, 64));                                                                      \
      hi[k] = max(hi[k], __shfl_xor(hi[k], o, 64));                                                                      \
    }                                                                                                                    \
    if ((t & 63) == 0) { red[(2 * k) * 4 + (t >> 6)] = lo[k]; red[(2 * k + 1) * 4 + (t >> 6)] = hi[k]; }                 \
  }                                                                                                                      \
  __syncthreads();                                                                                                       \
  int ext[3] = {1, 1, 1};                                                                                                \
  bool any = true;                                                                                                       \
  int64_t vol = 1;                                                                                                       \
  _Pragma("unroll") for (int k = 0; k < 3; ++k) {                                                                       \
    const int* r0 = red + (2 * k) * 4;                                                                                   \
    const int* r1 = red + (2 * k + 1) * 4;                                                                               \
    lo[k] = min(min(r0[0], r0[1]), min(r0[2], r0[3]));                                                                   \
    hi[k] = max(max(r1[0], r1[1]), max(r1[2], r1[3]));                                                                   \
    if (k < ND_) {                                                                                                       \
      any = any && hi[k] >= lo[k];                                                                                       \
      lo[k] = max(lo[k] - NS_, 0);                                                                                       \
      hi[k] = min(hi[k] + NS_, s.res[k] - 1);                                                                            \
      ext[k] = hi[k] - lo[k] + 1;                                                                                        \
      vol *= ext[k] > 0 ? ext[k] : 1;                                                                                    \
    } else {                                                                                                             \
      lo[k] = 0; hi[k] = 0;                                                                                              \
    }                                                                                                                    \
  }
// NFS_BOX_OFFSETS: defines off[3][SP], the address term of the cell along each axis for Hood's (i0, i1, i2), or -1
// outside the box (which is clipped to the grid): the slot of a cell is off[0][i0] + off[1][i1] + off[2][i2], and the
// cell lies outside when their OR is < 0
#define NFS_BOX_OFFSETS(ND_, NS_)                                                                                        \
  constexpr int SP = 2 * NS_ + 1;                                                                                        \
  int off[3][SP];                                                                                                        \
  _Pragma("unroll") for (int k = 0; k < 3; ++k)                                                                         \
    _Pragma("unroll") for (int i = 0; i < SP; ++i) {                                                                    \
      const int c = P.idx[k] + i - NS_;                                                                                  \
      const bool in = k < ND_ && c >= lo[k] && c <= hi[k];                                                               \
      const int stride = k == 0 ? ext[1] * ext[2] : (k == 1 ? ext[2] : 1);                                               \
      off[k][i] = in ? (c - lo[k]) * stride : (k < ND_ ? -1 : 0);                                                        \
    }
// NFS_BOX_CELL: defines c[3], the cell of slot i of the box
#define NFS_BOX_CELL(i_)                                                                                                 \
  int c[3];                                                                                                              \
  c[2] = lo[2] + (i_) % ext[2];                                                                                          \
  const int r = (i_) / ext[2];                                                                                           \
  c[1] = lo[1] + r % ext[1];                                                                                             \
  c[0] = lo[0] + r / ext[1];

// The same scatter with the block's cells privatised in LDS.  Particles arrive in the order of the grid (Styler.run
// sorts them once per sequence, by 8-cell bricks), so the own cells of a block's 256 particles sit in a small box
// [lo, hi] per axis -- and stay in one while a Lagrangian run moves them by a few cells.  When the box, widened by
// nsize, fits the LDS accumulators the block accumulates there (neighbouring particles share 18 of their 27 cells) and
// flushes each touched cell ONCE with a global atomic; otherwise (unsorted or very sparse particles: decided per block
// from a min / max reduction of the cell coordinates) it falls back to the per-cell global atomics above.  Same
// arithmetic per contribution.
//
// Round 4: the LDS accumulators are 64-bit FIXED POINT, as in the rotate adjoint (warp.hip; on gfx950 ds_add_f32
// sustains 0.33 lanes/clk/CU where ds_add_u64 runs at 9.4, tools/lds_atomic_bench.hip -- here that alone did not change
// the time, the index arithmetic was the bound; what it buys is sums that do not depend on the order of the adds).
// Every block scales by its own power of two, chosen from the largest
// |contribution| its particles can make (kernel maximum sigma x coefficient x largest |attribute|) times the
// particles per block, so that no cell sum can overflow 2^62; > 40 bits stay below the largest contribution (more than
// float accumulation keeps), and the integer sums do not depend on the order of the adds.
constexpr int SPL_LDS = 8192;      // 64-bit LDS accumulators (64 KB: two blocks per CU)

// The magnitude is converted and the integer negated: floor(c) and fract(c) of a NEGATIVE c with |c| < 1 are -1 and
// 1 - |c|, and the latter keeps 24 bits below 1 -- 2^8 quanta lost per contribution, which the cells that receive only
// small contributions of a block with large ones showed (tests/test_splat_gpu.py, attributes 1e-12 .. 1).  fract of a
// non-negative float is exact, so every contribution is now truncated toward zero by less than one quantum.
__device__ __forceinline__ unsigned long long splat_fix64(float c) {     // c = contribution * 2^(k - 32), |c| < 2^31
  const float a = fabsf(c);
  unsigned hi, lo;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(hi) : "v"(a));
  const float fr = __builtin_amdgcn_fractf(a) * 4294967296.f;
  asm("v_cvt_u32_f32 %0, %1" : "=v"(lo) : "v"(fr));
  const unsigned long long m = ((unsigned long long)hi << 32) | lo;
  return c < 0.f ? 0ull - m : m;
}

// One particle per thread, 256 per block.  A block whose box does not fit (15 % of the blocks of the 5e5-particle set:
// a block that straddles the end of a brick row, or sparse bricks far apart) sends its contributions to the grid with
// global atomics.  Measured in round 4 and removed (tools/splat_phase_bench.py on an ablation build): peeling such a
// block into groups that fit (first remaining particle's brick row, up to four bricks along the last axis; zero,
// accumulate, flush, repeat) -- 171 us against 116: every extra pass costs its own box reduction, LDS clear and flush
// (the flush runs at the global-atomic rate, ~85 G/s), more than the 29 us the scattered atomics of those blocks take.
// Where the 116 us go: block skeleton (reductions, LDS clear, barriers) ~40, accumulation ~45 (neighbouring lanes hold
// particles of the same cell: same-address LDS atomics serialise), flush ~35, fallback blocks ~29.
template <int ND, int NS>          // (ND, NS) = (nd, nsize) known at compile time
__global__ void __launch_bounds__(256) p2g_fwd_lds_kernel(SplatDev s, const float* __restrict__ p,
                                                          const float* __restrict__ attr, const float* __restrict__ pd,
                                                          float* __restrict__ grid, float* __restrict__ wsum, int N,
                                                          int C, int allow_lds) {
  extern __shared__ unsigned long long acc[];
  __shared__ int red[8 * 4];
  const int t = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * 256 + t;
  Particle P;
  P.valid = false;
  float coef = 1.f, at[4] = {0.f, 0.f, 0.f, 0.f}, cmax = 0.f;
  if (a < N) {
    P = load_particle(s, p, a);
    if (P.valid) {
      float pdv;
      coef = mode_coef(s, pd, a, pdv);
      float am = 1.f;
      if (s.mode != 0) {
        am = s.mode == 2 ? 1.f : 0.f;                   // (mode 2 also accumulates the bare weights)
        for (int ch = 0; ch < C; ++ch) { at[ch] = attr[a * C + ch]; am = fmaxf(am, fabsf(at[ch])); }
      }
      cmax = fabsf(coef) * am;                          // largest |coefficient x attribute| of this particle
    }
  }
  const int nch = s.mode == 0 ? 1 : (s.mode == 2 ? C + 1 : C);
  const float h2 = s.h * s.h, inv_h = 1.f / s.h;
  // one contribution of this thread's particle to cell c / LDS slot dst
  auto weight = [&](float d2) {
    // q = |r| / h as d2 * rsq(d2) * (1 / h): one v_rsq_f32 instead of a correctly rounded square root and a division
    // (~20 instructions per cell; 1-2 ulp in q, far inside the parity tolerance)
    return cubic_w(d2 > 0.f ? d2 * __frsqrt_rn(d2) * inv_h : 0.f, s.sigma);
  };
  auto to_global = [&](const int* c, float w) {
    const int64_t ci = cell_index(s, c);
    if (ci < 0) return;
    if (s.mode == 0) {
      atomicAdd(grid + ci, coef * w);
    } else {
      for (int ch = 0; ch < C; ++ch) atomicAdd(grid + ci * C + ch, coef * w * at[ch]);
      if (s.mode == 2) atomicAdd(wsum + ci, w);
    }
  };
  // the whole neighbourhood of the particle through global atomics
  auto all_global = [&]() {
    Hood<ND, NS> hd;
    hd.init(s, P);
    hd.each([&](int i0, int i1, int i2, float d2) {
      if (d2 > h2) return;
      const float w = weight(d2);
      if (w == 0.f) return;
      const int c[3] = {P.idx[0] + i0 - NS, P.idx[1] + i1 - NS, ND > 2 ? P.idx[2] + i2 - NS : 0};
      to_global(c, w);
    });
  };
  // block-wide maximum of cmax -> fixed-point scale 2^kexp: |any cell sum| <= 256 sigma cmax < 2^ebound stays below 2^62
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, o, 64));
  if ((t & 63) == 0) red[7 * 4 + (t >> 6)] = __float_as_int(cmax);
  __syncthreads();
  cmax = fmaxf(fmaxf(__int_as_float(red[28]), __int_as_float(red[29])), fmaxf(__int_as_float(red[30]), __int_as_float(red[31])));
  const float bound = 256.f * s.sigma * cmax;
  const bool scalable = bound > 0.f && bound < 3.0e38f;       // (inf / nan attributes: the float path reproduces them)
  int kexp = 0;
  float fs = 1.f, fs2 = 1.f;
  if (scalable) {
    int ebound;
    frexpf(bound, &ebound);
    kexp = 62 - ebound;
    const int ks = kexp - 32, k1 = min(max(ks, -120), 120);
    fs = ldexpf(1.f, k1);
    fs2 = ldexpf(1.f, ks - k1);                               // (2^ks may exceed the float range: two factors)
  }
  if (!(allow_lds && scalable)) {                             // NFS_SPLAT_LDS=0 / unscalable values: global atomics
    if (P.valid) all_global();
    return;
  }
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
  if (P.valid)
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = P.idx[k]; hi[k] = P.idx[k]; }
  NFS_BOX_REDUCE(ND, NS)
  if (!any) return;                                           // no live particle in the block
  if (vol * nch > SPL_LDS) {
    if (P.valid) all_global();
    return;
  }
  const int nvol = (int)vol;
  for (int i = t; i < nvol * nch; i += 256) acc[i] = 0ull;
  __syncthreads();
  if (P.valid) {
    Hood<ND, NS> hd;
    hd.init(s, P);
    NFS_BOX_OFFSETS(ND, NS)
    hd.each([&](int i0, int i1, int i2, float d2) {
      if (d2 > h2) return;
      if ((off[0][i0] | off[1][i1] | off[2][i2]) < 0) return;
      const float w = weight(d2);
      if (w == 0.f) return;
      unsigned long long* dst = acc + (off[0][i0] + off[1][i1] + off[2][i2]) * nch;
      if (s.mode == 0) {
        atomicAdd(dst, splat_fix64(coef * w * fs * fs2));
      } else {
        for (int ch = 0; ch < C; ++ch) atomicAdd(dst + ch, splat_fix64(coef * w * at[ch] * fs * fs2));
        if (s.mode == 2) atomicAdd(dst + C, splat_fix64(w * fs * fs2));
      }
    });
  }
  __syncthreads();
  for (int i = t; i < nvol; i += 256) {
    NFS_BOX_CELL(i)
    const unsigned long long* src = acc + (int64_t)i * nch;
    bool nz = false;
    for (int ch = 0; ch < nch; ++ch) nz = nz || src[ch] != 0ull;
    if (!nz) continue;
    const int64_t cell = cell_index(s, c);
#define NFS_SPL_F(q_) ((float)ldexp((double)(long long)(q_), -kexp))
    if (s.mode == 0) {
      atomicAdd(grid + cell, NFS_SPL_F(src[0]));
    } else {
      for (int ch = 0; ch < C; ++ch)
        if (src[ch] != 0ull) atomicAdd(grid + cell * C + ch, NFS_SPL_F(src[ch]));
      if (s.mode == 2 && src[C] != 0ull) atomicAdd(wsum + cell, NFS_SPL_F(src[C]));
    }
#undef NFS_SPL_F
  }
}


// WAVG: mode 2 with the adjoint of nfs_p2g_wavg_finish folded in -- g_grid is then dL/d(out) of the finished average,
// fin.xsum / fin.wsum the raw accumulators, and the gradients wrt the accumulators are formed per cell while the box is
// staged, instead of in a 5-array streaming pass over the whole grid (240 MB at 200 x 300 x 200).
struct WavgFinish { const float* xsum; const float* wsum; float eps; };

// adjoint of the weighted-average finish for one cell: gx[ch] = g / w and the return value -sum g x / w^2 where w > eps,
// g and 0 elsewhere
__device__ __forceinline__ float wavg_finish_adj(const WavgFinish& fin, const float* __restrict__ g_out, int64_t cell,
                                                 int C, float* gx) {
  const float w = fin.wsum[cell];
  float gw = 0.f;
  for (int ch = 0; ch < C; ++ch) {
    const float g = g_out[cell * C + ch];
    if (w > fin.eps) {
      gx[ch] = g / w;
      gw -= g * fin.xsum[cell * C + ch] / (w * w);
    } else {
      gx[ch] = g;
    }
  }
  return gw;
}

// the gradient of one cell as the adjoint reads it: gv[0..C) per channel, gv[C] wrt the weight sum (mode 2)
template <bool WAVG>
__device__ __forceinline__ void load_cell_grad(const SplatDev& s, const float* __restrict__ g_grid,
                                               const float* __restrict__ g_wsum, const WavgFinish& fin, int64_t cell,
                                               int C, float* gv) {
  if (WAVG) {
    gv[C] = wavg_finish_adj(fin, g_grid, cell, C, gv);
  } else {
    for (int ch = 0; ch < C; ++ch) gv[ch] = g_grid[cell * C + ch];
    if (s.mode == 2) gv[C] = g_wsum[cell];
  }
}

// One cell of a particle's neighbourhood added to its gradients gp / ga / gpd: gv the cell's gradient (load_cell_grad),
// q = |r| / h, rr the offsets r_k - n_k cell; over_dist_h(x) = x / (|r| h) in the caller's own arithmetic (the generic
// kernel divides, the box kernel multiplies by the rsq it already holds: the one place where the two differ).
template <class F>
__device__ __forceinline__ void adj_cell(const SplatDev& s, int nd, int C, float coef, float pdv, const float* at,
                                         const float* gv, float q, const float* rr, bool radial, F&& over_dist_h,
                                         float* gp, float* ga, float& gpd) {
  const float w = cubic_w(q, s.sigma);
  // dL/dW for this (particle, cell)
  float gw;
  if (s.mode == 0) {
    gw = coef * gv[0];
  } else {
    float dot = 0.f;
    for (int ch = 0; ch < C; ++ch) {
      dot += at[ch] * gv[ch];
      ga[ch] += coef * w * gv[ch];
    }
    // (mode 2 as ONE fma, the form both adjoints have always compiled to; written out so that it cannot move)
    gw = s.mode == 2 ? __fmaf_rn(coef, dot, gv[C]) : coef * dot;
    if (s.mode == 1) gpd -= coef * w * dot / pdv;
  }
  if (radial) {  // safe sqrt: zero gradient at the cell centre
    const float f = over_dist_h(gw * cubic_dw(q, s.sigma));
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < nd) gp[k] += f * rr[k];
  }
}

// the final stores of a particle's gradients
__device__ __forceinline__ void adj_store(const SplatDev& s, const Particle& P, int64_t a, int nd, int C, const float* gp,
                                          const float* ga, float gpd, float* __restrict__ g_p,
                                          float* __restrict__ g_attr, float* __restrict__ g_pd) {
  if (g_p)
    for (int k = 0; k < nd; ++k) g_p[a * nd + k] = P.grad_ok[k] ? gp[k] * s.dom[k] : 0.f;
  if (g_attr)
    for (int ch = 0; ch < C; ++ch) g_attr[a * C + ch] = ga[ch];
  if (g_pd) g_pd[a] = gpd;
}

// The gather from global memory: any nd / nsize, 64-bit cell indices.
__global__ void __launch_bounds__(256) p2g_bwd_kernel(SplatDev s, const float* __restrict__ p,
                                                      const float* __restrict__ attr, const float* __restrict__ pd,
                                                      const float* __restrict__ g_grid,
                                                      const float* __restrict__ g_wsum, float* __restrict__ g_p,
                                                      float* __restrict__ g_attr, float* __restrict__ g_pd, int N,
                                                      int C) {
  const int64_t a = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const Particle P = load_particle(s, p, a);
  float gp[3] = {0.f, 0.f, 0.f};
  float ga[4] = {0.f, 0.f, 0.f, 0.f};  // C <= 4
  float gpd = 0.f;
  if (P.valid) {
    float pdv;
    const float coef = mode_coef(s, pd, a, pdv);
    const float* at = attr + a * C;          // (read per cell, as in the forward)
    hood_each(s, P, [&](const int* c, const float* rr, float d2) {
      const float dist = sqrtf(d2);
      const float q = dist / s.h;
      if (q > 1.f) return;
      const int64_t ci = cell_index(s, c);
      if (ci < 0) return;
      float gv[5];
      load_cell_grad<false>(s, g_grid, g_wsum, WavgFinish{nullptr, nullptr, 0.f}, ci, C, gv);
      adj_cell(s, s.nd, C, coef, pdv, at, gv, q, rr, g_p && dist > 0.f, [&](float x) { return x / (dist * s.h); }, gp, ga,
               gpd);
    });
  }
  adj_store(s, P, a, s.nd, C, gp, ga, gpd, g_p, g_attr, g_pd);
}

// The adjoint with compile-time neighbourhoods and the block's box of the grid gradient staged in LDS: the 256 particles
// of a block (grid order) read the same ~1000 cells 27 times between them -- one coalesced pass brings them in, the
// gathers are LDS reads.  Same per-cell sums in the same order as p2g_bwd_kernel (cells in the order of the generic
// loop: axis 0 outermost), but not the same bits: q and 1 / (|r| h) come from one rsq here, from sqrtf and divisions
// there (1-2 ulp; each is held to the float64 bound of tests/splat_ref.py on its own).  A block whose box does not fit
// falls back to global gathers with this kernel's arithmetic.
constexpr int SPB_LDS = 12288;     // floats of staged gradient (48 KB)

template <int ND, int NS, bool WAVG>
__global__ void __launch_bounds__(256) p2g_bwd_box_kernel(SplatDev s, const float* __restrict__ p,
                                                          const float* __restrict__ attr, const float* __restrict__ pd,
                                                          const float* __restrict__ g_grid,
                                                          const float* __restrict__ g_wsum, float* __restrict__ g_p,
                                                          float* __restrict__ g_attr, float* __restrict__ g_pd, int N,
                                                          int C, WavgFinish fin) {
  extern __shared__ float gbox[];
  __shared__ int red[6 * 4];
  const int t = threadIdx.x;
  const int64_t a = (int64_t)blockIdx.x * 256 + t;
  Particle P;
  P.valid = false;
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
  if (a < N) {
    P = load_particle(s, p, a);
    if (P.valid)
#pragma unroll
      for (int k = 0; k < 3; ++k) { lo[k] = P.idx[k]; hi[k] = P.idx[k]; }
  }
  NFS_BOX_REDUCE(ND, NS)
  if (!any) {                                  // no live particle in the block: zero gradients
    if (a < N) {
      if (g_p) for (int k = 0; k < ND; ++k) g_p[a * ND + k] = 0.f;
      if (g_attr) for (int ch = 0; ch < C; ++ch) g_attr[a * C + ch] = 0.f;
      if (g_pd) g_pd[a] = 0.f;
    }
    return;
  }
  const int nch = s.mode == 2 ? C + 1 : C;     // (mode 0: C == 1)
  const bool staged = vol * nch <= SPB_LDS;
  const int nvol = (int)vol;
  if (staged) {
    for (int i = t; i < nvol; i += 256) {
      NFS_BOX_CELL(i)
      load_cell_grad<WAVG>(s, g_grid, g_wsum, fin, cell_index(s, c), C, gbox + i * nch);
    }
    __syncthreads();
  }
  if (a >= N) return;
  float gp[3] = {0.f, 0.f, 0.f};
  float ga[4] = {0.f, 0.f, 0.f, 0.f};  // C <= 4
  float gpd = 0.f;
  if (P.valid) {
    float pdv;
    const float coef = mode_coef(s, pd, a, pdv);
    float at[4] = {0.f, 0.f, 0.f, 0.f};
    if (s.mode != 0)
      for (int ch = 0; ch < C; ++ch) at[ch] = attr[a * C + ch];
    Hood<ND, NS> hd;
    hd.init(s, P);
    NFS_BOX_OFFSETS(ND, NS)
    const float h2 = s.h * s.h, inv_h = 1.f / s.h;
    hd.each([&](int i0, int i1, int i2, float d2) {
      if (d2 > h2) return;
      if ((off[0][i0] | off[1][i1] | off[2][i2]) < 0) return;
      const float inv_d = d2 > 0.f ? __frsqrt_rn(d2) : 0.f;       // (as in the forward kernel: rsq instead of sqrt + two divisions)
      const float dist = d2 * inv_d;
      const float q = dist * inv_h;
      if (q > 1.f) return;
      const int li = off[0][i0] + off[1][i1] + off[2][i2];
      float gv[5];
      if (staged) {
        for (int ch = 0; ch < nch; ++ch) gv[ch] = gbox[li * nch + ch];
      } else {
        const int c[3] = {P.idx[0] + i0 - NS, P.idx[1] + i1 - NS, P.idx[2] + i2 - NS};
        load_cell_grad<WAVG>(s, g_grid, g_wsum, fin, cell_index(s, c), C, gv);
      }
      const float rr[3] = {hd.rr[0][i0], hd.rr[1][i1], hd.rr[2][i2]};
      const float over = inv_d * inv_h;
      adj_cell(s, ND, C, coef, pdv, at, gv, q, rr, g_p && dist > 0.f, [&](float x) { return x * over; }, gp,
               ga, gpd);
    });
  }
  adj_store(s, P, a, ND, C, gp, ga, gpd, g_p, g_attr, g_pd);
}

__global__ void __launch_bounds__(256) wavg_finish_kernel(const float* __restrict__ xsum,
                                                          const float* __restrict__ wsum, float* __restrict__ out,
                                                          int64_t n, int C, float eps) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float w = wsum[i];
  for (int c = 0; c < C; ++c) out[i * C + c] = w > eps ? xsum[i * C + c] / w : xsum[i * C + c];
}

__global__ void __launch_bounds__(256) wavg_finish_bwd_kernel(WavgFinish fin, const float* __restrict__ g_out,
                                                              float* __restrict__ g_xsum, float* __restrict__ g_wsum,
                                                              int64_t n, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g_wsum[i] = wavg_finish_adj(fin, g_out, i, C, g_xsum + i * C);
}

static int make_dev_cfg(const nfs_splat_cfg* c, int C, SplatDev& s) {
  NFS_REQUIRE(c, "p2g: null config");
  NFS_REQUIRE(c->nd == 2 || c->nd == 3, "p2g: nd must be 2 or 3");
  NFS_REQUIRE(c->mode >= 0 && c->mode <= 2, "p2g: mode must be 0..2");
  NFS_REQUIRE(c->nsize >= 0 && c->nsize <= 8, "p2g: nsize out of range");
  NFS_REQUIRE(C >= 1 && C <= 4, "p2g: 1 <= C <= 4");
  s.nd = c->nd; s.mode = c->mode; s.nsize = c->nsize; s.clip = c->clip;
  for (int k = 0; k < 3; ++k) { s.res[k] = c->res[k]; s.dom[k] = c->domain[k]; }
  for (int k = 0; k < c->nd; ++k) NFS_REQUIRE(c->res[k] > 0 && c->domain[k] > 0.f, "p2g: bad res/domain");
  s.cell = c->domain[0] / (float)c->res[0];  // cell_size[0] (transform.py:1328-1330)
  s.h = c->radius * c->support;
  const double pi = 3.14159265358979323846;
  s.sigma = (float)(c->nd == 3 ? 8.0 / pi / ((double)s.h * s.h * s.h) : 40.0 / 7.0 / pi / ((double)s.h * s.h));
  const double d2r = 2.0 * c->radius;
  s.mass = (float)(0.8 * (c->nd == 3 ? d2r * d2r * d2r : d2r * d2r) * c->rest_density);
  s.rest_density = c->rest_density;
  return NFS_OK;
}


// ---- grid -> particle sampling (transform.py:771-1231) ---------------------------------------
// The axis rule (indices, weights), the stencil and the order of the taps are g2p_axis.h's, which libnfs_carrier.so's
// kernels (carrier.hip: the same sampling and its transpose in the grid) include too.  One thread per particle.
struct G2PArgs {
  const float* g;
  const float* p;
  float* out;
  int nd, n[3], C, cubic;
  int64_t N;
};

__global__ void __launch_bounds__(256) g2p_kernel(G2PArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.N) return;
  int ix[3][4];
  float wx[3][4];
  g2p_stencil(a.p, i, a.nd, a.n, a.cubic, ix, wx);
  g2p_gather(a.g, a.nd, a.n, a.C, a.cubic, ix, wx, [&](int c, float v) { a.out[i * a.C + c] = v; });
}

// ---- which kernel runs -------------------------------------------------------------------------------------------------
// THE list of compile-time (nd, nsize) instances (test_smokegun / chocolate: 3-D nsize 1; test_dambreak2d: 2-D nsize
// 2..4): f(ND, NS) as integral constants for the one that matches, false when there is none.  Both launchers and
// nfs_p2g_has_instance dispatch from here; an instance is added by adding its line.
template <class F>
static bool with_instance(const SplatDev& s, F&& f) {
#define NFS_SPLAT_INSTANCE(ND_, NS_)                                                        \
  if (s.nd == ND_ && s.nsize == NS_) {                                                      \
    f(std::integral_constant<int, ND_>{}, std::integral_constant<int, NS_>{});              \
    return true;                                                                            \
  }
  NFS_SPLAT_INSTANCE(3, 1)
  NFS_SPLAT_INSTANCE(3, 2)
  NFS_SPLAT_INSTANCE(2, 1)
  NFS_SPLAT_INSTANCE(2, 2)
  NFS_SPLAT_INSTANCE(2, 3)
  NFS_SPLAT_INSTANCE(2, 4)
#undef NFS_SPLAT_INSTANCE
  return false;
}

// the instanced kernels keep linear cell indices in 32 bits
static bool fits_int32(const SplatDev& s) {
  int64_t cells = 1;
  for (int k = 0; k < s.nd; ++k) cells *= s.res[k];
  return cells < ((int64_t)1 << 31);
}

// NFS_SPLAT_LDS=0: no LDS staging (read once per process)
static bool splat_lds() {
  static const int on = [] { const char* e = getenv("NFS_SPLAT_LDS"); return e ? atoi(e) : 1; }();
  return on != 0;
}

// the adjoint runs as p2g_bwd_box_kernel (and with it the one-launch weighted-average adjoint exists)
static bool has_box_adjoint(const SplatDev& s) {
  return splat_lds() && fits_int32(s) && with_instance(s, [](auto, auto) {});
}

// p2g adjoint launch: compile-time neighbourhoods with the box staged in LDS where they exist, the generic gather otherwise;
// fin != nullptr (mode 2): the adjoint of the weighted-average finish folded in (the generic kernel has no such form:
// the caller falls back to the two-step path)
static bool launch_p2g_bwd(const SplatDev& s, const float* p, const float* attr, const float* pd, const float* g_grid,
                           const float* g_wsum, float* g_p, float* g_attr, float* g_pd, int N, int C,
                           const WavgFinish* fin, hipStream_t stream) {
  const WavgFinish f = fin ? *fin : WavgFinish{nullptr, nullptr, 0.f};
  if (has_box_adjoint(s)) {
    with_instance(s, [&](auto nd, auto ns) {
      constexpr int ND = decltype(nd)::value, NS = decltype(ns)::value;
      if (fin)
        hipLaunchKernelGGL((p2g_bwd_box_kernel<ND, NS, true>), dim3(blocks_for(N, 256)), dim3(256),
                           SPB_LDS * sizeof(float), stream, s, p, attr, pd, g_grid, g_wsum, g_p, g_attr, g_pd, N, C, f);
      else
        hipLaunchKernelGGL((p2g_bwd_box_kernel<ND, NS, false>), dim3(blocks_for(N, 256)), dim3(256),
                           SPB_LDS * sizeof(float), stream, s, p, attr, pd, g_grid, g_wsum, g_p, g_attr, g_pd, N, C, f);
    });
    return true;
  }
  if (fin) return false;
  hipLaunchKernelGGL(p2g_bwd_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, stream, s, p, attr, pd, g_grid, g_wsum, g_p,
                     g_attr, g_pd, N, C);
  return true;
}

}  // namespace nfs

using namespace nfs;

extern "C" {

int nfs_p2g_has_instance(const nfs_splat_cfg* cfg_host) {
  SplatDev s;
  if (int e = make_dev_cfg(cfg_host, 1, s)) return e;
  return has_box_adjoint(s) ? 1 : 0;
}

int nfs_p2g_fwd(const float* p, const float* attr, const float* pd, float* grid, float* wsum, int N, int C,
                const nfs_splat_cfg* cfg_host, nfs_stream_t stream) {
  NFS_REQUIRE(p && grid && N > 0, "nfs_p2g_fwd: bad argument");
  SplatDev s;
  if (int e = make_dev_cfg(cfg_host, C, s)) return e;
  NFS_REQUIRE(s.mode == 0 || attr, "nfs_p2g_fwd: attr required for mode 1/2");
  NFS_REQUIRE(s.mode != 2 || wsum, "nfs_p2g_fwd: wsum required for mode 2");
  NFS_REQUIRE(s.mode != 0 || C == 1, "nfs_p2g_fwd: density mode has C=1");
  // 256 particles per block: measured 0.156 ms against 0.184 (512) and 0.247 (1024) on the 5e5-particle blob set.
  // NFS_SPLAT_LDS=0 keeps an instance's kernel and sends it down its global-atomic branch.
  const bool instanced = fits_int32(s) && with_instance(s, [&](auto nd, auto ns) {
    hipLaunchKernelGGL((p2g_fwd_lds_kernel<decltype(nd)::value, decltype(ns)::value>), dim3(blocks_for(N, 256)), dim3(256),
                       SPL_LDS * sizeof(unsigned long long), as_stream(stream), s, p, attr, pd, grid, wsum, N, C,
                       (int)splat_lds());
  });
  if (!instanced)
    hipLaunchKernelGGL(p2g_fwd_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, as_stream(stream), s, p, attr, pd, grid,
                       wsum, N, C);
  return check_launch("nfs_p2g_fwd");
}

int nfs_p2g_bwd(const float* p, const float* attr, const float* pd, const float* g_grid, const float* g_wsum,
                float* g_p, float* g_attr, float* g_pd, int N, int C, const nfs_splat_cfg* cfg_host,
                nfs_stream_t stream) {
  NFS_REQUIRE(p && g_grid && N > 0, "nfs_p2g_bwd: bad argument");
  SplatDev s;
  if (int e = make_dev_cfg(cfg_host, C, s)) return e;
  NFS_REQUIRE(s.mode == 0 || attr, "nfs_p2g_bwd: attr required for mode 1/2");
  NFS_REQUIRE(s.mode != 2 || g_wsum, "nfs_p2g_bwd: g_wsum required for mode 2");
  NFS_REQUIRE(s.mode != 0 || C == 1, "nfs_p2g_bwd: density mode has C=1");
  NFS_REQUIRE(s.mode != 0 || (!g_attr && !g_pd), "nfs_p2g_bwd: density mode has no attr/pd gradient");
  (void)launch_p2g_bwd(s, p, attr, pd, g_grid, g_wsum, g_p, g_attr, g_pd, N, C, nullptr, as_stream(stream));
  return check_launch("nfs_p2g_bwd");
}

/* nfs_p2g_wavg_finish_bwd + nfs_p2g_bwd (mode 2) in one launch: g_out [cells,C] = dL/d(finished average); returns
 * NFS_EINVAL where nfs_p2g_has_instance answers 0 (the caller then takes the two-step path) */
int nfs_p2g_wavg_bwd(const float* p, const float* attr, const float* xsum, const float* wsum, const float* g_out,
                     float* g_p, float* g_attr, int N, int C, float eps, const nfs_splat_cfg* cfg_host,
                     nfs_stream_t stream) {
  NFS_REQUIRE(p && attr && xsum && wsum && g_out && N > 0, "nfs_p2g_wavg_bwd: bad argument");
  SplatDev s;
  if (int e = make_dev_cfg(cfg_host, C, s)) return e;
  NFS_REQUIRE(s.mode == 2, "nfs_p2g_wavg_bwd: mode 2 (weighted average) only");
  const WavgFinish fin{xsum, wsum, eps};
  NFS_REQUIRE(launch_p2g_bwd(s, p, attr, nullptr, g_out, nullptr, g_p, g_attr, nullptr, N, C, &fin, as_stream(stream)),
              "nfs_p2g_wavg_bwd: nfs_p2g_has_instance is 0 for nd %d, nsize %d (no instance, >= 2^31 cells or "
              "NFS_SPLAT_LDS=0): use nfs_p2g_wavg_finish_bwd + nfs_p2g_bwd",
              s.nd, s.nsize);
  return check_launch("nfs_p2g_wavg_bwd");
}

int nfs_p2g_wavg_finish(const float* xsum, const float* wsum, float* out, int64_t n, int C, float eps,
                        nfs_stream_t stream) {
  NFS_REQUIRE(xsum && wsum && out && n > 0 && C > 0, "nfs_p2g_wavg_finish: bad argument");
  hipLaunchKernelGGL(wavg_finish_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream), xsum, wsum, out, n,
                     C, eps);
  return check_launch("nfs_p2g_wavg_finish");
}

int nfs_p2g_wavg_finish_bwd(const float* xsum, const float* wsum, const float* g_out, float* g_xsum, float* g_wsum,
                            int64_t n, int C, float eps, nfs_stream_t stream) {
  NFS_REQUIRE(xsum && wsum && g_out && g_xsum && g_wsum && n > 0 && C > 0, "nfs_p2g_wavg_finish_bwd: bad argument");
  hipLaunchKernelGGL(wavg_finish_bwd_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, as_stream(stream),
                     WavgFinish{xsum, wsum, eps}, g_out, g_xsum, g_wsum, n, C);
  return check_launch("nfs_p2g_wavg_finish_bwd");
}

int nfs_g2p_fwd(const float* g, const float* p, float* out, int nd, int X, int Y, int Z, int C, int64_t N, int cubic,
                nfs_stream_t stream) {
  NFS_REQUIRE(g && p && out, "nfs_g2p_fwd: null pointer");
  NFS_REQUIRE((nd == 2 || nd == 3) && X > 0 && Y > 0 && (nd == 2 || Z > 0) && C > 0 && N > 0,
              "nfs_g2p_fwd: bad dimension");
  G2PArgs a{g, p, out, nd, {X, Y, nd == 3 ? Z : 1}, C, cubic ? 1 : 0, N};
  hipLaunchKernelGGL(g2p_kernel, dim3(blocks_for(N, 256)), dim3(256), 0, as_stream(stream), a);
  return check_launch("nfs_g2p_fwd");
}

}  // extern "C"
