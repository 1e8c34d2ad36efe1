/* C ABI of libnfs_flow.so: particles carried along a FLOW of the carrier field in K explicit Euler steps, and the sweep
 * that carries a gradient back along the path (csrc/flow.hip; transform.carrier_flow, --carrier_steps of target_field 'g'
 * of the 3-D particle stylizer, Styler.apply_carrier).  A build extension: the reference has no carrier grid at all.
 *
 * The tenth library beside libnfs_hip.so (include/nfs_hip.h) and libnfs_grid2d.so .. libnfs_carrier.so
 * (include/nfs_<key>.h each), whose ABIs it leaves as they are: it links against libnfs_hip.so and shares its error
 * channel -- nfs_last_error() of libnfs_hip.so reports what an entry point here refused -- its stream type and its NFS_E*
 * codes.  Same conventions as include/nfs_carrier.h: row-major float32 device tensors, every call asynchronous on the given
 * HIP stream, int return codes, no allocation.  The Python binding (_lib.py) derives its argument types from this file.
 *
 * The model.  u [X,Y,(Z),nd] is a VELOCITY over one unit of pseudo-time on the carrier grid (nd is 2 or 3, the grid
 * cell-centred over the whole domain, positions in array order with the domain at [0,1]; Z is ignored where nd == 2),
 * g2p the sampling of include/nfs_carrier.h (csrc/g2p_axis.h: linear or Catmull-Rom, taps clipped to the grid), h = 1 / K:
 *     path[0]   = p
 *     path[k+1] = path[k] + h g2p(u, path[k])                      k = 0 .. K-1         the particles arrive at path[K]
 *     lam[K]    = g_out                                            the gradient in path[K]
 *     lam[k]    = lam[k+1] + h J(path[k])^T lam[k+1]               k = K-1 .. 0         lam[0] is the gradient in p
 *     (J^T lam)[a] = n_a sum_taps (w'_a prod_{b != a} w_b) (u[cell] . lam)
 * n_a is the grid's length on axis a and w' the derivative of an axis weight in t (cubic) or dx (linear), with t and dx
 * taken from the clipped index exactly as the sampling takes them (csrc/g2p_axis.h, g2p_axis_d):
 *     cubic    -1.5 t^2 + 2 t - 0.5,   4.5 t^2 - 5 t,   -4.5 t^2 + 4 t + 0.5,   1.5 t^2 - t
 *     linear   -1, +1            (where both taps are clipped onto one cell the two terms cancel: the sample is constant)
 * The gradient in u is h sum_k g2p^T(lam[k+1]; path[k]): nfs_carrier_bwd over the K N "particles" path[0:K] with the
 * gradients lam[1:K+1] -- each one contiguous [K N, nd] slice of these buffers -- times h.  No entry point here scatters.
 * K = 1 is nfs_carrier_displace: path[1] is its p_out bit for bit.  The steps are explicit Euler; nothing else is built. */
#ifndef NFS_FLOW_H
#define NFS_FLOW_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_flow_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_flow_fwd, nfs_flow_bwd */
#define NFS_FLOW_ABI_VERSION 100

int nfs_flow_version(void);

/* nfs_flow_fwd: u [X,Y,(Z),nd], p [N,nd] -> path [K+1,N,nd], in one launch, one thread per particle walking its K steps.
 *   path[0] is a bit copy of p.  Every sample is bit for bit what nfs_g2p_fwd returns for u at path[k] (C = nd), and the
 *   step is the float32 product h v followed by the float32 sum, never a fused multiply-add, with h = 1.0f / K: path[k+1]
 *   is reproducible bit for bit from path[k] with nfs_g2p_fwd, one multiplication and one addition.
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null pointer, nd outside {2,3}, a grid size below
 *   1 (Z where nd == 3), N < 0, K < 1, (K + 1) N nd >= 2^62, or path overlapping u or p.  N == 0: success, nothing is
 *   launched. */
int nfs_flow_fwd(const float* u, const float* p, float* path, int nd, int X, int Y, int Z, int64_t N, int K, int cubic,
                 nfs_stream_t stream);

/* nfs_flow_bwd: u, path [K+1,N,nd] (of nfs_flow_fwd: path[K] is not read), g_out [N,nd] -> lam [K+1,N,nd], the sweep
 *   above in one launch, one thread per particle walking k downward.  lam[K] is a bit copy of g_out.  A pure gather: no
 *   atomics, no LDS, every element written once, bitwise reproducible.  Per step and component the float32 result is within
 *   the bound of tests/flow_ref.py (pull) of the float64 value at the same path[k] and lam[k+1].
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null pointer, nd outside {2,3}, a grid size below
 *   1, N < 0, K < 1, (K + 1) N nd >= 2^62, or lam overlapping u, path or g_out.  N == 0: success, nothing is launched. */
int nfs_flow_bwd(const float* u, const float* path, const float* g_out, float* lam, int nd, int X, int Y, int Z, int64_t N,
                 int K, int cubic, nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_FLOW_H */
