/* C ABI of libnfs_carrier.so: particles moved by a displacement field on a coarse CARRIER GRID, and the transpose of that
 * sampling in the grid -- the scatter of per-particle gradients onto grid cells (csrc/carrier.hip; transform.carrier_displace,
 * target_field 'g' of the 3-D particle stylizer, Styler.apply_carrier).  A build extension: the reference samples grids at
 * particles in its resampler only and never differentiates that.
 *
 * The ninth library beside libnfs_hip.so (include/nfs_hip.h), libnfs_grid2d.so, libnfs_descent.so, libnfs_colour.so,
 * libnfs_emission.so, libnfs_liquid.so, libnfs_absorb.so and libnfs_exposure.so (include/nfs_<key>.h each), whose ABIs it
 * leaves as they are: it links against libnfs_hip.so and shares its error channel -- nfs_last_error() of libnfs_hip.so
 * reports what an entry point here refused -- its stream type and its NFS_E* codes.  Same conventions: row-major float32
 * device tensors, every call asynchronous on the given HIP stream, int return codes, no allocation.  The Python binding
 * (_lib.py) derives its argument types from this file exactly as it does from nfs_hip.h.
 *
 * The model (conventions of nfs_g2p_fwd: nd is 2 or 3, the grid [X,Y,(Z),C] cell-centred over the whole domain, p [N,nd] in
 * array order with the domain at [0,1]; Z is ignored where nd == 2).  Per axis a of length n, x = p n and b = floor(x - 0.5):
 *     linear   taps b, b+1 clipped to [0, n-1], weights 1 - dx, dx with dx = x - (clipped b + 0.5)
 *     cubic    taps b-1 .. b+2 clipped, Catmull-Rom weights of t = x - (clipped b + 0.5)
 * and a tap of the particle is one tap per axis, its weight w = (w_0 w_1) w_2.  csrc/g2p_axis.h holds that rule once, for
 * nfs_g2p_fwd and for this library: indices and weights are the same text in both.
 *     v[i,c]    = sum_taps w_i,tap u[cell(i,tap), c]                      the sampling (nfs_g2p_fwd)
 *     p_out     = p + v                                                   C = nd: u is a displacement in the units of p
 *     g_u[j,c]  = sum_i sum_{taps: cell(i,tap) = j} w_i,tap g_v[i,c]      the transpose
 * Clipping makes several taps of one particle land on the same border cell: their weights add.  On an axis of length 1 every
 * tap lands on cell 0.  A particle outside the domain has |t| > 1 and weights that grow as |t|^3; nothing is cut off.
 *
 * Numerics of the transpose.  A contribution is the float32 product w g_v[i,c], w formed as the sampling forms it.  A block
 * is NFS_CARRIER_BLOCK consecutive particles.
 *   box route: the block sums its contributions in LDS in 64-bit FIXED POINT and adds every touched (cell, channel) to g_u
 *     ONCE, with a global float atomic.  The block's quantum is a power of two chosen from
 *         m = the largest over its particles of (prod_a sum_taps |w_a,tap|) max_c |g_v[i,c]|
 *     (no particle can add more than its m to one cell): quantum <= 2^NFS_CARRIER_QUANTUM_LOG2 m, no cell sum overflows
 *     2^62, each contribution is truncated toward zero by less than one quantum, and the integer sums do not depend on the
 *     order of the adds.  The sum is converted to float32 once.
 *   per-tap route: one global float atomic per tap and channel.
 * Across blocks the float atomics add in an order of their own: g_u is NOT bitwise reproducible from run to run (no
 * store-and-sum or slab-per-block form is built); within the float64 bound of tests/carrier_ref.py for any order.
 * A NaN or an infinity in g_v or in a weight sends its block down the per-tap route and reaches the cells of its own
 * particle's taps only. */
#ifndef NFS_CARRIER_H
#define NFS_CARRIER_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_carrier_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_carrier_displace, nfs_carrier_bwd */
#define NFS_CARRIER_ABI_VERSION 100

/* particles per block of nfs_carrier_bwd, and the exponent of its fixed-point quantum relative to m (above) */
#define NFS_CARRIER_BLOCK 256
#define NFS_CARRIER_QUANTUM_LOG2 (-52)

int nfs_carrier_version(void);

/* nfs_carrier_displace: u [X,Y,(Z),nd], p [N,nd] -> p_out [N,nd] = p + v and, unless null, v_out [N,nd] = v, in one
 *   launch, one thread per particle.  v is bit for bit what nfs_g2p_fwd returns for the same u, p and cubic (C = nd), and
 *   p_out is the float32 sum p + v.
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null u, p or p_out, nd outside {2,3}, a grid size
 *   below 1 (Z where nd == 3), N < 0, or p_out or v_out overlapping u, p or one another.  N == 0: success, nothing is
 *   launched. */
int nfs_carrier_displace(const float* u, const float* p, float* p_out, float* v_out, int nd, int X, int Y, int Z, int64_t N,
                         int cubic, nfs_stream_t stream);

/* nfs_carrier_bwd: g_v [N,C], p [N,nd] -> g_u [X,Y,(Z),C], the transpose above.  C is general (the stylizer calls it with
 *   C = nd).  g_u is OVERWRITTEN: the call zeroes it on the stream itself, then adds.
 *   Correct for any order of the particles; fast where consecutive particles are neighbours (transform.grid_order): a block
 *   whose cells -- the box its particles' taps span -- times C fit 8192 LDS accumulators takes the box route, any other the
 *   per-tap route (unsorted particles, a huge grid, a large C).  The decision is per block.
 *   route 0: each block decides for itself.  route 1: every block takes the per-tap route.
 *   n_box_blocks: null, or one device word that the call zeroes and into which every block that took the box route adds 1.
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null g_v, p or g_u, nd outside {2,3}, a grid size
 *   or C below 1, N < 0, a route outside {0,1}, X * Y * Z * C >= 2^31 (every cell index the kernel forms is then an int), or
 *   g_u or n_box_blocks overlapping g_v, p or one another.  N == 0: success, g_u (and n_box_blocks) zeroed, no further
 *   launch. */
int nfs_carrier_bwd(const float* g_v, const float* p, float* g_u, uint32_t* n_box_blocks, int nd, int X, int Y, int Z, int C,
                    int64_t N, int cubic, int route, nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_CARRIER_H */
