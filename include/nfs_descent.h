/* C ABI of libnfs_descent.so: the update kernels of Laplacian-normalised descent (csrc/descent.hip; engine:
 * engine.LapDescentState, optimizer 'lapnorm' of the grid stylizers).
 *
 * A library of its own beside libnfs_hip.so (include/nfs_hip.h) and libnfs_grid2d.so (include/nfs_grid2d.h), whose ABIs it
 * leaves as they are: it links against libnfs_hip.so and shares its error channel -- nfs_last_error() of libnfs_hip.so
 * reports what an entry point here refused -- its stream type and its NFS_E* codes.  Same conventions: row-major float32
 * device tensors, channels last, every call asynchronous on the given HIP stream, int return codes.  The Python binding
 * (_lib.py) derives its argument types from this file exactly as it does from nfs_hip.h. */
#ifndef NFS_DESCENT_H
#define NFS_DESCENT_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_descent_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_descent_step, nfs_advect_descent_fwd, nfs_advect2d_descent_fwd */
#define NFS_DESCENT_ABI_VERSION 100

int nfs_descent_version(void);

/* ---- one step of descent along a normalised gradient g (util.lap_normalize of dL/dx): x <- x - lr g ----------------------
 * nfs_descent_step: x[i] = fmaf(-lr, g[i], x[i]) for i < n, in place: ONE rounding per element, the unfused update of
 *   every variable (any shape: n counts floats).  n = 0 is a no-op; n < 0 or a null pointer returns NFS_EINVAL.  g may
 *   not alias x.
 * nfs_advect_descent_fwd (velocity variable, 3-D): in one pass per voxel
 *     vel [D,H,W,3] <- fmaf(-lr, g, vel)            the bits of nfs_descent_step
 *     adv_next [D,H,W] = advect(d0, new vel)        the bits of nfs_advect_fwd (C = 1) on the new velocity
 *     live_next (nullable) = that sample's live mask, nfs_live_mask_words(D,H,W) words: the bits of nfs_advect_fwd_live
 *   The velocity a voxel's back-trace needs is its own, so the pass is local (as in nfs_advect_bwd_adam_fwd_live): the
 *   composition's second launch and its 12-byte-per-voxel re-read of the velocity disappear.
 *   Shapes: any D, H, W >= 2 with D * H * W < 2^30.  A voxel count that is a multiple of 4 runs the lean stencil, four
 *   voxels of a wave's 256 per lane, as nfs_advect_fwd does there; any other count runs the reference stencil, one voxel
 *   per lane, as nfs_advect_fwd does there.  live_next is taken where nfs_advect_fwd_live is: a multiple of 4 voxels.
 *   Anything else, a null required pointer or an aliased buffer (adv_next with d0, vel or g; g with vel) returns
 *   NFS_EINVAL with nfs_last_error() set, before any launch.
 * nfs_advect2d_descent_fwd (velocity variable, 2-D): vel [H,W,2] <- fmaf(-lr, g, vel) and adv_next [H,W] = advect2d(d0,
 *   new vel): the bits of nfs_descent_step followed by nfs_advect2d_fwd (C = 1).  H, W >= 2, H * W < 2^30.
 * Every index a kernel forms is clamped into the grid before it is used, wherever the back-traced point lies (a NaN
 *   velocity reads index 0 on that axis and only its own voxel's sample is NaN). */
int nfs_descent_step(float* x, const float* g, int64_t n, float lr, nfs_stream_t stream);
int nfs_advect_descent_fwd(const float* d0, float* vel, const float* g, float lr, float* adv_next,
                           unsigned long long* live_next, int D, int H, int W, nfs_stream_t stream);
int nfs_advect2d_descent_fwd(const float* d0, float* vel, const float* g, float lr, float* adv_next, int H, int W,
                             nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_DESCENT_H */
