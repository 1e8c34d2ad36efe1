/* C ABI of libnfs_emission.so: the emission model of a colour GRID -- a colour field c [D,H,W,C] seen through a grey
 * volume e [D,H,W] that both absorbs and emits (csrc/emission.hip; engine: engine.ColourGridStylizer, grid_variable 'c' of
 * the grid-sequence stylizer).
 *
 * The fifth library beside libnfs_hip.so (include/nfs_hip.h), libnfs_grid2d.so (include/nfs_grid2d.h), libnfs_descent.so
 * (include/nfs_descent.h) and libnfs_colour.so (include/nfs_colour.h), whose ABIs it leaves as they are: it links against
 * libnfs_hip.so and shares its error channel -- nfs_last_error() of libnfs_hip.so reports what an entry point here
 * refused -- its stream type and its NFS_E* codes.  Same conventions: row-major float32 device tensors, channels last,
 * every call asynchronous on the given HIP stream, int return codes, no allocation.  The Python binding (_lib.py) derives
 * its argument types from this file exactly as it does from nfs_hip.h.
 *
 * The model.  e = smooth3d_relu(d) is the grey volume of one frame (a constant of the step), c the variable:
 *     q[i,ch]   = clamp01(c[i,ch]) * e[i]                     the emission nfs_colour_project_fwd renders
 *     g_c[i,ch] = g_q[i,ch] * e[i]  where 0 <= c[i,ch] <= 1,  else +0
 * clamp01 is the expression of nfs_colour_clamp_gather (fminf(fmaxf(x, 0), 1): a NaN colour goes to 0), the mask the
 * convention of nfs_clamp01_bwd (a colour exactly 0 or 1 passes its gradient, a NaN colour none).  e may carry the -0.0
 * with which nfs_smooth3d_relu_fwd marks the voxels its ReLU cut: the products are then zeros of the product's sign. */
#ifndef NFS_EMISSION_H
#define NFS_EMISSION_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_emission_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_emission_fwd, nfs_emission_bwd, nfs_emission_bwd_adam */
#define NFS_EMISSION_ABI_VERSION 100

int nfs_emission_version(void);

/* Every entry point returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null pointer, n < 1 or
 * n >= 2^36 voxels, C outside 1..4 and the aliasing named below.  n is the voxel count, the flat arrays hold n * C floats.
 * The flat arrays are read and written 16 bytes per lane where every one of them is 16-byte aligned, else float by float;
 * any alignment of 4 is taken.
 *
 * nfs_emission_fwd: q[i,ch] = clamp01(c[i,ch]) * e[i].  q may alias neither c nor e.
 * nfs_emission_bwd: g_c[i,ch] = g_q[i,ch] * e[i] where 0 <= c[i,ch] <= 1, else +0.  g_c may alias none of g_q, c, e.
 * nfs_emission_bwd_adam: the same g_c formed in registers and consumed on the spot by TF ApplyAdam on (c, m, v) in place
 *   (lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), the caller's): bit-equal to nfs_emission_bwd followed by
 *   nfs_adam_tf_step.  The mask is taken from c BEFORE its update.  c, m and v are written; they must be three different
 *   arrays and none of them g_q or e. */
int nfs_emission_fwd(const float* c, const float* e, float* q, int64_t n, int C, nfs_stream_t stream);
int nfs_emission_bwd(const float* g_q, const float* c, const float* e, float* g_c, int64_t n, int C, nfs_stream_t stream);
int nfs_emission_bwd_adam(const float* g_q, float* c, const float* e, float* m, float* v, int64_t n, int C, float lr_t,
                          float beta1, float beta2, float eps, nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_EMISSION_H */
