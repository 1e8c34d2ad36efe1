/* C ABI of libnfs_liquid.so: the ray weights of a LIQUID colour render -- front-to-back alpha compositing of a colour volume
 * over a background (csrc/liquid.hip; engine: engine.ColourRenderLoss(render="liquid"), --colour_render liquid of the two
 * colour stylizers).
 *
 * The sixth library beside libnfs_hip.so (include/nfs_hip.h), libnfs_grid2d.so (include/nfs_grid2d.h), libnfs_descent.so
 * (include/nfs_descent.h), libnfs_colour.so (include/nfs_colour.h) and libnfs_emission.so (include/nfs_emission.h), whose
 * ABIs it leaves as they are: it links against libnfs_hip.so and shares its error channel -- nfs_last_error() of
 * libnfs_hip.so reports what an entry point here refused -- its stream type and its NFS_E* codes.  Same conventions:
 * row-major float32 device tensors, every call asynchronous on the given HIP stream, int return codes, no allocation.  The
 * Python binding (_lib.py) derives its argument types from this file exactly as it does from nfs_hip.h.
 *
 * The model (conventions of nfs_colour.h: rays along D, the far end z = D - 1 first).  S_v = rotate(d, R_v) is the rotated
 * absorbing grey volume, q [D,H,W,C] the emission:
 *     B_v[z] = sum_{z' > z} S_v[z']                           exclusive running sum
 *     A_v[z] = exp(-tau B_v[z]) (1 - exp(-tau S_v[z]))        alpha of sample z seen through what lies in front of it
 *     w_v[z] = A_v[z] / S_v[z] = tau exp(-tau B_v[z]) phi(tau S_v[z]),   phi(x) = (1 - exp(-x)) / x,  phi(0) = 1
 *     t_v    = exp(-tau sum_z S_v[z])                         the ray's total transmittance
 *     J_v    = sum_z w_v[z] rotate(q, R_v)[z] + t_v bg        (nfs_colour_project_fwd with these weights, plus the background)
 * sum_z w S + t = 1 (the sum telescopes); with q = c0 d, J = c0 (1 - t) + t bg; 0 <= w <= tau where S >= 0.  There is no
 * maximum over the image: the weights of a ray depend on that ray alone. */
#ifndef NFS_LIQUID_H
#define NFS_LIQUID_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_liquid_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_liquid_weights */
#define NFS_LIQUID_ABI_VERSION 100

int nfs_liquid_version(void);

/* nfs_liquid_weights: d [D,H,W], rot [V,9] (row-major, as nfs_rotate_fwd) -> w [V,D,H,W] as above, and per ray
 *   t_total [V,H,W] = t and grey [V,H,W] = 1 - t (the image of nfs_rotate_render_fwd(liquid = 1)); grey and t_total may
 *   each be null.  One pass: one lane per ray, a wave on 64 consecutive x of one (view, row), far end first; a sample is
 *   gathered by nfs_rotate_fwd's border-replicating trilinear stencil (ray_coords and axis_setup per axis, common.h: every
 *   index is clamped into the volume whatever the matrix is; the corners come as x-pairs from 8-byte loads where W >= 2,
 *   and through tri_setup, which is the same three axis_setup calls, and eight scalar loads where W == 1), its weight
 *   written from the running sum held in a register, then the sample added to the sum.  Nothing of size [V,D,H,W] is read
 *   and no rotated volume is stored.
 *   Numerics: the transmittances go through the hardware exp2 (a result below the smallest normal float is flushed to
 *   zero); phi is a four-term series below tau S = 2^-5 (truncation below 2^-27 relative) and -expm1(-x) / x above it, so
 *   it keeps its relative accuracy as tau S -> 0.  A sample of -0.0 (the mark of nfs_smooth3d_relu_fwd) counts as 0: its
 *   weight is the finite tau exp(-tau B).  A NaN sample makes the weights from it to the near end of ITS ray, that ray's
 *   t_total and grey NaN, and touches no other ray.
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null d, rot or w, a size below 1,
 *   V * D * H * W >= 2^30 (every index the kernel forms is then an int), or an output (w, grey, t_total) that overlaps d,
 *   rot or another output. */
int nfs_liquid_weights(const float* d, const float* rot, float tau, float* w, float* grey, float* t_total, int V, int D,
                       int H, int W, nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_LIQUID_H */
