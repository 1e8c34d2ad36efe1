/* C ABI of libnfs_exposure.so: the smoke colour render at a FIXED EXPOSURE -- emission-absorption without the maximum of
 * the grey image -- and its derivative with respect to the density it is seen through (csrc/exposure.hip; engine:
 * engine.ColourRenderLoss(render='exposure'), colour_render 'exposure' of the colour stylizers, target_field 'pc' of the
 * 3-D particle stylizer on smoke).
 *
 * The eighth library beside libnfs_hip.so (include/nfs_hip.h), libnfs_grid2d.so, libnfs_descent.so, libnfs_colour.so,
 * libnfs_emission.so, libnfs_liquid.so and libnfs_absorb.so (include/nfs_<key>.h each), whose ABIs it leaves as they are:
 * it links against libnfs_hip.so and shares its error channel -- nfs_last_error() of libnfs_hip.so reports what an entry
 * point here refused -- its stream type and its NFS_E* codes.  Same conventions: row-major float32 device tensors, every
 * call asynchronous on the given HIP stream, int return codes, no allocation.  The Python binding (_lib.py) derives its
 * argument types from this file exactly as it does from nfs_hip.h.
 *
 * The model (conventions of nfs_colour.h: rays along D, the running sum starting at the far end z = D - 1).  With
 * S = rotate(d, R_v) and Q[z,c] = rotate(q, R_v)[z,c], both by nfs_rotate_fwd's border-replicating trilinear stencil, tau
 * the transmit coefficient and kappa (``gain``) the exposure:
 *     T[z] = exp(-tau sum_{z' >= z} S[z'])     inclusive: nfs_render_fwd's transmittance, nfs_ray_weights' numerator
 *     w[z] = kappa tau T[z]                    no maximum anywhere: a weight depends on its own ray alone
 *     J[c] = sum_z w[z] Q[z,c]                 over black (nfs_colour_project_fwd of w)
 *     grey = sum_z w[z] S[z]
 * S e^{-tau S} <= (1 - e^{-tau S}) / tau term by term, so grey <= kappa (1 - t) with t = exp(-tau sum_z S): at kappa = 1 a
 * uniform colour c0 (q = c0 d) renders at most c0 (1 - t) and is never clipped.
 * At the gradient g_J of J, per ray, with q held constant: a[z] = sum_c g_J[c] Q[z,c] (= dL/dw[z]), and because
 * dw[z'] / dS[z] = -tau w[z'] for z' <= z and 0 beyond,
 *     g_S[z] = dL/dS[z] = -tau sum_{z' <= z} a[z'] w[z']         an inclusive prefix from z = 0 upwards
 * and dL/dd = rotate^T(g_S) (nfs_rotate_bwd).  Neither S nor d appears in g_S. */
#ifndef NFS_EXPOSURE_H
#define NFS_EXPOSURE_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_exposure_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_exposure_weights, nfs_exposure_absorb_bwd */
#define NFS_EXPOSURE_ABI_VERSION 100

int nfs_exposure_version(void);

/* nfs_exposure_weights: d [D,H,W], rot [V,9] (row-major, as nfs_rotate_fwd) -> w [V,D,H,W] and, unless null,
 *   grey [V,H,W], as above.  One pass: one lane per ray, a wave on 64 consecutive x of one (view, row), the far end
 *   z = D - 1 first with the running sum in a register; each sample is gathered on the fly (x-pairs where W >= 2, eight
 *   scalar corners where W == 1).  The only [V,D,H,W] traffic is w written.
 *   Numerics: T through the hardware exp2 as nfs_ray_weights forms it; kappa tau is one product formed once per ray.
 *   A sample of -0.0 counts as 0.  A NaN sample touches its own ray only.
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null d, rot or w, a size below 1,
 *   V * D * H * W >= 2^30 (every index the kernel forms is then an int), a tau or gain that is not finite and positive,
 *   or w or grey overlapping d, rot or one another. */
int nfs_exposure_weights(const float* d, const float* rot, float tau, float gain, float* w, float* grey, int V, int D, int H,
                         int W, nfs_stream_t stream);

/* nfs_exposure_absorb_bwd: g_img [V,H,W,C] (g_J above), q [D,H,W,C] with C in 1..4, rot [V,9], w [V,D,H,W] as
 *   nfs_exposure_weights wrote it for the same rot and tau -> g_s [V,D,H,W] as above.  One pass: one lane per ray, the near
 *   end z = 0 first with the prefix in a register; per sample one stencil gathers the C channels of q (the gather of
 *   nfs_liquid_absorb_bwd without its density: csrc/ray_gather.h), four samples' gathers issued before any is consumed.
 *   The only [V,D,H,W] traffic is w read and g_s written; nothing of size [V,D,H,W,C] is formed.
 *   g_s may be the very buffer w (a lane reads w[z] before it writes g_s[z]; the weights are then gone).
 *   A ray whose g_img is all zero gives zeros (of either sign).  A NaN in q or w touches its own ray only.
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null pointer, a size below 1, C outside 1..4,
 *   V * D * H * W >= 2^30, a tau that is not finite and positive, g_s overlapping g_img, q or rot, or g_s overlapping w
 *   without being w itself. */
int nfs_exposure_absorb_bwd(const float* g_img, const float* q, const float* rot, const float* w, float tau, float* g_s,
                            int V, int D, int H, int W, int C, nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_EXPOSURE_H */
