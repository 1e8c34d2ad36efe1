/* C ABI of libnfs_absorb.so: the derivative of a LIQUID colour render with respect to the density it is seen through
 * (csrc/absorb.hip; engine: engine.ColourRenderLoss.loss_and_grad(absorb=True), target_field 'pc' of the 3-D particle
 * stylizer).
 *
 * The seventh library beside libnfs_hip.so (include/nfs_hip.h), libnfs_grid2d.so (include/nfs_grid2d.h), libnfs_descent.so
 * (include/nfs_descent.h), libnfs_colour.so (include/nfs_colour.h), libnfs_emission.so (include/nfs_emission.h) and
 * libnfs_liquid.so (include/nfs_liquid.h), whose ABIs it leaves as they are: it links against libnfs_hip.so and shares its
 * error channel -- nfs_last_error() of libnfs_hip.so reports what an entry point here refused -- its stream type and its
 * NFS_E* codes.  Same conventions: row-major float32 device tensors, every call asynchronous on the given HIP stream, int
 * return codes, no allocation.  The Python binding (_lib.py) derives its argument types from this file exactly as it does
 * from nfs_hip.h.
 *
 * The model is nfs_liquid.h's (rays along D, the running sum starting at the far end z = D - 1).  With S = rotate(d, R_v)
 * and Q[z,c] = rotate(q, R_v)[z,c], both by nfs_rotate_fwd's border-replicating trilinear stencil:
 *     B[z] = sum_{z' > z} S[z']     w[z] = tau exp(-tau B[z]) phi(tau S[z])     t = exp(-tau sum_z S[z])
 *     J[c] = sum_z w[z] Q[z,c] + t bg[c]
 * At the gradient g_J of J, per ray, with q held constant:
 *     a[z] = sum_c g_J[c] Q[z,c]  (= dL/dw[z])        b = sum_c g_J[c] bg[c]  (= dL/dt)
 *     P[z] = sum_{z'' < z} a[z''] w[z'']              psi(x) = phi'(x) / phi(x) = 1 / (e^x - 1) - 1 / x,  psi(0) = -1/2
 *     g_S[z] = dL/dS[z] = tau (a[z] w[z] psi(tau S[z]) - P[z] - t b)
 * and dL/dd = rotate^T(g_S) (nfs_rotate_bwd).  With Q = kappa_c S the sum g_S[z] + w[z] sum_c g_J[c] kappa_c is
 * -tau t sum_c g_J[c] (bg[c] - kappa_c) for every z: the total derivative is constant along the ray. */
#ifndef NFS_ABSORB_H
#define NFS_ABSORB_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_absorb_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_liquid_absorb_bwd */
#define NFS_ABSORB_ABI_VERSION 100

int nfs_absorb_version(void);

/* nfs_liquid_absorb_bwd: g_img [V,H,W,C] (g_J above), q [D,H,W,C] with C in 1..4, d [D,H,W], rot [V,9] (row-major, as
 *   nfs_rotate_fwd), w [V,D,H,W] and t_total [V,H,W] as nfs_liquid_weights wrote them for the same d, rot and tau,
 *   bg [C] on the device -> g_s [V,D,H,W] as above.  One pass: one lane per ray, a wave on 64 consecutive x of one (view,
 *   row), the near end z = 0 first with P in a register; per sample one stencil gathers d and the C channels of q (x-pairs
 *   where W >= 2, eight scalar corners where W == 1).  The only [V,D,H,W] traffic is w read and g_s written; nothing of size
 *   [V,D,H,W,C] is formed.
 *   g_s may be the very buffer w (a lane reads w[z] before it writes g_s[z]; the weights are then gone).
 *   Numerics: psi is a five-term series below tau S = 1, the difference of two quotients from there to 32 and -1 / x
 *   beyond (csrc/absorb.hip states each branch's error); it is finite for every tau S >= 0.  A sample of -0.0 counts as 0.
 *   A ray whose t_total or weights are 0 gives finite results; a ray whose g_img is all zero gives zeros.  A NaN sample
 *   touches its own ray only.
 *   Returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null pointer, a size below 1, C outside 1..4,
 *   V * D * H * W >= 2^30 (every index the kernel forms is then an int), g_s overlapping g_img, q, d, rot, t_total or bg,
 *   or g_s overlapping w without being w itself. */
int nfs_liquid_absorb_bwd(const float* g_img, const float* q, const float* d, const float* rot, const float* w,
                          const float* t_total, const float* bg, float tau, float* g_s, int V, int D, int H, int W, int C,
                          nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_ABSORB_H */
