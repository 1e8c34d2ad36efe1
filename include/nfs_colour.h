/* C ABI of libnfs_colour.so: emission-absorption rendering of a COLOUR volume through the views (csrc/colour.hip; engine:
 * engine.ColourRenderLoss, target_field 'c' of the 3-D particle stylizer).
 *
 * The fourth library beside libnfs_hip.so (include/nfs_hip.h), libnfs_grid2d.so (include/nfs_grid2d.h) and
 * libnfs_descent.so (include/nfs_descent.h), whose ABIs it leaves as they are: it links against libnfs_hip.so and shares
 * its error channel -- nfs_last_error() of libnfs_hip.so reports what an entry point here refused -- its stream type and its
 * NFS_E* codes.  Same conventions: row-major float32 device tensors, channels last, every call asynchronous on the given
 * HIP stream, int return codes, no allocation.  The Python binding (_lib.py) derives its argument types from this file
 * exactly as it does from nfs_hip.h.
 *
 * The model.  A grey density d [D,H,W] absorbs, a colour volume q [D,H,W,C] emits.  Per view v with rotation R_v (rot
 * [V,9], row-major, acting on (D,H,W)-ordered normalised coordinates as in nfs_rotate_fwd), rays along D:
 *     S_v    = rotate(d, R_v)
 *     T_v[z] = exp(-tau sum_{z' >= z} S_v[z'])         far end (z = D - 1) first, as nfs_render_fwd
 *     w      = T_v / M_g(v)                             M_g = the max of the grey image over the views of group g
 *     J_v    = sum_z w[v,z] rotate(q, R_v)[z]           LINEAR in q
 * Sample coordinates and the border-replicating trilinear stencil are nfs_rotate_fwd's (lin_coord, tri_setup). */
#ifndef NFS_COLOUR_H
#define NFS_COLOUR_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_colour_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_ray_weights, nfs_colour_project_fwd, nfs_colour_project_bwd */
#define NFS_COLOUR_ABI_VERSION 100

int nfs_colour_version(void);

/* Every entry point returns NFS_EINVAL with nfs_last_error() set, before any launch, on a null pointer, a size below 1,
 * V * D * H * W >= 2^30 (every index a kernel forms is then an int or a product with C <= 4 held in 64 bits) and the
 * aliasing named below.
 *
 * nfs_ray_weights: w[v,z,y,x] = exp(-tau sum_{z' >= z} d_rot[v,z',y,x]) / gmax[v / (V / G)], the running sum far end
 *   first.  d_rot [V,D,H,W] is what nfs_rotate_render_fwd(d_rot=...) kept, gmax [G] what nfs_maxnorm_fwd wrote for the
 *   grey image; 1 <= G <= V and G divides V.  One lane per ray, a wave on 64 consecutive x.  w may alias d_rot (a lane
 *   reads a sample before it writes that sample's weight); it may not alias gmax.  gmax > 0 is the caller's duty: the
 *   division is unguarded, and a group whose grey image is identically zero gives w = inf (the grey path's own
 *   normalisation divides 0 by 0 there).
 * nfs_colour_project_fwd: img[v,y,x,c] = sum_z w[v,z,y,x] trilinear(q[...,c]; R_v x), C in 1..4.  One pass over the rays,
 *   the C channels of a sample from one stencil; nothing of size [V,D,H,W,C] is written.  img may alias neither q nor w.
 * nfs_colour_project_bwd: the transpose, g_q[corner,c] (+)= sum over views and samples of w g_img[v,y,x,c] times the
 *   corner's stencil weight.  overwrite != 0: the entry point zero-fills g_q first (a kernel on the same stream), else
 *   it accumulates into what g_q holds.  The sums are global float atomic adds in whatever order the lanes arrive:
 *   g_q is NOT bit-reproducible from run to run (callers that need that take nfs_rotate_bwd's tiled form per channel,
 *   as ops.colour_project_bwd can).  g_q may alias neither g_img nor w. */
int nfs_ray_weights(const float* d_rot, float tau, const float* gmax, int G, float* w, int V, int D, int H, int W,
                    nfs_stream_t stream);
int nfs_colour_project_fwd(const float* q, const float* rot, const float* w, float* img, int V, int D, int H, int W, int C,
                           nfs_stream_t stream);
int nfs_colour_project_bwd(const float* g_img, const float* rot, const float* w, float* g_q, int overwrite, int V, int D,
                           int H, int W, int C, nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_COLOUR_H */
