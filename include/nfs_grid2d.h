/* C ABI of libnfs_grid2d.so: the 2-D grid stylizer's field operators (csrc/grid2d.hip; engine: grid2d.py).
 *
 * A library of its own beside libnfs_hip.so (include/nfs_hip.h, whose ABI it leaves as it is): it links against that
 * library and shares its error channel -- nfs_last_error() of libnfs_hip.so reports what an entry point here refused --
 * its stream type and its NFS_E* codes.  Same conventions: row-major float32 device tensors, channels last, every call
 * asynchronous on the given HIP stream, int return codes.  The Python binding (_lib.py) derives its argument types from
 * this file exactly as it does from nfs_hip.h. */
#ifndef NFS_GRID2D_H
#define NFS_GRID2D_H

#include "nfs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what nfs_grid2d_version() returns; the Python binding refuses a library that reports another number.
 * 100: nfs_source2d_velocity_fwd / _bwd, nfs_advect2d_source_fwd / _bwd, nfs_advect2d_bwd_adam_fwd, nfs_transport_step2d */
#define NFS_GRID2D_ABI_VERSION 100

int nfs_grid2d_version(void);

/* ---- stylising a 2-D grid: the 2-D branches of advect (transform.py:583-588), curl(is_2d) (517-527) and _transport
 * (styler_base.py:59-89) as one path (engine: grid2d.py) -------------------------------------------------------------
 * Density d [H,W]; a velocity is [H,W,2] in nfs_advect2d_fwd's own units (component k moves along array axis k, one cell
 * along an axis of n nodes is 2/(n-1)).  The variables are the D = 1 restriction of the 3-D definitions of nfs_hip.h with the D
 * component dropped; D_A is the forward difference along array axis A, the last slice replicated.  src takes source_ops.h's
 * values:
 *   0  vel [H,W,2]               the velocity itself
 *   1  psi [H,W] (channel s2 of the 3-D stream function)   vel0 = -D_W psi, vel1 = D_H psi: nfs_curl_fwd(nd = 2) with its
 *                                two channels reversed, no scale factor, D_H vel0 + D_W vel1 = 0
 *   2  phi [H,W]                 vel0 = D_H phi, vel1 = D_W phi   (D_H vel1 = D_W vel0)
 *   3  a [H,W,2] = (psi, phi)    each part formed as above, then added once: vel = fl(stream part + potential part)
 * All transposes are gathers, summed in the order H then W, with no atomics (deterministic): g_psi = D_H^T g1 - D_W^T g0,
 * g_phi = D_H^T g0 + D_W^T g1.
 * nfs_source2d_velocity_fwd: vel [H,W,2] = the velocity of var (src 0: a copy).
 * nfs_source2d_velocity_bwd: g_var (shaped like the variable, overwritten) = the transpose applied to g_vel [H,W,2].
 * nfs_advect2d_source_fwd: out [H,W] = advect2d(d, vel(var)), the velocity formed in registers and never stored;
 *   bit-identical to nfs_advect2d_fwd (C = 1) on the materialised velocity.
 * nfs_advect2d_source_bwd: g_vel [H,W,2] only (d is constant: no scatter); bit-identical to nfs_advect2d_bwd's g_vel on
 *   the stored velocity.
 * nfs_advect2d_bwd_adam_fwd (target 'v'): that velocity gradient consumed on the spot by TF ApplyAdam
 *   (nfs_adam_tf_step's expression) on vel, m, v [H,W,2] in place, and adv_next (nullable) [H,W] = advect2d(d, updated vel)
 *   -- all local to the pixel, as in nfs_advect_bwd_adam_fwd.
 *   Targets 's', 'p', 'sp' update through nfs_source2d_velocity_bwd followed by nfs_adam_tf_step.
 * nfs_transport_step2d: out [H,W,C] = w_g * advect2d(g, scale * u) + w_addend * addend (addend nullable) for any C >= 1:
 *   the 2-D twin of nfs_transport_step, on its lean form of the stencil (the coordinate in cells by one FMA, clamped
 *   into the grid, weights in [0,1], chained FMAs): the same sample as nfs_advect2d_fwd's to rounding, exact where u = 0.
 * Shapes: H, W >= 2 of any parity and H * W < 2^30; anything else, a null required pointer or src outside 0..3 returns
 *   NFS_EINVAL with nfs_last_error() set and writes nothing.  out must not alias d / var / g / u; g_vel none of its inputs;
 *   adv_next none of d, g_out, vel, m, v.
 * Every index a kernel forms is clamped into [0,H) x [0,W) before it is used, wherever the back-traced point lies: a
 *   pixel traced past a border reads the border cell (both corners of that axis clipped to it, the reference's stencil);
 *   a pixel whose velocity is NaN reads index 0 on that axis and its own result is NaN (nfs_transport_step2d: the value
 *   at index 0) -- no other pixel's is. */
int nfs_source2d_velocity_fwd(const float* var, int src, float* vel, int H, int W, nfs_stream_t stream);
int nfs_source2d_velocity_bwd(const float* g_vel, int src, float* g_var, int H, int W, nfs_stream_t stream);
int nfs_advect2d_source_fwd(const float* d, const float* var, int src, float* out, int H, int W, nfs_stream_t stream);
int nfs_advect2d_source_bwd(const float* d, const float* var, int src, const float* g_out, float* g_vel, int H, int W,
                            nfs_stream_t stream);
int nfs_advect2d_bwd_adam_fwd(const float* d, float* vel, const float* g_out, float* m, float* v, float* adv_next,
                              int H, int W, float lr_t, float beta1, float beta2, float eps, nfs_stream_t stream);
int nfs_transport_step2d(const float* g, const float* u, float scale, float w_g, const float* addend,
                         float w_addend, float* out, int H, int W, int C, nfs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NFS_GRID2D_H */
