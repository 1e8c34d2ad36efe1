// Error channel, version and device query of libnfs_hip.so.
#include "common.h"

namespace nfs {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace nfs

extern "C" {
int nfs_version(void) { return NFS_ABI_VERSION; }   // (include/nfs_hip.h) 1.5.9: + nfs_conv2d_plan, nfs_conv2d_group_plan (launch nothing); a sum_with_prev problem that carries bias, relu or y_pre is refused; 1.5.8: + nfs_conv3x3_plan (which kernels a conv shape runs; launches nothing); 1.5.7: + the 3-D resize of the grid octaves (nfs_resize3d); 1.5.6: + the gradient of a potential and the potential / Helmholtz variables (nfs_grad_fwd / _bwd, nfs_advect_potential_fwd / _bwd, nfs_advect_helmholtz_fwd / _bwd, nfs_potential_bwd_adam, nfs_helmholtz_bwd_adam); 1.5.5: + nfs_maxnorm_workspace_floats; 1.5.4: + nfs_p2g_has_instance; 1.5.3: + the differentiable MacCormack advection (nfs_advect_maccormack_keep / _bwd); 1.5.2: + the batched GEMM's test hook (nfs_gemm_last and its forcing twin); 1.5.1: + nfs_advect_bwd_adam_fwd_live_ever; 1.5: live masks (nfs_live_mask_words, nfs_advect_fwd_live, nfs_advect_bwd_adam_fwd_live, nfs_rotate_bwd_coef_live, nfs_rotate_live_workspace_ints); 1.4.1: the packed filters carry the 16 x 16 fragment order once more as bf16 limb planes (nfs_conv3x3_packed_floats grew by 54 (+ 73.5) floats per (ci, co)); 1.4: split-limb GEMMs by default (nfs_gemm_mode), round 2's limb planes gone from the packed filters (nfs_conv3x3_packed_floats shrank), nfs_gemm_timer_read_kind, nfs_slab_pack, nfs_lap_up_rms, the colour-chain operators; 1.3.3: packed filters carry two more layouts (nfs_conv3x3_packed_floats grew); 1.3.2: nfs_rotate_bwd overwrite; 1.3.1: addend_unmasked; 1.3: ReLU bit cache argument of the conv entry points; 1.2.1: + content loss; 1.2: fused pool conv, g2p, advect+Adam, max|g| hand-off
const char* nfs_last_error(void) { return nfs::g_err; }
int nfs_device_cus(void) {
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) {
    nfs::set_error("nfs_device_cus: no HIP device");
    return NFS_ELAUNCH;
  }
  return p.multiProcessorCount;
}
}
