// Host-side helpers shared by the C-ABI entry points (error reporting, tuning knobs).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/sr_hip.h"

int sr_fail(int code, const char* msg);
int sr_check(hipError_t e, const char* what);
// compute units of the current device (cached per device)
int sr_device_cus();

// Tuning knobs (sr_core.hip): environment variable of the same name read once per process,
// overridable by sr_set_knob; -1 = unset.
enum SrKnob {
  K_LWK,            // SR_LWK=0: linears on the lin kernel instead of linear_wk_kernel (A/B)
  K_LWK_MINK,       // SR_LWK_MINK: linear_wk_kernel only for K above this
  K_RING_WIDE,      // SR_RING_WIDE: 0 off / > 0 block target of the row-streaming wgrad over 64-co tiles
  K_RING_PS,        // SR_RING_PS=0: pixel-shuffled dy off the ring wgrad (A/B)
  K_LWG,            // SR_LWG=0: 1x1 wgrads on the pp kernel instead of linear_wgrad_kernel (A/B)
  K_LWG_T,          // SR_LWG_T: block target of the linear_wgrad split plan
  K_RING_SPLITS,    // SR_RING_SPLITS: block target of the narrow ring wgrad split plan
  K_DCN_CPP,        // SR_DCN_CPP: channels per pass of the DCN scatter
  K_DCN_DBG,        // SR_DCN_DBG: DCN forward timing ablations (wrong results)
  K_DCN_R,          // SR_DCN_R: x-window margin of the fused DCN forward
  K_DCN_FUSED,      // SR_DCN_FUSED=0: unfused DCN forward (A/B)
  K_DCN_COORD_WIN,  // SR_DCN_COORD_WIN=0: global-memory coordinate gradients (A/B)
  K_DCN_GX_FX,      // SR_DCN_GX_FX: 32 / 64-bit fixed-point scatter image
  K_SWIN_ATTN_DBG,  // SR_SWIN_ATTN_DBG: fused attention timing ablations (wrong results)
  K_WG_ROW3,        // SR_WG_ROW3: 0 = the kernel-row wgrad off (pp kernel), > 0 = its bias-role group size
  K_PPH_GRID,       // SR_PPH_GRID: blocks of the persistent pph forward grid (default: the CU count)
  K_WG_PAIR,        // SR_WG_PAIR: 0 = the paired kernel-row wgrad off (two single calls), > 0 = its bias-role group size
  K_COUNT
};
int sr_knob(SrKnob k);

// [-1, 1] fp32 -> ubyte exactly as utils/img_util.py:minusone_one_tensor_to_ubyte_numpy: clamp,
// (t + 1) * 0.5, * 255 with individually rounded fp32 operations, round half to even, clip.  Shared by
// the validation-metric kernels (metrics.hip, niqe.hip) so that both see the host's pixel values.
__device__ __forceinline__ unsigned char quantise(float v) {
  v = fminf(fmaxf(v, -1.f), 1.f);
  float t = __fmul_rn(__fadd_rn(v, 1.f), 0.5f);
  t = rintf(__fmul_rn(t, 255.f));
  return (unsigned char)fminf(fmaxf(t, 0.f), 255.f);
}
// diagnostics buffer of per-block clock stamps (sr_conv3x3_set_stamps; null = off)
extern unsigned long long* g_sr_stamps;
