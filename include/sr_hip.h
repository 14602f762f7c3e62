/*
 * sr_hip.h — C ABI of the MI355X (gfx950) super-resolution engine (libsr_hip.so).
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json:north_star:
 * the SR network forward/backward (EDSR / RCAN / RRDBNet / SwinIR) and the three
 * native ops of basicsr/ops (DCN, fused_act, upfirdn2d).  Every entry point takes
 * plain device pointers, sizes and a hipStream_t (passed as void*), never allocates,
 * never synchronises, and returns 0 on success or a negative sr_status code; the
 * message of the last failure on the calling thread is available from
 * sr_last_error().  The Python host layer (basicsr4rs_amd/_lib.py) binds these with
 * ctypes and raises RuntimeError on a non-zero status, matching the reference's
 * TORCH_CHECK -> RuntimeError behaviour (basicsr/ops/dcn/src/deform_conv_cuda.cpp:511-516).
 *
 * Reference interfaces replaced (file:line in the reference checkout):
 *   sr_conv3x3_*         nn.Conv2d(C, C', 3, 1, 1) as instantiated in
 *                        basicsr/archs/arch_util.py:78-79, edsr_arch.py:44-48,
 *                        rcan_arch.py:40-42, rrdbnet_arch.py:21-25, swinir_arch.py:543
 *                        (cuDNN in the reference; no reference kernel exists)
 *   sr_pixel_shuffle     nn.PixelShuffle (arch_util.py:136,139) and
 *                        pixel_unshuffle (arch_util.py:217-234)
 *   sr_l1_loss           L1Loss (basicsr/losses/basic_loss.py:27-52)
 *   sr_dcn_*             deform_conv_ext.modulated_deform_conv_forward/backward
 *                        (basicsr/ops/dcn/src/deform_conv_ext.cpp:107-147)
 *   sr_fused_bias_act    fused_act_ext.fused_bias_act (basicsr/ops/fused_act/src/fused_bias_act.cpp:14-26)
 *   sr_upfirdn2d         upfirdn2d_ext.upfirdn2d (basicsr/ops/upfirdn2d/src/upfirdn2d.cpp:10-24)
 */
#ifndef SR_HIP_H
#define SR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum sr_dtype { SR_F32 = 0, SR_BF16 = 1 };
enum sr_status { SR_OK = 0, SR_EINVAL = -1, SR_ELAUNCH = -2, SR_ETOOBIG = -3 };
enum sr_act { SR_ACT_NONE = 0, SR_ACT_RELU = 1, SR_ACT_LRELU = 2 };

/* Library identity / error reporting. */
const char* sr_version(void);
const char* sr_last_error(void);
/* Tuning knobs (A/B switches and split-plan targets, not part of the reference interface).  Each
 * knob is its environment variable of the same name (SR_RING_SPLITS, SR_LWK, SR_DCN_GX_FX, ...), read
 * once per process; sr_set_knob overrides it at run time (value < 0: back to the built-in default)
 * and stores the previous value in *previous when non-NULL.  sr_get_knob returns the current value
 * (-1 unset, -2 unknown name). */
int sr_set_knob(const char* name, int value, int* previous);
int sr_get_knob(const char* name);

/* ---------------------------------------------------------------------------------
 * 3x3 convolution, stride 1, zero padding 1 (implicit GEMM on MFMA).
 *
 * Feature maps are NHWC with an explicit pixel stride (ld*) and channel offset
 * (*coff), element type `dtype`.  Channel counts are the padded GEMM counts
 * (multiples of 8); padded weight rows/columns are zero.
 *
 * Forward:  y = beta*res + alpha * gate_factor * act(conv(x, w) + bias)
 *   in_ps  = r > 0: x is the pixel-shuffled tensor [N, H*r, W*r, Cin/r^2] and GEMM
 *                   input channel k = (i*r + j)*(Cin/r^2) + c is gathered from it
 *                   (dgrad of an Upsample conv reads its pixel-shuffled grad directly).
 *   out_ps = r > 0: output GEMM column n = s*(Cout/r^2) + c is stored pixel-shuffled
 *                   at [n, y*r + s/r, x*r + s%r, c]  (nn.PixelShuffle fused in the store).
 *   out_nchw = 1:   store fp32 NCHW [N, Cout_real, H, W] as v*aff_scale[c] + aff_shift[c]
 *                   (EDSR/RCAN mean un-shift fused into conv_last).
 * w    : [Cout][ldw] GEMM weight rows, K index = tap*Cin + ci (tap = ky*3 + kx).
 * gate : optional, output layout; v *= (gate > 0 ? 1 : gate_slope)  (ReLU/LReLU backward).
 * ------------------------------------------------------------------------------- */
typedef struct sr_conv3x3_desc {
  int dtype;
  int N, H, W;
  int Cin, ldx, xcoff, in_ps;
  int Cout, Cout_real, ldw;
  int ldy, ycoff, out_ps, out_nchw;
  int act;
  float slope, alpha;
  int ldg, gcoff;
  float gate_slope;
  int ldr, rcoff;
  float beta;
  int ldr2, r2coff;
  float beta2;
  int rcols;  /* residuals apply to output columns n < rcols (0 = all) */
  int in_up;  /* x is the [N, H/u, W/u] map read through nearest-neighbour upsampling (0/1 = none) */
  int ksize;  /* 3 (default, 0 = 3) or 1: a 1x1 conv = nn.Linear over the NHWC tokens */
  int gate_mode; /* 0: v *= (gate > 0 ? 1 : gate_slope); 1: v *= gate (gate = the GELU' map a GELU
                  forward stored as its aux: the backward evaluates no erf);
                  2: after the residuals, v *= (gate > 0 ? 1 : gate_slope) on output columns
                  gcol0 <= n < gcol1 only (activation backward of a dense-block slice whose
                  gradient this call completes) */
  int gcol0, gcol1;
  const float* row_scale; /* optional fp32 [N]: alpha of every output pixel of image n is multiplied by
                             row_scale[n] (per-sample stochastic depth, swinir_arch.py:14-40, fused into
                             the proj / fc2 residual epilogues); NULL = 1 */
  const void* dot; /* optional, with colsum: the partial sums are of y * dot (bf16 [M][ldd], channel
                      columns dcoff.. in y's channel order) instead of y -- RCAN's channel-attention
                      backward dot sum_p dy * u (rcan_arch.py:19-27) fused into the conv dgrad that
                      produces dy; band kernel only (bf16, 64 -> 64 channels, W 64 / 128) */
  int ldd, dcoff;
} sr_conv3x3_desc;

/* A SwinIR block's LayerNorm fused into the following linear (norm1 -> attn.qkv, norm2 -> mlp.fc1:
 * basicsr/archs/swinir_arch.py:240, 251, 289-291, 320-323): y = Linear(LayerNorm(x)) on bf16
 * token rows [M][Cin] (dense, ldx == Cin), LayerNorm over the first ln_C channels (fp32 statistics,
 * eps), the normalised rows also written to ln_out [M][Cin] (padded columns zero) with the per-row
 * mean / rstd, as sr_layernorm_fwd would (they feed the weight gradient and the LayerNorm
 * backward).  The linear is sr_conv3x3_fwd's ksize-1 path with a plain (act 0) or GELU +
 * GELU' aux epilogue and Cin <= 192, Cout <= 640. */
int sr_linear_ln_fwd(const sr_conv3x3_desc* d, const void* x, const float* ln_gamma, const float* ln_beta, int ln_C,
                     float eps, void* ln_out, float* ln_mean, float* ln_rstd, const void* w, const float* bias, void* y,
                     void* aux, void* stream);


/* y = beta*res + beta2*res2 + alpha * gate_factor * act(conv(x, w) + bias); res/res2/gate may be NULL.
 * act: SR_ACT_* or 3 = GELU (exact erf).  aux (may be NULL): also store, in y's layout, GELU'(z) for
 * act 3 (z = conv(x, w) + bias; the fc2 dgrad's gate_mode-1 factor, computed with the GELU from one
 * erf) and z itself for the other activations.  colsum (may be NULL): fp32
 * [N * P][Cout] partial channel sums of y as stored, P = sr_conv3x3_fwd_colsum_parts(d) rows per
 * image, sum_p colsum[n*P + p][c] = sum over image n's pixels of y[n, pixel, c] -- RCAN's
 * AdaptiveAvgPool2d(1) (rcan_arch.py:19) fused into the conv that produces its input. */
int sr_conv3x3_fwd(const sr_conv3x3_desc* d, const void* x, const void* w, const float* bias,
                   const void* gate, const void* res, const void* res2, const float* aff_scale,
                   const float* aff_shift, void* y, void* aux, float* colsum, void* stream);
/* Partial rows per image of sr_conv3x3_fwd's colsum for this descriptor (0: not available). */
/* 1 when a call with this descriptor plus a residual, colsum and the dot operand (sr_conv3x3_desc.dot)
 * runs on the band kernel's fused epilogue, else 0 (the caller then computes the dot separately). */
int sr_conv3x3_fwd_dot_ok(const sr_conv3x3_desc* d);
int sr_conv3x3_fwd_colsum_parts(const sr_conv3x3_desc* d);

/* Name of the GPU kernel that sr_conv3x3_fwd / sr_conv3x3_wgrad would launch for a
 * descriptor (static string; for traces and profiler summaries). */
const char* sr_conv3x3_fwd_kernel_name(const sr_conv3x3_desc* d);
const char* sr_conv3x3_wgrad_kernel_name(const struct sr_conv3x3_wgrad_desc* d);
/* Number of kernel launches one sr_conv3x3_fwd call makes for a descriptor (1, or the 64-channel
 * output slices of the sliced band form) -- the per-launch unit of traces and profiler summaries. */
int sr_conv3x3_fwd_launches(const sr_conv3x3_desc* d);

/* Kernel-variant switch for the parity tests' cross-checks and A/B timing: 0 = automatic (default); every
 * other value routes one kernel family back to the kernel it replaced.  The one list of accepted values:
 * X(name, value), also what sr_conv3x3_set_variant validates against (basicsr4rs_amd/_lib.py mirrors it). */
#define SR_CONV_VARIANTS(X)                                                                                             \
  X(SR_VARIANT_AUTO, 0)                /* automatic selection */                                                        \
  X(SR_VARIANT_TILE_ONLY, 1)           /* every family -> the register-staged tile kernels (no 256x256, halo, band, lin, tail, ring, linear_wgrad) */ \
  X(SR_VARIANT_TWO_BARRIER, 2)         /* 256x256 forward and wgrad -> the two-barrier kernels (the previous schedule) */ \
  X(SR_VARIANT_NO_PPH, 24)             /* forward pph (halo rows, strips) -> the per-tap pp kernel */                   \
  X(SR_VARIANT_WG_NO_PARTIAL, 28)      /* wgrad pp with partial tiles and the kernel-row wgrad -> the 128x128 tile kernel */ \
  X(SR_VARIANT_NO_TAIL, 29)            /* HR tail convs (Cout <= 16, NCHW store): tail / W-256 halo kernel -> the tile kernel */ \
  X(SR_VARIANT_REDUCE_PLAIN, 33)       /* narrow-Cin slab reduce (block per channel) -> the one-thread-per-weight reduce */ \
  X(SR_VARIANT_NO_BAND, 34)            /* band kernel (whole rows, strips, slices) -> the tile kernel */                \
  X(SR_VARIANT_BAND_64, 35)            /* band kernel on 64 blocks: long bands that wrap the ring and cross images */   \
  X(SR_VARIANT_BAND_256, 36)           /* automatic; the band tests' name for the default 256-block grid */             \
  X(SR_VARIANT_BAND_CS_ROWS, 37)       /* band channel sums per row -> not reduced over the band */                     \
  X(SR_VARIANT_PPH_NO_PS, 50)          /* pixel-shuffled input: pph -> the pp kernel */                                 \
  X(SR_VARIANT_LIN_WIDE_BIG, 55)       /* linears with 192 < K <= 576: 64-token lin kernel -> the 256x256 pp kernel */  \
  X(SR_VARIANT_FOUR_PHASE, 59)         /* two-interval pph forward and wgrad pp -> their 4-phase forms */               \
  X(SR_VARIANT_PPH_P2_1, 61)           /* pph two-interval schedule without the B prefetch two K-steps ahead */         \
  X(SR_VARIANT_RING_WIDE_ALL, 62)      /* every bf16 3x3 wgrad with Cout > 64 -> the ring kernel over 64-co tiles */    \
  X(SR_VARIANT_NO_LINEAR_WGRAD, 63)    /* 1x1 wgrad: linear_wgrad_kernel -> the pp kernel */                            \
  X(SR_VARIANT_NO_LINEAR_WK, 64)       /* linears: linear_wk_kernel -> the lin kernel */                                \
  X(SR_VARIANT_RING_NO_PS, 67)         /* pixel-shuffled dy: ring wgrad over 64-co tiles -> pp / tile kernels */        \
  X(SR_VARIANT_HALO_NO_PS, 68)         /* pixel-shuffled input: halo kernel -> the tile kernel */                       \
  X(SR_VARIANT_NO_BAND_STRIP, 76)      /* band kernel over 128-px column strips -> the tile kernel */                   \
  X(SR_VARIANT_NO_PPH_STRIP, 77)       /* pph over 64-px column strips -> the pp kernel */                              \
  X(SR_VARIANT_NO_ROW3, 78)            /* kernel-row wgrad -> the pp kernel */                                          \
  X(SR_VARIANT_NO_BIG_PARTIAL, 79)     /* 128 < Cout < 256 from Cin >= 128: pph with a partial tile -> the halo kernel */ \
  X(SR_VARIANT_PPH_ONE_TILE, 80)       /* persistent multi-tile pph -> its one-tile form */
enum sr_conv_variant {
#define SR_VARIANT_ENUM(name, value) name = value,
  SR_CONV_VARIANTS(SR_VARIANT_ENUM)
#undef SR_VARIANT_ENUM
};
int sr_conv3x3_set_variant(int variant);
int sr_conv3x3_get_variant(void); /* the current kernel-variant switch */
/* Diagnostics (not part of the reference interface): per-block clock stamps of the row-band
 * forward kernel into a device buffer of 16 uint64 per block; NULL turns them off. */
int sr_conv3x3_set_stamps(void* buf);

/* Weight gradient: dw[co][ci][ky][kx] = scale * sum_pixels dy[p][co'] * x[p + tap][ci]
 * (param layout, fp32, co = perm(co') undoing out_ps), db[co] = scale * sum_p dy[p][co'].
 * dy is read in GEMM column order (gathered when out_ps > 0).  Needs a workspace of
 * sr_conv3x3_wgrad_workspace(d) bytes (split-K fp32 partial slabs, deterministic). */
typedef struct sr_conv3x3_wgrad_desc {
  int dtype;
  int N, H, W;
  int Cin, Cin_real, ldx, xcoff;
  int Cout, Cout_real, ldy, ycoff, out_ps;
  float scale;
  int in_up;  /* x read through nearest-neighbour upsampling by in_up (0/1 = none) */
  int ksize;  /* 3 (0 = 3) or 1 */
  int accumulate;  /* 1: dw += result, db += result (gradient accumulation in place, e.g. into
                      a flat .grad buffer); 0: overwrite */
} sr_conv3x3_wgrad_desc;

size_t sr_conv3x3_wgrad_workspace(const sr_conv3x3_wgrad_desc* d);
/* co_map[co] / ci_map[ci] (optional, device int arrays over the real param rows / cols) give
 * the GEMM column / input channel of each parameter row / column (padded head layouts). */
int sr_conv3x3_wgrad(const sr_conv3x3_wgrad_desc* d, const void* dy, const void* x,
                     void* workspace, size_t ws_bytes, float* dw, float* db, const int* co_map,
                     const int* ci_map, void* stream);
/* accumulate bit 1 of the descriptor: sr_conv3x3_wgrad writes only the split-K slab into the
 * workspace; sr_conv3x3_wgrad_reduce (same descriptor and workspace, e.g. on another stream)
 * then reduces it into dw / db (bit 0 of accumulate as for sr_conv3x3_wgrad). */
int sr_conv3x3_wgrad_reduce(const sr_conv3x3_wgrad_desc* d, void* workspace, size_t ws_bytes, float* dw, float* db,
                            const int* co_map, const int* ci_map, void* stream);

/* Two weight gradients of ONE geometry in one split-K launch and one reduce launch (the two convs of a
 * residual block): the descriptor gives the shared geometry, dtype and accumulate bit 0 (its scale is
 * unused), each item its operands, outputs and scale; both db are non-NULL or both NULL.  Each result is
 * deterministic and independent of the other item.
 * sr_conv3x3_wgrad_pair_ok: 1 exactly where the paired form runs (bf16 3x3 on the kernel-row wgrad, no
 * pixel shuffle, no maps; knob SR_WG_PAIR=0: never), else the caller makes two sr_conv3x3_wgrad calls.
 * sr_conv3x3_wgrad_pair_plan: the split plan (host-only query): splits per item, pixels per split and the
 * blocks of the launch with bias gradients. */
typedef struct sr_conv3x3_wgrad_item {
  const void* dy;
  const void* x;
  float* dw;
  float* db;
  float scale;
} sr_conv3x3_wgrad_item;
int sr_conv3x3_wgrad_pair_ok(const sr_conv3x3_wgrad_desc* d);
size_t sr_conv3x3_wgrad_pair_workspace(const sr_conv3x3_wgrad_desc* d);
int sr_conv3x3_wgrad_pair_plan(const sr_conv3x3_wgrad_desc* d, int* splits, int* kper, int* blocks);
int sr_conv3x3_wgrad_pair(const sr_conv3x3_wgrad_desc* d, const sr_conv3x3_wgrad_item* items, void* workspace,
                          size_t ws_bytes, void* stream);

/* Weight preparation from the nn.Conv2d parameter w[Cout_real][Cin_real][3][3] (fp32):
 *   wf[n][tap*Cin + ci]       forward GEMM rows (n = GEMM column, permuted by out_ps)
 *   wd[ci][tap'*Cout + n]     dgrad GEMM rows (spatially flipped, transposed)
 *   bias_g[n]                 bias in GEMM column order (zero for padded columns)
 * Any of wf / wd / bias_g may be NULL. */
int sr_conv3x3_prep(int dtype, const float* w, const float* bias, int Cout_real, int Cin_real,
                    int Cout, int Cin, int out_ps, void* wf, void* wd, float* bias_g,
                    void* stream);
/* One conv / linear weight of a batched GEMM-image preparation (same meaning as the arguments
 * of sr_conv_prep_mapped; ksize 1, 3, 5, 7 or 9). */
typedef struct {
  const float* w;
  const float* bias;
  int Cout_real, Cin_real, Cout, Cin, out_ps, ksize;
  const int* row_map;
  const int* col_map;
  void* wf;
  void* wd;
  float* bias_g;
} sr_prep_item;
/* Blocks (32 x 32 GEMM-row x channel tiles) item needs (host helper for building block_start). */
int sr_conv_prep_blocks(const sr_prep_item* item);
/* sr_conv_prep_mapped for n items in ONE launch: items and block_start (n + 1 prefix sums of
 * sr_conv_prep_blocks, block_start[n] = total_blocks) in device memory, all items of dtype.
 * Replaces the per-parameter re-preparation after every optimizer step. */
int sr_conv_prep_batch(int dtype, const sr_prep_item* items, const int* block_start, int n, int total_blocks,
                       void* stream);
/* General form: ksize 1 or 3, or 5 / 7 / 9 for the k x k convs of sr_convk_fwd (taps = ksize^2,
 * w[Cout_real][Cin_real][ksize][ksize], tap = ky*ksize + kx); row_map[n] (n < Cout) = parameter row of GEMM column n or -1
 * (zero row), col_map[k] (k < Cin) = parameter column of GEMM input channel k or -1; NULL maps
 * = identity (+ out_ps permutation).  nn.Linear weights are [out][in] = 1x1 conv weights. */
int sr_conv_prep_mapped(int dtype, int ksize, const float* w, const float* bias, int Cout_real,
                        int Cin_real, int Cout, int Cin, int out_ps, const int* row_map,
                        const int* col_map, void* wf, void* wd, float* bias_g, void* stream);

/* ---------------------------------------------------------------------------------
 * k x k convolution for narrow channel counts (csrc/convk.hip): stride 1, zero padding k / 2,
 * dilation 1, groups 1, odd k in {3, 5, 7, 9}, dense NHWC maps [N][H][W][C] of `dtype` with the
 * padded channel counts Cin, Cout (multiples of 8, <= 64; padded channels of x are zero), any
 * N, H, W >= 1.  SRCNN's 9x9 / 5x5 layers (nn.Conv2d(c, c', k, 1, k // 2)).  Anything outside
 * this envelope returns SR_EINVAL before any launch.
 *
 * Forward:  y = alpha * act(conv(x, w) + bias), act SR_ACT_NONE / SR_ACT_RELU; channels
 *   Cout_real .. Cout - 1 of y are stored as zeros.  w: [Cout][k*k*Cin] GEMM rows, K index =
 *   tap*Cin + ci (tap = ky*k + kx): the wf image of sr_conv_prep_mapped with ksize = k; bias:
 *   its bias_g, or NULL.  The input gradient is the same call on the wd image (Cin and Cout
 *   swapped, no bias), after sr_act_backward for a ReLU layer.
 * Weight gradient:  dw[co][ci][ky][kx] = scale * sum_p dy[p][co] * x[p + tap][ci], db[co] = scale *
 *   sum_p dy[p][co] (fp32, nn.Conv2d parameter layout over the real channels; db may be NULL), from
 *   fp32 partial slabs in a workspace of sr_convk_wgrad_workspace(d) bytes reduced in a fixed order
 *   (deterministic, no atomics).  accumulate bit 0: dw += / db += in place (sr_conv3x3_wgrad's
 *   convention).
 * ------------------------------------------------------------------------------- */
typedef struct sr_convk_desc {
  int dtype;
  int N, H, W;
  int k;
  int Cin, Cin_real;
  int Cout, Cout_real;
  int act;         /* forward */
  float alpha;     /* forward */
  float scale;     /* weight gradient */
  int accumulate;  /* weight gradient */
} sr_convk_desc;
int sr_convk_fwd(const sr_convk_desc* d, const void* x, const void* w, const float* bias, void* y, void* stream);
size_t sr_convk_wgrad_workspace(const sr_convk_desc* d);
int sr_convk_wgrad(const sr_convk_desc* d, const void* dy, const void* x, void* workspace, size_t ws_bytes, float* dw,
                   float* db, void* stream);
/* Bicubic upsampling by an integer scale s >= 1 with torch's align_corners=True semantics (source
 * coordinate o*(in-1)/(out-1), A = -0.75, clamped taps, fp32 arithmetic), layout change fused:
 * fp32 NCHW [N,C,H,W] -> NHWC dtype [N,H*s,W*s,Cp] (channels >= C zero). */
int sr_bicubic_up(int dtype, const float* x, int N, int C, int H, int W, int s, int Cp, void* y, void* stream);
/* Bicubic upsampling by an integer scale s >= 1 with torch's align_corners=False semantics (source
 * coordinate (o + 0.5) / s - 0.5, not clamped; A = -0.75, clamped taps, fp32 arithmetic): fp32 NCHW
 * [N,C,H,W] -> channels [c0, c0 + C) of the fp32 NCHW tensor y [N,Cy,H*s,W*s]; the other channels of y
 * are not touched (a fused torch.cat).  SR_EINVAL unless 0 <= c0 and c0 + C <= Cy. */
int sr_bicubic_up_hp(const float* x, int N, int C, int H, int W, int s, float* y, int Cy, int c0, void* stream);

/* ---------------------------------------------------------------------------------
 * Validation metrics (csrc/metrics.hip): PSNR / SSIM inputs of metrics/psnr_ssim.py computed on the
 * device.  sr, gt: fp32 NCHW [N,C,H,W] in nominal [-1, 1].  Both are quantised to ubyte as
 * minusone_one_tensor_to_ubyte_numpy does (clamp, (t + 1) / 2, * 255 in fp32, round half to even,
 * clip; bit-identical to the host), `crop` pixels are dropped on each edge, and per (n, c):
 *   sse[n*C + c]   the exact integer sum of squared ubyte differences over the crop
 *                  (PSNR = 10 log10(255^2 n / sse) on the host);
 *   ssim[n*C + c]  the mean of the 11-tap Gaussian (sigma 1.5) valid-mode SSIM map in float64
 *                  (C1 = (0.01*255)^2, C2 = (0.03*255)^2); NaN when the crop is smaller than 11 x 11.
 * Per-tile partials go to a workspace of sr_val_metrics_workspace(...) bytes (8-byte aligned) and are
 * reduced in a fixed order: no atomics, two runs are bit-identical.  SR_EINVAL for null pointers,
 * non-positive sizes, crop < 0, 2 * crop >= min(H, W) or a workspace that is too small (the size
 * query then returns 0).
 * ------------------------------------------------------------------------------- */
size_t sr_val_metrics_workspace(int N, int C, int H, int W, int crop);
int sr_val_metrics(const float* sr, const float* gt, int N, int C, int H, int W, int crop, int64_t* sse, double* ssim,
                   void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * NIQE block moments (csrc/niqe.hip): the device form of metrics/niqe.py:niqe_plane + niqe_moments for P
 * planes (1 <= P <= 64) of x, fp32 NCHW [N,C,H,W] in nominal [-1, 1], in one call.  The host turns the
 * moments into scores (metrics/niqe.py:niqe_from_moments).
 *   plane_desc  host int [P][4]: image n, then channels c0, c1, c2.  c1 = c2 = -1: the plane is band c0 as
 *               it is; otherwise the BT.601 Y of the three, y_coef[0]*c0 + y_coef[1]*c1 + y_coef[2]*c2 +
 *               y_coef[3] on the [0, 1] pixels (y_coef: host double [4]; NULL allowed without such a plane).
 *   window      host double [49], the 7 x 7 window as scipy.ndimage.convolve takes it (row-major).
 * Pixels are quantised to ubyte like sr_val_metrics, `crop` pixels dropped on each edge, the Y rounded, and
 * the plane truncated (top-left) to Hb x Wb = whole 96 x 96 blocks, bh x bw of them: the host plane exactly.
 *   moments     device double [P][2][bh][bw][5][6]: per scale (96-blocks of the plane, 48-blocks of its
 *               antialiased half-size resample), block and map (the MSCN block, its products with its
 *               circular rolls by (0,1), (1,0), (1,1), (1,-1)): count and sum of squares of the negative
 *               elements, the same of the positive ones, sum |x|, sum x^2.
 *   planes_out  optional device fp32 [P][Hb][Wb], the planes; mscn_out: optional, the scale-1 MSCN maps.
 * Workspace of sr_niqe_moments_workspace(...) bytes (4-byte aligned; 0 = unsupported shape).  Fixed-order
 * reductions, no atomics: two calls give identical bytes.  SR_EINVAL for null pointers, non-positive sizes,
 * crop < 0, H or W after the crop below 96, P outside 1..64, an image or channel index out of range, or a
 * workspace that is too small; SR_ETOOBIG when P * Hb * Wb exceeds 2^31 - 1.  Nothing is launched then.
 * ------------------------------------------------------------------------------- */
size_t sr_niqe_moments_workspace(int N, int C, int H, int W, int crop, int P);
int sr_niqe_moments(const float* x, int N, int C, int H, int W, int crop, int P, const int* plane_desc,
                    const double* y_coef, const double* window, double* moments, float* planes_out, float* mscn_out,
                    void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Layout / elementwise ops (HBM-bound).
 * ------------------------------------------------------------------------------- */
/* NCHW fp32 [N,C,H,W] -> NHWC dtype [N,H,W,Cp] (channels >= C zero):
 *   y = (x - shift[c]) * scale[c]   (shift/scale may be NULL -> 0 / 1). */
int sr_nchw_to_nhwc(int dtype, const float* x, int N, int C, int H, int W, int Cp,
                    const float* shift, const float* scale, void* y, void* stream);
/* NHWC dtype [N,H,W,ld] (channel offset coff) -> NCHW fp32 [N,C,H,W], y = x*scale[c]+shift[c]. */
int sr_nhwc_to_nchw(int dtype, const void* x, int N, int H, int W, int ld, int coff, int C,
                    const float* scale, const float* shift, float* y, void* stream);
/* Pixel shuffle (r > 0) / unshuffle (r < 0) on NCHW tensors of dtype, bit-exact index map
 * out[n, c, h*r+i, w*r+j] = in[n, c*r*r + i*r + j, h, w]; C/H/W are of the INPUT. */
int sr_pixel_shuffle_nchw(int dtype, const void* x, int N, int C, int H, int W, int r, void* y,
                          void* stream);
/* L1 loss partial sums + gradient: loss = weight * mean|pred - gt| (reduction 'mean') or
 * weight * sum (reduction 'sum'); grad = weight * sign(pred - gt) / norm.  Writes the loss to
 * *loss (fp32 device scalar) and the gradient to grad (may be NULL).  fp32 tensors. */
int sr_l1_loss(const float* pred, const float* gt, int64_t n, float weight, int mean,
               float* loss, float* grad, void* workspace, size_t ws_bytes, void* stream);
size_t sr_l1_loss_workspace(int64_t n);
/* Pixel-loss family (csrc/loss.hip; basicsr/losses/basic_loss.py:12-114 with weight_reduce_loss of
 * loss_util.py:26-55) fused with its gradient.  Per element d = pred - target:
 *   SR_LOSS_L1 |d|, SR_LOSS_MSE d^2, SR_LOSS_CHARBONNIER sqrt(d^2 + eps).
 * pred: NCHW-contiguous [N,C,H,W] of pred_dtype (SR_F32 / SR_BF16); target: the same shape, SR_F32 or
 * pred's dtype; weight: NULL (weight_channels 0) or an fp32 map [N,weight_channels,H,W] with 1 (broadcast
 * over the channels) or C channels.  Pointers need only element alignment; 16-byte aligned ones are
 * accessed with 16-byte vectors, with the same result bits.
 *   SR_REDUCE_SUM   *loss = loss_weight * sum(w * phi)
 *   SR_REDUCE_MEAN  the same over n = N*C*H*W without a weight, over sum(w) with a C-channel weight and
 *                   over C * sum(w) with a one-channel weight (computed on the device)
 *   SR_REDUCE_NONE  out[i] = loss_weight * w * phi in pred's dtype (loss is not written)
 * grad (may be NULL), pred's dtype: loss_weight * w * phi'(d) / denom, denom as above (1 for sum and none:
 * for 'none' the caller multiplies by the upstream gradient map).  phi' = sign(d) with sign(0) = 0, 2d,
 * d / sqrt(d^2 + eps).  loss: fp32 device scalar.  workspace: sr_pixel_loss_workspace(n) bytes, 8-byte
 * aligned.  Sums have a fixed order (no atomics): two runs are bit-identical; nothing synchronises or
 * allocates, so the call can be captured in a HIP graph. */
enum sr_loss_kind { SR_LOSS_L1 = 0, SR_LOSS_MSE = 1, SR_LOSS_CHARBONNIER = 2 };
enum sr_loss_reduction { SR_REDUCE_NONE = 0, SR_REDUCE_MEAN = 1, SR_REDUCE_SUM = 2 };
int sr_pixel_loss(int kind, int reduction, int pred_dtype, int target_dtype, const void* pred, const void* target,
                  const float* weight, int weight_channels, int N, int C, int H, int W, float loss_weight, float eps,
                  float* loss, void* out, void* grad, void* workspace, size_t ws_bytes, void* stream);
size_t sr_pixel_loss_workspace(int64_t n);
/* LDL artifact map and the ldl_opt term (csrc/ldl.hip; basicsr/losses/loss_util.py:99-145,
 * basicsr/models/realesrgan_model.py:211-226).  out / gt / ema: NCHW-contiguous [N,C,H,W]; out of
 * out_dtype (SR_F32 / SR_BF16), gt and ema SR_F32 or out's dtype.  Per image n and pixel p: r = sum_c |gt - out|,
 * e = sum_c |gt - ema|, mu and L the mean and the unbiased variance of the 7x7 window of the reflect-padded r,
 * V_n the unbiased variance of r over the image, P_n = V_n^(1/5), m = (r >= e):  w = P_n L m.
 *
 * sr_ldl_map_fwd writes what the backward keeps -- planes: fp32 [4,N,H,W] = r, mu, m L, m; stats: fp32 [N,8] =
 * mean of r, V, P, S = sum_p m L r, Q = (1/5) V^(-4/5) 2 / (H W - 1) (0 when V == 0: the dP/dV term of a constant
 * residual map is defined as 0), T, 0, 0 -- and
 *   l1 == 0: w, fp32 [N,1,H,W] (required);
 *   l1 != 0: *loss = k sum_n P_n S_n, the L1Loss of (w out, w gt) with k = loss_weight / (N C H W) for
 *            SR_REDUCE_MEAN and loss_weight for SR_REDUCE_SUM; T = k S; w is written too when not NULL.
 * sr_ldl_map_bwd writes d out (out's dtype, rounded once from fp32, every element once) through the whole map,
 * the window variances and V_n included (the reference does not detach w):
 *   dW != NULL: the gradient of sum_p dW w (dW fp32 [N,1,H,W]); needs the workspace;
 *   dW == NULL: the gradient of the fused L1 term (reduction / loss_weight as in the forward call).
 * upstream (may be NULL = 1): an fp32 device scalar every element is multiplied by before the rounding.
 * ksize must be 7, H and W >= 4, N <= 65535, N C H W < 2^31; pointers element-aligned; workspace:
 * sr_ldl_map_workspace bytes, 4-byte aligned.  Anything else is SR_EINVAL before any launch.  Fixed summation
 * orders, no atomics: two runs give the same bits; nothing allocates or synchronises. */
size_t sr_ldl_map_workspace(int N, int H, int W);
int sr_ldl_map_fwd(int out_dtype, int gt_dtype, int ema_dtype, const void* out, const void* gt, const void* ema, int N,
                   int C, int H, int W, int ksize, int l1, int reduction, float loss_weight, float* w, float* planes,
                   float* stats, float* loss, void* workspace, size_t ws_bytes, void* stream);
int sr_ldl_map_bwd(int out_dtype, int gt_dtype, const void* out, const void* gt, const float* planes, const float* stats,
                   const float* dW, const float* upstream, int N, int C, int H, int W, int ksize, int reduction,
                   float loss_weight, void* dout, void* workspace, size_t ws_bytes, void* stream);
/* RegisteredLoss (csrc/regloss.hip; basicsr/losses/align_loss.py:161-256): the smallest, per image,
 * of the L1 / MSE losses between every sub-pixel shift of pred and the target, fused with its gradient.
 * pred / target: NCHW-contiguous [B,C,H,W]; pred of pred_dtype (SR_F32 / SR_BF16), target SR_F32 or pred's dtype.
 * taps: fp32 [S,K] on the device, K = 2r + 1 odd, one row of 1-D taps per shift value; the same table serves both
 * axes and the kernels take it as data.  Shift s = sy * S + sx (the y index is the slow one) is the
 * cross-correlation with zero padding
 *   shifted[b,s,c,h,w] = sum_j sum_i taps[sy,j] taps[sx,i] pred[b,c,h+j-r,w+i-r],
 * scored on the crop [r,H-r) x [r,W-r) only: loss[b,s] = mean over c and the crop of phi(shifted - target),
 * phi = |d| (SR_LOSS_L1) or d^2 (SR_LOSS_MSE).  idx[b] (int32 [B]) = argmin_s loss[b,s] of the fp32 values, the
 * first index on ties, a NaN entry before any number (torch.argmin).  table (may be NULL): fp32 [B,S*S] = loss[b,s].
 *   SR_REDUCE_MEAN  *loss = loss_weight * mean_b loss[b,idx[b]]
 *   SR_REDUCE_SUM   *loss = loss_weight * sum_b
 *   SR_REDUCE_NONE  loss[b] = loss_weight * loss[b,idx[b]]   (fp32 [B])
 * grad (may be NULL), pred's dtype, every element written once: the gradient through the selected shift alone,
 *   d pred[b,c,p,q] = sum_j sum_i taps[sy*,j] taps[sx*,i] g[b,c,p-j+r,q-i+r],  g = k phi'(d) / n on the crop, 0 on the
 * border strips (whose pixels of pred do receive gradient), n = C (H-2r)(W-2r), phi' = sign(d) with sign(0) = 0, or
 * 2d, k = loss_weight / B (mean) or loss_weight (sum; and none, where the caller multiplies image b by its upstream
 * element).  No shifted image is stored: the workspace (sr_registered_loss_workspace bytes, 8-byte aligned) holds
 * per-tile partial sums only, nothing the call touches grows with S*S*H*W.  S 1 to 9, K odd 7 to 13, H and W >= K,
 * B*C*H*W < 2^31, pointers element-aligned; anything else is SR_EINVAL with a message before any launch.  Sums have
 * a fixed order (double past the tile, no atomics): two runs give the same bits; nothing synchronises or allocates
 * and idx is read back on the device, so the call can be captured in a HIP graph. */
size_t sr_registered_loss_workspace(int B, int C, int H, int W, int S);
int sr_registered_loss(int kind, int reduction, int pred_dtype, int target_dtype, const void* pred, const void* target,
                       const float* taps, int S, int K, int B, int C, int H, int W, float loss_weight, float* loss,
                       int* idx, float* table, void* grad, void* workspace, size_t ws_bytes, void* stream);
/* ---------------------------------------------------------------------------------
 * Perceptual / style loss kernels (csrc/perceptual.hip; PerceptualLoss of basicsr/losses/basic_loss.py:147-253
 * over the VGGFeatureExtractor of basicsr/archs/vgg_arch.py).  Feature maps are dense NHWC of dtype
 * (SR_F32 / SR_BF16), 16-byte aligned, C a multiple of 8.  Fixed summation orders, no atomics: two calls
 * give identical bits; nothing allocates or synchronises.  SR_EINVAL for null pointers, non-positive sizes,
 * an unsupported dtype / stride / channel count or a misaligned pointer, SR_ETOOBIG when a tensor reaches
 * 2^31 bytes; nothing is launched then.
 *
 * sr_maxpool2_fwd: nn.MaxPool2d(kernel_size=2, stride) with stride 1 or 2, no padding, floor mode:
 *   y [N, Ho, Wo, C], Ho = (H - 2) / stride + 1.  The first maximum in row-major window order wins and a
 *   NaN propagates, as torch.
 * sr_maxpool2_bwd: dx [N, H, W, C] of the same, all of it written: dy goes to the element the forward chose
 *   (recomputed from x with the forward's rule), overlapping stride-1 windows sum (fp32, fixed order), a
 *   row / column the floor drops is zero.
 * ------------------------------------------------------------------------------- */
int sr_maxpool2_fwd(int dtype, const void* x, int N, int H, int W, int C, int stride, void* y, void* stream);
int sr_maxpool2_bwd(int dtype, const void* x, const void* dy, int N, int H, int W, int C, int stride, void* dx,
                    void* stream);
/* Gram matrix per image: G[n] = F[n]^T F[n] * scale, F [N, HW, C] of dtype (C <= 512), G fp32 [N, C, C]
 * (basic_loss.py:240-253 with scale = 1 / (C * H * W)); MFMA bf16 16x16x32 / f32 16x16x4 as the convs.
 * K = HW is split over sr_gram_splits(HW) blocks per image of sr_gram_kblock() * m rows each (m the smallest
 * integer that keeps the splits at 64 or fewer; the last block takes the rest); with more than one split
 * the fp32 partials go to ws (sr_gram_workspace bytes, 4-byte aligned; 0 and ws may be NULL with one
 * split) and are summed in a fixed order. */
int sr_gram_kblock(void);
int sr_gram_splits(int HW);
size_t sr_gram_workspace(int N, int HW, int C);
int sr_gram_fwd(int dtype, const void* F, int N, int HW, int C, float scale, float* G, void* ws, size_t ws_bytes,
                void* stream);
/* dF[n] = alpha * F[n] (dG[n] + dG[n]^T) + beta * res[n] in F's dtype: the gradient of sr_gram_fwd (alpha
 * carries its scale) plus, optionally, another gradient of the same feature map in the same store (res:
 * F's shape and dtype, may be NULL).  dG fp32 [N, C, C], symmetrised while it is staged; products and sums
 * in fp32 (f32 MFMA for both dtypes). */
int sr_gram_bwd(int dtype, const void* F, const float* dG, const void* res, int N, int HW, int C, float alpha,
                float beta, void* dF, void* stream);
/* ---------------------------------------------------------------------------------
 * GAN training (csrc/gan.hip, csrc/loss.hip): the kernels of the VGGStyleDiscriminator
 * (basicsr/archs/discriminator_arch.py) and the GANLoss (basicsr/losses/gan_loss.py).  Feature maps are dense
 * NHWC of dtype (SR_F32 / SR_BF16), 16-byte aligned, channels padded to multiples of 8.  Fixed summation
 * orders, no atomics; nothing allocates or synchronises; SR_EINVAL / SR_ETOOBIG before any launch.
 *
 * GAN loss of a prediction of n elements: *loss = w * mean(l(x)), grad (may be NULL, pred's dtype) =
 * w * l'(x) / n, with w = loss_weight for a generator and 1 when is_disc.  vanilla: BCE with logits against
 * target_val; lsgan: (x - target_val)^2; wgan: -x (real) / x (fake); wgan_softplus: softplus(-x) / softplus(x);
 * hinge: relu(1 - x) / relu(1 + x) when is_disc, -x for a generator.  workspace: sr_gan_loss_workspace bytes,
 * 4-byte aligned; sr_gan_loss_block: the elements one block of the streaming pass covers per trip.
 * ------------------------------------------------------------------------------- */
enum sr_gan_kind { SR_GAN_VANILLA = 0, SR_GAN_LSGAN = 1, SR_GAN_WGAN = 2, SR_GAN_WGAN_SOFTPLUS = 3, SR_GAN_HINGE = 4 };
size_t sr_gan_loss_workspace(int64_t n);
int sr_gan_loss_block(int pred_dtype);
int sr_gan_loss(int kind, int pred_dtype, const void* pred, int64_t n, float target_val, int target_is_real, int is_disc,
                float loss_weight, float* loss, void* grad, void* workspace, size_t ws_bytes, void* stream);
/* nn.Conv2d(cin, cout, 4, 2, 1, bias=False) on x [N, H, W, Cin] -> y [N, H/2, W/2, Cout]; H, W even, Cin and
 * Cout multiples of 8 from 8 to 512.  An implicit GEMM on MFMA bf16 16x16x32 / f32 16x16x4 with fp32 sums.
 * prep: the GEMM images of the fp32 parameter w [cout_real][cin_real][4][4] in dtype: wf [Cout][16 * Cin] for
 *   the forward, wd [4][Cin][4 * Cout] for the dgrad (one image per (row, column) parity of the input pixel);
 *   padded channels are zeros.
 * dgrad: dx [N, H, W, Cin] from dy [N, H/2, W/2, Cout]; every dx element is written once (a gather over the
 *   four parity classes, 4 taps each).
 * wgrad: dw [cout_real][cin_real][4][4] fp32 = (or += with accumulate) scale * the weight gradient; split K
 *   over sr_conv4s2_wgrad_splits blocks of output pixels, fp32 partials in ws (sr_conv4s2_wgrad_workspace
 *   bytes), summed in split order. */
int sr_conv4s2_prep(int dtype, const float* w, int cout_real, int cin_real, int Cout, int Cin, void* wf, void* wd,
                    void* stream);
int sr_conv4s2_fwd(int dtype, const void* x, const void* wf, int N, int H, int W, int Cin, int Cout, void* y,
                   void* stream);
int sr_conv4s2_dgrad(int dtype, const void* dy, const void* wd, int N, int H, int W, int Cin, int Cout, void* dx,
                     void* stream);
size_t sr_conv4s2_wgrad_workspace(int N, int H, int W, int Cin, int Cout);
int sr_conv4s2_wgrad_splits(int N, int H, int W, int Cin, int Cout);
int sr_conv4s2_wgrad(int dtype, const void* dy, const void* x, int N, int H, int W, int Cin, int cin_real, int Cout,
                     int cout_real, float scale, int accumulate, float* dw, void* ws, size_t ws_bytes, void* stream);
/* sr_conv4s2_fwd with an activation epilogue: y = act(conv), act SR_ACT_NONE (the bits of sr_conv4s2_fwd) or
 * SR_ACT_LRELU with slope.  The backward applies sr_act_backward to dy, then the dgrad / wgrad above. */
int sr_conv4s2_fwd_act(int dtype, const void* x, const void* wf, int N, int H, int W, int Cin, int Cout, int act,
                       float slope, void* y, void* stream);
/* Spectral normalisation of conv weights (torch.nn.utils.spectral_norm: one power iteration, fp32 throughout),
 * GROUPED: one call serves n <= SR_SN_MAX_PROBLEMS matrices M = w [R][K] (R = cout, K = cin kh kw, R K < 2^30), so the
 * launch count does not depend on n.  The table is read on the host and travels to the kernels in their argument
 * segment: nothing is uploaded and it need not outlive the call.
 * fwd, iterate != 0: t = M^T u, v = t / max(|t|, eps), s = M v, u = s / max(|s|, eps), sigma = u . s; u and v are
 *   updated in place and also copied to u_fwd / v_fwd (what this forward's backward reads); out = w / sigma.
 *   iterate == 0 (eval): u, v untouched, u_fwd / v_fwd their copies, sigma = u . (M v).
 * bwd: w = the normalised weight the forward wrote, g = dL/dW or NULL (the problem is skipped; with no g at all
 *   nothing is launched); out [R][K] (=, or += with accumulate) (g - <g, w> u_fwd v_fwd^T) / sigma.
 * Fixed summation orders, no atomics.  16-byte accesses where K % 4 == 0 and w, v_fwd, out, g are 16-byte
 * aligned, scalar ones otherwise.  ws: sr_spectral_norm_workspace(problems, n) bytes, 16-byte aligned. */
#define SR_SN_MAX_PROBLEMS 16
typedef struct sr_sn_problem {
  const float* w;
  float* u;
  float* v;
  float* u_fwd;
  float* v_fwd;
  float* sigma;
  float* out;
  const float* g;
  int R, K;
} sr_sn_problem;
size_t sr_spectral_norm_workspace(const sr_sn_problem* problems, int n);
int sr_spectral_norm_fwd(const sr_sn_problem* problems, int n, int iterate, float eps, void* ws, size_t ws_bytes,
                         void* stream);
int sr_spectral_norm_bwd(const sr_sn_problem* problems, int n, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* Bilinear x2 upsampling (align_corners=False) of an NHWC map x [N, H, W, C] -> y [N, 2H, 2W, C], C a multiple of
 * 8, fp32 or bf16, 16-byte accesses (misaligned pointers are refused), fp32 arithmetic and one rounding on store.
 * Per axis out[2i] = .25 in[max(i-1, 0)] + .75 in[i], out[2i+1] = .75 in[i] + .25 in[min(i+1, n-1)].
 * bwd: dx [N, H, W, C] from dy [N, 2H, 2W, C], the transpose as a gather (every dx element written once). */
int sr_bilinear_up2_fwd(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream);
int sr_bilinear_up2_bwd(int dtype, const void* dy, int N, int H, int W, int C, void* dx, void* stream);
/* BatchNorm2d over the M = N H W <= 2^24 rows of an NHWC map x [M][C] (C a multiple of 8 up to 1024), statistics and
 * affine parameters fp32.  act: SR_ACT_NONE or SR_ACT_LRELU (fused after the affine).
 * stats: save_mean, save_rstd = 1 / sqrt(biased variance + eps) by Welford updates per thread merged with
 *   (count, mean, M2) partials in a fixed order over sr_bn_blocks(M) blocks (no E[x^2] - E[x]^2); with
 *   running_mean / running_var (both or neither) also r = (1 - f) r + f * (mean | unbiased variance),
 *   f = momentum, or 1 / *nbt (the already incremented num_batches_tracked, int64 on the device) when
 *   momentum < 0.  M >= 2.  ws: sr_bn_workspace bytes.
 * apply: y = act(gamma * (x - mean) * rstd + beta); rstd_or_var is save_rstd, or with use_var the running
 *   variance (eval mode: rstd = 1 / sqrt(var + eps)).
 * bwd_reduce: dbeta = sum g, dgamma = sum g * xhat, g = dy * act'(gamma * xhat + beta) recomputed from x.
 * bwd_dx: dx = rstd * gamma * (g - dbeta / M - xhat * dgamma / M) when training, g * gamma * rstd otherwise. */
size_t sr_bn_workspace(int64_t M, int C);
int sr_bn_blocks(int64_t M);
int sr_bn_stats(int dtype, const void* x, int64_t M, int C, float eps, float momentum, const int64_t* nbt, float* save_mean,
                float* save_rstd, float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream);
int sr_bn_apply(int dtype, const void* x, int64_t M, int C, const float* mean, const float* rstd_or_var, int use_var,
                float eps, const float* gamma, const float* beta, int act, float slope, void* y, void* stream);
int sr_bn_bwd_reduce(int dtype, const void* x, const void* dy, int64_t M, int C, const float* mean,
                     const float* rstd_or_var, int use_var, float eps, const float* gamma, const float* beta, int act,
                     float slope, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
int sr_bn_bwd_dx(int dtype, const void* x, const void* dy, int64_t M, int C, const float* mean, const float* rstd_or_var,
                 int use_var, float eps, const float* gamma, const float* beta, int act, float slope,
                 const float* dgamma, const float* dbeta, int training, void* dx, void* stream);
/* Head linears on the fp32 nn.Linear parameters as they are: y fp32 [M][O] = act(x W^T + bias), x [M][K] of
 * dtype, W [O][K].  P > 1: x's feature index is NHWC ((h w) * C + c, C = K / P) while W's is the NCHW flatten
 * (c * P + (h w)); the kernels permute on the x side, so dw is in the parameter's order.  dgrad / wgrad take
 * dy fp32 [M][O] and, with a fused LeakyReLU, the forward's output y (NULL: no activation); dx in dtype;
 * dw / db = or += (accumulate), db may be NULL.  Sums in index order. */
int sr_fc_fwd(int dtype, const void* x, const float* w, const float* bias, int M, int K, int O, int P, int act, float slope,
              float* y, void* stream);
int sr_fc_dgrad(int dtype, const float* dy, const float* y, const float* w, int M, int K, int O, int P, float slope,
                void* dx, void* stream);
int sr_fc_wgrad(int dtype, const float* dy, const float* y, const void* x, int M, int K, int O, int P, float slope,
                int accumulate, float* dw, float* db, void* stream);
/* Activation backward: out = alpha * dy * (y > 0 ? 1 : neg), neg = 0 for SR_ACT_RELU, slope for
 * SR_ACT_LRELU, 1 for SR_ACT_NONE; y is the activation OUTPUT (same sign as its input). */
int sr_act_backward(int dtype, const void* dy, const void* y, int64_t n, int act, float slope, float alpha,
                    void* out, void* stream);
/* out[m][c] = x[m][c] * scale[m / HW] on a dense [M][C] map (C a multiple of 8 bf16 / 4 f32):
 * the per-sample DropPath factor (swinir_arch.py:14-40) on a residual-branch gradient. */
int sr_row_scale(int dtype, const void* x, int64_t M, int C, int HW, const float* scale, void* out, void* stream);
/* Fused Adam (torch.optim.Adam semantics, no amsgrad/weight decay) + EMA of a flat fp32
 * parameter vector: g is scaled by grad_scale (DDP 1/world_size averaging), p, exp_avg,
 * exp_avg_sq updated in place; if ema != NULL, ema = ema*decay + p*(1-decay) after the step
 * (basicsr/models/base_model.py:75-82).  bc1/bc2 = 1 - beta^step. */
int sr_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr,
                float beta1, float beta2, float eps, float bc1, float bc2, float ema_decay,
                float grad_scale, void* stream);
/* Graph-capturable form: hyper = device float[3] {step, lr, grad_scale}; the call first
 * increments hyper[0] on the device, then applies the update with bc = 1 - beta^step. */
int sr_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float* hyper,
                    float beta1, float beta2, float eps, float ema_decay, void* stream);

/* ---------------------------------------------------------------------------------
 * Block kernels of MSRResNet / RCAN / RRDBNet (csrc/blocks.hip).
 * ------------------------------------------------------------------------------------- */
/* y = base + bilinear_upsample(x, s) (align_corners=False), fp32 NCHW, x [N,C,H,W]
 * (MSRResNet skip, basicsr/archs/srresnet_arch.py:64-65). */
int sr_bilinear_up_add(const float* x, int N, int C, int H, int W, int s, const float* base, float* y,
                       void* stream);
/* out[n][c] = scale * sum_p a[n,p,c] (* b[n,p,c] if b) over the HW pixels of NHWC maps (channel
 * slices via ld/coff), deterministic; RCAN AdaptiveAvgPool2d(1) (rcan_arch.py:19) and its backward. */
size_t sr_channel_reduce_workspace(int N, int HW, int C);
int sr_channel_reduce(int dtype, const void* a, int lda, int acoff, const void* b, int ldb, int bcoff, int N,
                      int HW, int C, float scale, float* out, void* workspace, size_t ws_bytes, void* stream);
/* First pass of sr_channel_reduce only: parts[n][p][c] partial sums (dots) over pixel chunks,
 * P = sr_channel_partials_count(HW) chunks per image (the consumer sums them). */
int sr_channel_partials_count(int HW);
int sr_channel_partials(int dtype, const void* a, int lda, int acoff, const void* b, int ldb, int bcoff, int N,
                        int HW, int C, float* parts, void* stream);
/* RCAN squeeze MLP (the two 1x1 convs of rcan_arch.py:19-20): pool[n][c] = scale * sum_p
 * parts[n*P + p][c] (P = 1, scale = 1: parts is the pooled vector), h = relu(W1 pool + b1),
 * s = sigmoid(W2 h + b2); W1 [Cr][C], W2 [C][Cr]. */
int sr_ca_mlp_fwd(const float* parts, int P, float scale, const float* w1, const float* b1, const float* w2,
                  const float* b2, int N, int C, int Cr, float* pool, float* h, float* s, void* stream);
/* Its backward for the batch: ds[n][c] = scale * sum_p parts[n*P + p][c] = dL/ds -> dpool, dW1,
 * db1, dW2, db2 (db1/db2 may be NULL); accumulate = 1 adds the parameter gradients into
 * dw1/db1/dw2/db2 (the optimizer's gradient views) instead of storing them. */
int sr_ca_mlp_bwd(const float* parts, int P, float scale, const float* s, const float* h, const float* pool,
                  const float* w1, const float* w2, int N, int C, int Cr, float* dpool, float* dw1, float* db1,
                  float* dw2, float* db2, int accumulate, void* stream);
/* RCAB channel attention fused with its elementwise pass (rcan_arch.py:8-24, :44-46): every block
 * of the pass recomputes its image's squeeze MLP from the partial sums (fixed order, identical in
 * every block), so the MLP is not a dependent single-block launch.
 *   fwd: pool = scale*sum_p parts, h = relu(W1 pool + b1), s = sigmoid(W2 h + b2), y = x + alpha*u*s;
 *        pool / h / s are also stored (for the backward);
 *   bwd: ds = alpha*sum_p parts (parts of dy.u), dz2 = ds*s*(1-s), dz1 = relu'(h)*(W2^T dz2),
 *        du = alpha*dy*s + (W1^T dz1)/HW; dz2 [N][C] and dz1 [N][Cr] are stored for
 *   sr_ca_param_grad: dW2 = dz2^T h, dW1 = dz1^T pool, db2 = sum dz2, db1 = sum dz1 (accumulate = 1
 *        adds into the optimizer's gradient views; db1 / db2 may be NULL).
 * Dense NHWC [N, HW, C], C % 8 == 0, C <= 256, Cr <= 64; W1 [Cr][C], W2 [C][Cr]. */
int sr_ca_fwd_apply(int dtype, const float* parts, int P, float scale, const float* w1, const float* b1,
                    const float* w2, const float* b2, const void* x, const void* u, int N, int HW, int C, int Cr,
                    float alpha, void* y, float* pool, float* h, float* s, void* stream);
int sr_ca_bwd_apply(int dtype, const float* parts, int P, float alpha, const float* s, const float* h, const float* w1,
                    const float* w2, const void* dy, int N, int HW, int C, int Cr, void* du, float* dz2, float* dz1,
                    void* stream);
int sr_ca_param_grad(const float* dz2, const float* dz1, const float* h, const float* pool, int N, int C, int Cr,
                     float* dw1, float* db1, float* dw2, float* db2, int accumulate, void* stream);
/* out = beta*x + alpha*u*s[n,c] + gamma*t[n,c] on dense NHWC [N,HW,C] (x, t may be NULL):
 * RCAB tail x + rs*u*s and its backward rs*dout*s + dpool/HW. */
int sr_nc_affine(int dtype, const void* x, const void* u, const float* s, const float* t, int N, int HW, int C,
                 float beta, float alpha, float gamma, void* out, void* stream);
/* Strided activation backward over channel slices: out = alpha*dy*(y > 0 ? 1 : neg). */
int sr_act_backward_nhwc(int dtype, int64_t P, int C, const void* dy, int ldd, int dcoff, const void* y, int ldy,
                         int ycoff, void* out, int ldo, int ocoff, int act, float slope, float alpha,
                         void* stream);
/* Backward of nearest upsampling by s: out[n,y,x,c] (+)= sum of d over the s x s block
 * (rrdbnet_arch.py:116-117); out has H x W pixels, d has sH x sW. */
int sr_nearest_up_backward(int dtype, const void* d, int ldd, int N, int H, int W, int C, int s, void* out,
                           int ldo, int accumulate, void* stream);
/* The same times the activation derivative of the upsampled map (gate: its H x W LeakyReLU / ReLU output,
 * row stride ldg): out = sum * (gate > 0 ? 1 : slope) -- the conv_up1 / conv_up2 lrelu backward
 * (rrdbnet_arch.py:116-117) fused into the 2x2 sum; gate null = sr_nearest_up_backward. */
int sr_nearest_up_backward_gate(int dtype, const void* d, int ldd, int N, int H, int W, int C, int s,
                                const void* gate, int ldg, float slope, void* out, int ldo, int accumulate,
                                void* stream);
/* Strided channel-slice copy (RRDB dense-block buffers). */
int sr_copy_channels(int dtype, const void* src, int lds, int scoff, void* dst, int ldd, int dcoff, int64_t P,
                     int C, void* stream);

/* ---------------------------------------------------------------------------------
 * SwinIR token kernels (csrc/swin.hip).  Token maps are NHWC rows (= the reference's
 * [B, H*W, C] after PatchEmbed, swinir_arch.py:600-604).
 * ------------------------------------------------------------------------------------- */
/* nn.LayerNorm(C) over rows of [M][ld]: y = (x-mean)*rstd*gamma + beta (channels < C; columns
 * C..Cp-1 of y set to 0); saves per-row mean / rstd (fp32). */
int sr_layernorm_fwd(int dtype, const void* x, int ldx, const float* gamma, const float* beta, int64_t M,
                     int C, int Cp, float eps, void* y, int ldy, float* mean, float* rstd, void* stream);
size_t sr_layernorm_bwd_workspace(int64_t M, int C);
/* dx = LN backward (+ res if not NULL), dgamma / dbeta over all rows (deterministic);
 * accumulate bit 0 adds them to dgamma / dbeta (the optimizer's gradient views); bit 1 leaves
 * the dgamma / dbeta partial rows in the workspace for sr_layernorm_bwd_reduce (when
 * sr_layernorm_bwd_parts > 0), so that reduction can run on another stream. */
int sr_layernorm_bwd(int dtype, const void* dy, int lddy, const void* x, int ldx, const float* mean,
                     const float* rstd, const float* gamma, int64_t M, int C, int Cp, const void* res,
                     int ldr, void* dx, int lddx, float* dgamma, float* dbeta, void* workspace,
                     size_t ws_bytes, int accumulate, void* stream);
/* sr_layernorm_bwd that also writes dx_scaled[m] = dx[m] * row_scale[m / HW] (same layout as dx):
 * the SwinIR proj-branch gradient under stochastic depth (swinir_arch.py:14-40, 320) in the same
 * pass (bf16, Cp <= 256 path only). */
int sr_layernorm_bwd_scaled(int dtype, const void* dy, int lddy, const void* x, int ldx, const float* mean,
                            const float* rstd, const float* gamma, int64_t M, int C, int Cp, const void* res, int ldr,
                            void* dx, int lddx, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes,
                            int accumulate, const float* row_scale, int HW, void* dx_scaled, void* stream);
int sr_layernorm_bwd_parts(int dtype, int64_t M, int Cp, int ldx, int lddx, int lddy, int ldr);
int sr_layernorm_bwd_reduce(const float* workspace, int nparts, int C, float* dgamma, float* dbeta, int accumulate,
                            void* stream);
/* Shifted-window multi-head attention on [N*H*W][ldq] qkv rows laid out [3][nH][hdp]
 * (head_dim hd <= hdp, zero padded): cyclic shift by `shift`, ws x ws windows, scale,
 * relative-position bias table [(2ws-1)^2][nH], -100 shift mask; out rows [nH][hdp];
 * lse = per-query log-sum-exp (for the backward).  ws <= 8, hd <= 32. */
int sr_window_attn_fwd(int dtype, const void* qkv, int ldq, int N, int H, int W, int ws, int shift, int nH,
                       int hd, int hdp, float scale, const float* bias_table, void* out, int ldo, float* lse,
                       void* stream);
/* Fused attention half of a SwinTransformerBlock (basicsr/archs/swinir_arch.py:283-314 with
 * WindowAttention :144-175; round 4): x2 = x + row_scale[n] * proj(WindowAttention(qkv(LN1(x)))) in
 * one launch on bf16 token maps [N][H][W][Cp] (Cp <= 192), window 8, nH heads of dim <= 32 padded
 * to 32 (nH * 32 <= 192), cyclic shift `shift`.  wqkv / wproj are the GEMM images of the qkv
 * (rows [3][nH][32], Cp columns) and proj (Cp rows, nH * 32 columns) linears with their fp32
 * biases; bias_table [(2*8-1)^2][nH]; row_scale [N] (DropPath) or NULL.  Training: qkv != NULL
 * and ln_out / ln_mean / ln_rstd / attn_out / lse receive what sr_linear_ln_fwd and
 * sr_window_attn_fwd write (the backward reads them unchanged); inference: all NULL, only x2 is
 * written.  sr_swin_attn_fused_ok: 1 when a geometry is on this path. */
int sr_swin_attn_fused_ok(int dtype, int N, int H, int W, int ws, int nH, int hd, int hdp, int C, int Cp);
int sr_swin_attn_fused_fwd(const void* x, const float* ln_g, const float* ln_b, int C, float eps, const void* wqkv,
                           const float* bqkv, const float* bias_table, const void* wproj, const float* bproj,
                           const float* row_scale, int N, int H, int W, int shift, int nH, int Cp, float scale, void* x2,
                           void* ln_out, float* ln_mean, float* ln_rstd, void* qkv, void* attn_out, float* lse,
                           void* stream);
/* Fused MLP half of a SwinTransformerBlock (swinir_arch.py:322-323, Mlp :43-60; round 4):
 * out = x + row_scale[n] * fc2(GELU(fc1(LN2(x)))) on bf16 token rows [N * HW][Cp] (Cp <= 192,
 * hidden Hp <= 368, multiples of 8): w1 / w2 the fc1 [Hp][Cp] / fc2 [Cp][Hp] GEMM images with fp32
 * biases.  Training: z != NULL, and ln_out / ln_mean / ln_rstd / z (pre-activation) / h
 * (activation) receive what sr_linear_ln_fwd writes for norm2 -> fc1 (the backward reads them);
 * inference: all NULL. */
int sr_swin_mlp_fused_ok(int dtype, int C, int Cp, int Hp);
int sr_swin_mlp_fused_fwd(const void* x, const float* ln_g, const float* ln_b, int C, float eps, const void* w1,
                          const float* b1, const void* w2, const float* b2, const float* row_scale, int N, int HW,
                          int Cp, int Hp, void* out, void* ln_out, float* ln_mean, float* ln_rstd, void* z, void* h,
                          void* stream);
size_t sr_window_attn_bwd_workspace(int N, int H, int W, int ws, int nH);
int sr_window_attn_bwd(int dtype, const void* qkv, int ldq, const void* out, const void* dout, int ldo,
                       const float* lse, int N, int H, int W, int ws, int shift, int nH, int hd, int hdp,
                       float scale, const float* bias_table, void* dqkv, float* dbias_table, void* workspace,
                       size_t ws_bytes, int accumulate, void* stream);
/* accumulate bit 1 of sr_window_attn_bwd: the relative-bias gradient partial rows (count:
 * sr_window_attn_bwd_parts) stay in the workspace for sr_window_attn_dbias_reduce.  A negative
 * count -P means P per-lane slot rows (the two-wave MFMA backward: 64 lanes x 28 pre-summed bins
 * per row, folded into the (2ws-1)^2 bins by the reduce); pass it through unchanged. */
int sr_window_attn_bwd_parts(int dtype, int N, int H, int W, int ws, int nH, int hd, int hdp, int ldq, int ldo);
int sr_window_attn_dbias_reduce(const float* workspace, int parts, int nH, int ws, float* dbias_table, int accumulate,
                                void* stream);

/* SwinIR absolute position embedding (ape=True, swinir_arch.py:789-791, :879-880) on dense token rows
 * [N][P][Cp]: y = x + pos[p][c] for c < C (pos fp32 [P][C]); its gradient dpos[p][c] (+)= sum_n dy. */
int sr_add_pos_embed(int dtype, const void* x, int N, int P, int C, int Cp, const float* pos, void* y, void* stream);
int sr_pos_embed_grad(int dtype, const void* dy, int N, int P, int C, int Cp, float* dpos, int accumulate,
                      void* stream);

/* ---------------------------------------------------------------------------------
 * basicsr/ops native extensions (replacements of deform_conv_ext, fused_act_ext,
 * upfirdn2d_ext).
 * ------------------------------------------------------------------------------------- */
/* Deformable convolution geometry (csrc/dcn.hip: entry points and geometry; kernels in csrc/dcn_cols.hip,
 * dcn_fwd_fused.hip and dcn_bwd_win.hip).  x is NHWC [N][H][W][Cp] (dtype);
 * offset [N][DG*2*kh*kw][Ho][Wo] and mask [N][DG*kh*kw][Ho][Wo] are the reference's NCHW
 * fp32 tensors (channel 2*tap = dy, 2*tap+1 = dx, per deformable group).  Columns are
 * pixel-major rows [N*Ho*Wo][groups][kh*kw][cgp] (cgp = padded C/groups), the operand of
 * the 1x1 GEMM (sr_conv3x3_fwd with ksize 1). */
typedef struct sr_dcn_desc {
  int dtype;
  int N, C, H, W, Cp, Ho, Wo;
  int kh, kw, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
  int groups, deformable_groups, cgp;
} sr_dcn_desc;
/* columns = mask * bilinear(x, p + tap + offset); mask NULL = DCNv1 (all ones).
 * Replaces modulated_deformable_im2col_cuda / deformable_im2col
 * (deform_conv_cuda_kernel.cu:191-278, :571-634), batched over all images. */
int sr_dcn_im2col(const sr_dcn_desc* d, const void* x, const float* offset, const float* mask, void* cols,
                  void* stream);
/* Fused forward (bf16 only; groups 1, C = Cp = cgp = 64, Cout <= 64, cpg % 8 == 0 -- query with
 * sr_dcn_fwd_fused_ok): y[N][cout][Ho][Wo] fp32 = bf16(W x columns + bias), the columns gathered per
 * tap into LDS and never stored unless cols != NULL (then written as sr_dcn_im2col would, for the
 * backward's weight gradient).  x_blocked: x is [N][8][H][W][8] (channel vectors of 8 as planes; faster
 * gathers) instead of the NHWC [N][H][W][64] of the other entries.  wf: the GEMM weight image [wrows >= cout][ldw >= kh*kw*64] bf16, column
 * tap*64 + ci; bias fp32 [cout] or NULL.  Replaces modulated_deformable_im2col_cuda + the per-image
 * addmm of modulated_deform_conv_cuda_forward (deform_conv_cuda.cpp:560-590). */
int sr_dcn_fwd_fused_ok(const sr_dcn_desc* d, int cout);
int sr_dcn_fwd_fused(const sr_dcn_desc* d, const void* x, int x_blocked, const float* offset, const float* mask,
                     const void* wf, int ldw, int wrows, int cout, const float* bias, float* y, void* cols,
                     void* stream);
/* From dcols (= dy x W, column layout): grad_x += scatter (fp32 NHWC [N][H][W][Cp], caller
 * zeroes it; LDS fixed-point accumulation + fp32 atomics), grad_offset / grad_mask written in
 * full (grad_mask NULL for v1).  Workspace: sr_dcn_col2im_workspace bytes (per-image scale).
 * Replaces the col2im + col2im_coord pair (deform_conv_cuda_kernel.cu:280-466, :636-770). */
size_t sr_dcn_col2im_workspace(const sr_dcn_desc* d);
int sr_dcn_col2im(const sr_dcn_desc* d, const void* dcols, const void* x, const float* offset, const float* mask,
                  float* grad_x, float* grad_offset, float* grad_mask, void* workspace, size_t ws_bytes,
                  void* stream);
/* Fused backward without the column gradient matrix (bf16, groups 1, C = Cp = cgp = 64, cout_p <= 64, a
 * multiple of 8; query sr_dcn_bwd_fused_ok): from dy (bf16 NHWC [N][Ho][Wo][ldy], channels [0, cout_p))
 * and the transposed weight image wd (bf16 [K*64][ldw], row tap*64 + ci, column co -- the GEMM image the
 * dcols path multiplies dy by), each tap's dcols tile is formed on MFMA in registers and consumed at once:
 * grad_offset / grad_mask written in full; grad_x: grad_x_nchw = 0 -> += the bilinear scatter into fp32
 * NHWC [N][H][W][Cp] (caller zeroes it, as sr_dcn_col2im), 1 -> fp32 NCHW [N][C][H][W] written in full.
 * Same results as sr_dcn_col2im on dcols = bf16(dy x wd^T).  Workspace as sr_dcn_col2im.
 * Replaces the addmm into columns + col2im + col2im_coord of deform_conv_cuda.cpp:640-685. */
int sr_dcn_bwd_fused_ok(const sr_dcn_desc* d, int cout_p);
int sr_dcn_bwd_fused(const sr_dcn_desc* d, const void* dy, int ldy, const void* wd, int ldw, int cout_p, const void* x,
                     const float* offset, const float* mask, float* grad_x, int grad_x_nchw, float* grad_offset,
                     float* grad_mask, void* workspace, size_t ws_bytes, void* stream);

/* deform_conv_ext-compatible entries (basicsr/ops/dcn/src/deform_conv_ext.cpp:52-163; argument order
 * of :52-57, :70-76, :89-94, :107-113, :127-134): the reference's tensors in its order as fp32 NCHW
 * contiguous device pointers, then the sizes they carried (input N, C, H, W; Cout = weight.size(0)),
 * then the reference's integer arguments in its order, then a workspace of
 * sr_deform_conv_workspace(...) bytes (the same query serves all five; the modulated entries use
 * im2col_step = N) and the stream.  Buffer semantics as deform_conv_cuda.cpp: output written;
 * gradInput / grad_input += (the reference scatters into it atomically); gradOffset / grad_offset /
 * grad_mask written; gradWeight += scale * dW; grad_weight / grad_bias +=.  columns / ones are
 * accepted and ignored (the reference re-allocates columns itself, deform_conv_cuda.cpp:198, 303, 419,
 * 532, 610; the bias rides in the GEMM epilogue).  with_bias: 0 / 1. */
size_t sr_deform_conv_workspace(int N, int C, int H, int W, int Cout, int kW, int kH, int dW, int dH, int padW,
                                int padH, int dilationW, int dilationH, int group, int deformable_group,
                                int im2col_step);
int sr_deform_conv_forward(const float* input, const float* weight, const float* offset, float* output,
                           float* columns, float* ones, int N, int C, int H, int W, int Cout, int kW, int kH, int dW,
                           int dH, int padW, int padH, int dilationW, int dilationH, int group, int deformable_group,
                           int im2col_step, void* workspace, size_t ws_bytes, void* stream);
int sr_deform_conv_backward_input(const float* input, const float* offset, const float* gradOutput, float* gradInput,
                                  float* gradOffset, const float* weight, float* columns, int N, int C, int H, int W,
                                  int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationW,
                                  int dilationH, int group, int deformable_group, int im2col_step, void* workspace,
                                  size_t ws_bytes, void* stream);
int sr_deform_conv_backward_parameters(const float* input, const float* offset, const float* gradOutput,
                                       float* gradWeight, float* columns, float* ones, int N, int C, int H, int W,
                                       int Cout, int kW, int kH, int dW, int dH, int padW, int padH, int dilationW,
                                       int dilationH, int group, int deformable_group, float scale, int im2col_step,
                                       void* workspace, size_t ws_bytes, void* stream);
int sr_modulated_deform_conv_forward(const float* input, const float* weight, const float* bias, float* ones,
                                     const float* offset, const float* mask, float* output, float* columns, int N,
                                     int C, int H, int W, int Cout, int kernel_h, int kernel_w, int stride_h,
                                     int stride_w, int pad_h, int pad_w, int dilation_h, int dilation_w, int group,
                                     int deformable_group, int with_bias, void* workspace, size_t ws_bytes,
                                     void* stream);
int sr_modulated_deform_conv_backward(const float* input, const float* weight, const float* bias, float* ones,
                                      const float* offset, const float* mask, float* columns, float* grad_input,
                                      float* grad_weight, float* grad_bias, float* grad_offset, float* grad_mask,
                                      const float* grad_output, int N, int C, int H, int W, int Cout, int kernel_h,
                                      int kernel_w, int stride_h, int stride_w, int pad_h, int pad_w, int dilation_h,
                                      int dilation_w, int group, int deformable_group, int with_bias,
                                      void* workspace, size_t ws_bytes, void* stream);

/* fused_bias_act_op (basicsr/ops/fused_act/src/fused_bias_act_kernel.cu): out = scale *
 * act(x + bias[(i / step_b) % size_b]) with act 1 linear / 3 leaky-relu(alpha), grad 0/1/2
 * (grad 1 gates by ref > 0).  bias / ref may be NULL.  size_x < 2^31 (as the reference). */
int sr_fused_bias_act(int dtype, const void* x, const void* bias, const void* ref, void* out, int64_t size_x,
                      int step_b, int size_b, int act, int grad, float alpha, float scale, void* stream);
/* FusedLeakyReLUFunctionBackward.forward (fused_act.py:30-44) on [R][C][S]:
 * dx = dy * scale * (out > 0 ? 1 : alpha); grad_bias[c] = sum of dx over R, S (fp32,
 * deterministic; grad_bias may be NULL). */
size_t sr_fused_lrelu_bwd_workspace(int R, int C, int64_t S);
int sr_fused_lrelu_bwd(int dtype, const void* dy, const void* out, void* dx, float* grad_bias, int R, int C,
                       int64_t S, float alpha, float scale, void* workspace, size_t ws_bytes, void* stream);

/* upfirdn2d (basicsr/ops/upfirdn2d/upfirdn2d.py:97-192): planes [major][in_h][in_w], FIR
 * kernel fp32 [kh][kw]; out [major][out_h][out_w]. */
int sr_upfirdn2d_out_size(int in_h, int in_w, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                          int pad_x0, int pad_x1, int pad_y0, int pad_y1, int* out_h, int* out_w);
int sr_upfirdn2d(int dtype, const void* x, int major, int in_h, int in_w, const float* kernel, int kh, int kw,
                 int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                 void* out, void* stream);

/* The Real-ESRGAN degradation pipeline on the device (csrc/degrade.hip; basicsr/models/realesrgan_model.py:68-185).
 * Images are contiguous NCHW fp32; every pointer 4-byte aligned (16-byte vector stores are chosen where the
 * pointer and the row length allow, never required); tensors below 2^31 elements; no fp atomics.
 * round255 != 0 stores clamp(rint(255 v), 0, 255) / 255 (a true division) in place of v. */

/* filter2D (img_process_util.py:7-31): reflect-padded correlation of every plane of sample n with
 * kernel[n] ([B][k][k], kernel_batch != 0) or kernel[0] ([1][k][k]); k odd, 3..21; k / 2 < min(H, W);
 * y must not be x. */
int sr_filter2d(const float* x, int B, int C, int H, int W, const float* kernel, int kernel_batch, int k, int round255,
                float* y, void* stream);
/* Separable blur: y = the r-tap filter `taps` along rows, then along columns, each reflect-padded by r / 2
 * (r odd <= 51, r / 2 < min(H, W)); tmp (planes H W floats) holds the row pass.  Two launches. */
int sr_sep_blur(const float* x, int planes, int H, int W, const float* taps, int r, float* tmp, float* y,
                void* stream);
/* USMSharp.forward (img_process_util.py:74-83) with the separable blur: residual = x - blur(x) and
 * mask = |residual| * 255 > threshold (both written, planes H W floats each), soft = blur(mask),
 * y = soft * clip(x + weight * residual, 0, 1) + (1 - soft) * x.  sr_usm_sharp_launches() kernel launches:
 * row, column + residual / mask, row, column + blend. */
int sr_usm_sharp_launches(void);
int sr_usm_sharp(const float* x, int planes, int H, int W, const float* taps, int r, float weight, float threshold,
                 float* tmp, float* residual, float* mask, float* y, void* stream);
/* F.interpolate(align_corners=False, antialias=False) to Hout x Wout; mode 0 area (adaptive average,
 * integer windows), 1 bilinear, 2 bicubic (A = -0.75, clamped indices, not clamped values).  scale_h / scale_w:
 * the source-coordinate scales, 1 / scale_factor when torch is given a scale_factor, in / out when it is given
 * a size (ignored by area). */
int sr_resize(const float* x, int planes, int Hin, int Win, int Hout, int Wout, int mode, float scale_h, float scale_w,
              float* y, void* stream);
/* add_gaussian_noise_pt (degradations.py:460-511) with the draws given: out = clamp(img + (normal sigma_n / 255)
 * (1 - gray_n) + (normal_gray sigma_n / 255) gray_n, 0, 1); img, normal [B][3][H][W], normal_gray [H][W] shared
 * by the batch, sigma, gray [B]; normal_gray and gray both NULL: colour noise only.  finish (both noise entries):
 * flags 1 = round to 8 bits (rint(255 v) / 255), 2 = no clip, 4 = store the noise alone, without the image. */
int sr_gaussian_apply(const float* img, const float* normal, const float* normal_gray, const float* sigma,
                      const float* gray, int B, int H, int W, int finish, float* out, void* stream);
/* generate_poisson_noise_pt (degradations.py:609-654) without the host: sr_level_presence ORs the 8-bit levels
 * clamp(rint(255 v), 0, 255) present in sample n into bitmap[n][0][8] (the three channels) and bitmap[n][1][8]
 * (the gray image 0.2989 r + 0.587 g + 0.114 b); the caller zeroes bitmap ([B][2][8] 32-bit words) first.
 * sr_poisson_rate: vals[n][c] = 2^ceil(log2(levels present)), rate_c [B][3][H][W] = level / 255 * vals[n][0],
 * rate_g [B][H][W] likewise for gray.  sr_poisson_apply: out = clamp(img + ((draw_c / vals_c - level / 255)
 * (1 - gray_n) + (draw_g / vals_g - gray level / 255) gray_n) scale_n, 0, 1); draw_g and gray both NULL:
 * colour noise only. */
int sr_level_presence(const float* img, int B, int H, int W, unsigned* bitmap, void* stream);
int sr_poisson_rate(const float* img, const unsigned* bitmap, int B, int H, int W, float* rate_c, float* rate_g,
                    float* vals, void* stream);
int sr_poisson_apply(const float* img, const float* draw_c, const float* draw_g, const float* vals, const float* scale,
                     const float* gray, int B, int H, int W, int finish, float* out, void* stream);
/* DiffJPEG.forward (diffjpeg.py:449-491) of x [B][3][H][W] in [0, 1] at quality[n] ([B], read only): zero pad
 * to multiples of 16, x 255, YCbCr, 2 x 2 chroma mean, 8 x 8 DCT, / (table factor_n), rint (differentiable != 0:
 * r + (v - r)^3), and back; y = clamp(., 0, 255) / 255 cropped to H x W.  coef (may be NULL): the quantised
 * coefficients, Y [B][H16/8][W16/8][8][8] followed by Cb and Cr [B][H16/16][W16/16][8][8] each. */
int sr_jpeg(const float* x, int B, int H, int W, const float* quality, int differentiable, int round255, float* y,
            float* coef, void* stream);
/* Bilinear x2 with an output scale (EDVR's PCD alignment: upsample(offset) * 2 in one pass): the result of
 * sr_bilinear_up2_fwd / _bwd times scale, multiplied in fp32 before the one rounding on store. */
int sr_bilinear_up2_fwd_scaled(int dtype, const void* x, int N, int H, int W, int C, float scale, void* y, void* stream);
int sr_bilinear_up2_bwd_scaled(int dtype, const void* dy, int N, int H, int W, int C, float scale, void* dx,
                               void* stream);
/* ---------------------------------------------------------------------------------
 * EDVR kernels (csrc/edvr.hip; basicsr/archs/edvr_arch.py).  Feature maps are dense NHWC of dtype (SR_F32 /
 * SR_BF16), 16-byte aligned, channels multiples of 8, fp32 arithmetic.  Fixed summation orders, no atomics: two
 * calls give identical bits; nothing allocates or synchronises.  SR_EINVAL for null or misaligned pointers,
 * non-positive sizes and unsupported channel counts, SR_ETOOBIG when a tensor reaches 2^31 bytes; nothing is
 * launched then.
 *
 * nn.Conv2d(cin, cout, 3, 2, 1) on x [N, H, W, Cin] -> y [N, Ho, Wo, Cout], Ho = (H - 1) / 2 + 1 (odd sizes
 * included), H, W >= 2, Cin and Cout multiples of 8 from 8 to 512.  An implicit GEMM on MFMA bf16 16x16x32 /
 * f32 16x16x4 with fp32 sums, the sibling of sr_conv4s2_*.
 * prep: the GEMM images of the fp32 parameter w [cout_real][cin_real][3][3] in dtype: wf [Cout][9 * Cin] for the
 *   forward, wd (9 * Cin * Cout elements) for the dgrad: one image [Cin][taps * Cout] per (row, column) parity
 *   class of the input pixel with 1, 2, 2 and 4 taps; padded channels are zeros.
 * fwd: y = act(conv + bias), bias fp32 [cout_real] or NULL, act SR_ACT_NONE or SR_ACT_LRELU with slope, applied
 *   to the fp32 sums; padded output channels are zeros.
 * dgrad: dx [N, H, W, Cin] from dy [N, Ho, Wo, Cout]; every dx element is written once (a gather over the four
 *   parity classes, 9 tap products per 4 pixels).
 * wgrad: dw [cout_real][cin_real][3][3] fp32 = (or += with accumulate) scale * the weight gradient; split K over
 *   sr_conv3s2_wgrad_splits blocks of output pixels, fp32 partials in ws (sr_conv3s2_wgrad_workspace bytes),
 *   summed in split order.  The bias gradient is sr_channel_reduce of dy. */
int sr_conv3s2_prep(int dtype, const float* w, int cout_real, int cin_real, int Cout, int Cin, void* wf, void* wd,
                    void* stream);
int sr_conv3s2_fwd(int dtype, const void* x, const void* wf, const float* bias, int N, int H, int W, int Cin, int Cout,
                   int cout_real, int act, float slope, void* y, void* stream);
int sr_conv3s2_dgrad(int dtype, const void* dy, const void* wd, int N, int H, int W, int Cin, int Cout, void* dx,
                     void* stream);
size_t sr_conv3s2_wgrad_workspace(int N, int H, int W, int Cin, int Cout);
int sr_conv3s2_wgrad_splits(int N, int H, int W, int Cin, int Cout);
int sr_conv3s2_wgrad(int dtype, const void* dy, const void* x, int N, int H, int W, int Cin, int cin_real, int Cout,
                     int cout_real, float scale, int accumulate, float* dw, void* ws, size_t ws_bytes, void* stream);
/* nn.MaxPool2d(3, 2, 1) and nn.AvgPool2d(3, 2, 1) of x [N, H, W, C] in one pass: y [N, Ho, Wo, 2C] with the max in
 * channels [0, C) and the average in [C, 2C).  Max: padding never wins, the first maximum in row-major window order
 * wins, a NaN propagates (torch).  Average: the fp32 window sum divided by 9 everywhere (count_include_pad).
 * bwd: dx [N, H, W, C] from dy [N, Ho, Wo, 2C], all of it written: per input pixel the max gradient of the (at most
 *   four) windows that chose it, the choice recomputed from x, plus the sum of their average gradients / 9. */
int sr_pool3s2_fwd(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream);
int sr_pool3s2_bwd(int dtype, const void* x, const void* dy, int N, int H, int W, int C, void* dx, void* stream);
/* Temporal attention of TSAFusion: emb, aligned [B * T, H, W, C], emb_ref [B, H, W, C] (C <= 512):
 * prob [B, T, H, W] fp32 = sigmoid(sum_c emb * emb_ref), out [B, H, W, T * C], out[..., t * C + c] =
 * aligned[b * T + t][...][c] * prob.
 * bwd, from d_out: d_aligned = d_out * prob, dcorr = (sum_c d_out * aligned) * prob * (1 - prob),
 *   d_emb = dcorr * emb_ref, d_emb_ref = sum over t ascending of dcorr_t * emb_t. */
int sr_tsa_corr_fwd(int dtype, const void* emb, const void* emb_ref, const void* aligned, int B, int T, int H, int W,
                    int C, void* out, float* prob, void* stream);
int sr_tsa_corr_bwd(int dtype, const void* d_out, const void* emb, const void* emb_ref, const void* aligned,
                    const float* prob, int B, int T, int H, int W, int C, void* d_aligned, void* d_emb, void* d_emb_ref,
                    void* stream);
/* y = feat * sigmoid(attn) * 2 + attn_add over n elements (a multiple of 8); bwd: d_feat = dy * 2 sigmoid(attn),
 * d_attn = dy * 2 feat * sigmoid(attn) (1 - sigmoid(attn)); the gradient of attn_add is dy itself. */
int sr_tsa_modulate_fwd(int dtype, const void* feat, const void* attn, const void* attn_add, int64_t n, void* y,
                        void* stream);
int sr_tsa_modulate_bwd(int dtype, const void* dy, const void* feat, const void* attn, int64_t n, void* d_feat,
                        void* d_attn, void* stream);

/* ---------------------------------------------------------------------------------
 * ECBSR on its collapsed form (csrc/ecb.hip).  An ECB block (basicsr/archs/ecbsr_arch.py) is a 3x3 conv plus
 * four 1x1 -> 3x3 sequences (a free 3x3 with mid_planes channels; Sobel-x, Sobel-y and Laplacian depthwise
 * masks times a per-channel scale), every 1x1 output padded with its own bias; the sum is one 3x3 conv with
 *   RK[o][i][t] = W3 + sum_m k1[o][m][t] k0[m][i] + sum_e scale_e[o] mask_e[o][t] k0_e[o][i] (+ 1 at o == i,
 *                 centre tap, with_idt)
 *   RB[o] = b3 + sum_m (sum_t k1[o][m][t]) b0[m] + b1 + sum_e (scale_e[o] (sum_t mask_e[o][t]) b0_e[o] + bias_e[o]).
 * A net's blocks are described by a table of sr_ecb_block in DEVICE memory (all pointers device pointers, fp32
 * unless noted), built once; sr_ecb_table_check validates a HOST copy of it (channels 1 .. 64, mid_planes
 * 1 .. 256, padded counts the next multiples of 8, no null parameter or image pointer) before it is uploaded.
 * ------------------------------------------------------------------------------- */
typedef struct sr_ecb_block {
  const float* w3;        /* conv3x3.weight [Cout][Cin][3][3] */
  const float* b3;        /* conv3x3.bias [Cout] */
  const float* k0;        /* conv1x1_3x3: k0 [mid][Cin], b0 [mid], k1 [Cout][mid][3][3], b1 [Cout] */
  const float* b0;
  const float* k1;
  const float* b1;
  const float* ek0[3];    /* edge branches sbx, sby, lpl: k0 [Cout][Cin], b0 [Cout], scale [Cout], bias [Cout], */
  const float* eb0[3];    /* mask [Cout][3][3] (read, never assumed) */
  const float* escale[3];
  const float* ebias[3];
  const float* emask[3];
  float* rk;              /* out: collapsed weight [Cout][Cin][3][3] */
  float* rb;              /* out: collapsed bias [Cout] */
  void* wf;               /* out: forward GEMM image [Cout_p][P 9 Cin_p], K = (part 9 + tap) Cin_p + ci, feature dtype */
  void* wd;               /* out: input-gradient image [Cin_p][P 9 Cout_p], taps flipped, feature dtype */
  float* bias_g;          /* out: RB padded to [Cout_p] */
  const float* drk;       /* backward in: dRK [Cout][Cin][3][3], dRB [Cout] */
  const float* drb;
  float* g_w3;            /* backward out: the gradients, in the order of the parameters above */
  float* g_b3;
  float* g_k0;
  float* g_b0;
  float* g_k1;
  float* g_b1;
  float* g_ek0[3];
  float* g_eb0[3];
  float* g_escale[3];
  float* g_ebias[3];
  float* g_act;           /* PReLU slope gradient [Cout] (sr_ecb_da_reduce) or NULL */
  int Cin, Cout, mid, Cin_p, Cout_p, with_idt;
} sr_ecb_block;
int sr_ecb_table_check(const sr_ecb_block* host_table, int L);
/* One launch over all L blocks (grid max_cout_p x L): rk, rb, and the images wf / wd / bias_g in `dtype`
 * (padded rows and columns exactly zero).  fp32 arithmetic in a fixed order.  fp32 images have P = 1 part, the
 * sr_convk_fwd layout; bf16 images P = 2: part 0 is RK rounded to bf16 (hi), part 1 the rounded remainder
 * RK - hi (lo), which the conv multiplies with the same nine taps -- the collapsed weight is not a bf16 number
 * even when every parameter is, and hi + lo keeps it to ~2^-17. */
int sr_ecb_rep_fwd(int dtype, const sr_ecb_block* table, int L, int max_cout_p, void* stream);
/* The transpose, one launch (grid max_units x L, max_units >= every Cout + mid): from drk / drb the gradients of
 * the 18 trainable tensors of every block, written (accumulate 0) or added in place (1); every element by one
 * thread in a fixed order, no atomics.
 *   dW3 = dRK; db3 = db1 = dbias_e = dRB; dk1[o][m][t] = sum_i dRK[o][i][t] k0[m][i] + dRB[o] b0[m];
 *   dk0[m][i] = sum_{o,t} dRK[o][i][t] k1[o][m][t]; db0[m] = sum_o dRB[o] sum_t k1[o][m][t];
 *   dscale_e[o] = sum_i (sum_t dRK[o][i][t] mask_e[o][t]) k0_e[o][i] + dRB[o] (sum_t mask_e) b0_e[o];
 *   dk0_e[o][i] = scale_e[o] sum_t mask_e[o][t] dRK[o][i][t]; db0_e[o] = scale_e[o] (sum_t mask_e) dRB[o]. */
int sr_ecb_rep_bwd(const sr_ecb_block* table, int L, int max_units, int accumulate, void* stream);
/* 3x3 conv, stride 1, zero padding 1, on dense NHWC maps of `dtype` with padded channel counts Cin, Cout
 * (multiples of 8, <= 64), any N, H, W >= 1; w is a GEMM image [Cout][P 9 Cin] as written by sr_ecb_rep_fwd.
 *   mode 0  z = conv + bias; y = z > 0 ? z : slope[c] z (slope NULL: y = z).  y, and z unless NULL, are stored
 *           [N][H][W][Cout]; padded channels exactly zero.  slope has Cout_real entries.
 *   mode 1  the network tail: out[n][c][h ps + i][w ps + j] = conv[q] + bias[q] + img[n][img_c == 1 ? 0 : c][h][w],
 *           q = c ps^2 + i ps + j < Cout_real; img, out fp32 NCHW.
 *   mode 2  the input gradient on the flipped transposed image wd (x = the consumer's dz, Cout = the producer's
 *           padded channels): y = g * (z > 0 ? 1 : slope[c]) with g the conv and z the producer's stored
 *           pre-activation (NULL: y = g; at z == 0 the gate is the slope, as torch); with `parts`
 *           [sr_ecb_conv_blocks(d)][64] each block also writes its channel sums of g * min(z, 0). */
typedef struct sr_ecb_conv_desc {
  int dtype;
  int mode;
  int N, H, W;
  int Cin, Cout, Cout_real;
  int ps;     /* mode 1 */
  int img_c;  /* mode 1 */
} sr_ecb_conv_desc;
int sr_ecb_conv_blocks(const sr_ecb_conv_desc* d);
int sr_ecb_conv(const sr_ecb_conv_desc* d, const void* x, const void* w, const float* bias, const float* slope, void* y,
                void* z, float* parts, const float* img, float* out, void* stream);
/* g_act[c] (+)= sum over the nblocks partial rows of layer l (parts [layers][nblocks][64]) for the first `layers`
 * table entries whose g_act is not NULL; fixed order. */
int sr_ecb_da_reduce(const sr_ecb_block* table, int layers, const float* parts, int nblocks, int accumulate, void* stream);
/* dz[n][h][w][q] = dOut[n][q / s^2][h s + i][w s + j], q = c s^2 + i s + j < C s^2 (pixel-unshuffle of the fp32
 * NCHW output gradient into the NHWC map of `dtype` with Cp >= C s^2 channels, the rest zero). */
int sr_ecb_tail_bwd(int dtype, const float* dout, int N, int C, int H, int W, int s, int Cp, void* dz, void* stream);

#ifdef __cplusplus
}
#endif
#endif
