// Deformable convolution (DCNv1 / DCNv2) for gfx950: the entry points, the shape predicates and every
// geometry.  This file has no kernel; the kernels and their launchers are in one source per family.
//
// The reference (basicsr/ops/dcn/src/deform_conv_cuda.cpp:490-685, kernels
// deform_conv_cuda_kernel.cu:571-770) loops over the batch: per image it builds an fp32
// column matrix [C*K, Ho*Wo] with one thread per (c, pixel), runs a serial addmm, and in
// backward scatters with atomics and re-reads the columns once per offset channel.
//
// Here the deformable part is reduced to batched HBM-bound passes around MFMA GEMMs (the GEMMs are the 1x1
// path of the conv code: conv3x3.hip selects, conv3x3_linear.hip has the kernels), or fused with them:
//   dcn_cols.hip      : the any-shape column path.  sr_dcn_im2col builds the pixel-major column matrix of
//                       all images in one launch; sr_dcn_col2im is the reference's backward scatters as two
//                       passes over dcols (dcn_coord_grad_kernel, dcn_grad_x_kernel).
//   dcn_fwd_fused.hip : sr_dcn_fwd_fused (bf16, C = 64, Cout <= 64), the sampling and the GEMM in one
//                       kernel: dcn_fwd_win_kernel for NHWC x, dcn_fwd_mfma_kernel for blocked x.
//   dcn_bwd_win.hip   : the backward on the forward's 8 x 16 tile and LDS window: dcn_coord_win_kernel (the
//                       coordinate pass of sr_dcn_col2im for the fused forward's shapes) and sr_dcn_bwd_fused
//                       (dcn_coord_dy8_kernel, dcn_gradx_dy8_kernel), which never stores dcols.
//   dcn_args.h        : the argument struct, geometries, tile constants and launchers these share.
//   dcn_dev.h         : the device helpers more than one family uses.
#include "dcn_args.h"

#include <algorithm>
#include <cstdlib>

using namespace sr_dcn;

namespace {

int make_args(const sr_dcn_desc* d, DcnArgs& a) {
  if (!d) return sr_fail(SR_EINVAL, "dcn: null descriptor");
  a.N = d->N; a.C = d->C; a.H = d->H; a.W = d->W; a.Cp = d->Cp; a.Ho = d->Ho; a.Wo = d->Wo;
  a.kh = d->kh; a.kw = d->kw; a.sh = d->stride_h; a.sw = d->stride_w; a.ph = d->pad_h; a.pw = d->pad_w;
  a.dh = d->dil_h; a.dw = d->dil_w; a.G = d->groups; a.DG = d->deformable_groups; a.cgp = d->cgp;
  if (a.N <= 0 || a.C <= 0 || a.H <= 0 || a.W <= 0 || a.Ho <= 0 || a.Wo <= 0 || a.kh <= 0 || a.kw <= 0 ||
      a.sh <= 0 || a.sw <= 0 || a.dh <= 0 || a.dw <= 0 || a.ph < 0 || a.pw < 0)
    return sr_fail(SR_EINVAL, "dcn: non-positive size");
  if (a.G <= 0 || a.DG <= 0 || a.C % a.G || a.C % a.DG)
    return sr_fail(SR_EINVAL, "dcn: channels must be divisible by groups and deformable_groups");
  if (a.Cp < a.C || a.Cp % 8) return sr_fail(SR_EINVAL, "dcn: Cp must be >= C and a multiple of 8");
  a.cg = a.C / a.G;
  a.cpg = a.C / a.DG;
  if (a.cgp < a.cg || a.cgp % 8) return sr_fail(SR_EINVAL, "dcn: cgp must be >= C/groups and a multiple of 8");
  if (a.Ho != (a.H + 2 * a.ph - (a.dh * (a.kh - 1) + 1)) / a.sh + 1 ||
      a.Wo != (a.W + 2 * a.pw - (a.dw * (a.kw - 1) + 1)) / a.sw + 1)
    return sr_fail(SR_EINVAL, "dcn: output size does not match the convolution geometry");
  a.K = a.kh * a.kw;
  a.L = a.G * a.K * a.cgp;
  // pixel tile: offsets + masks of every deformable group in LDS (<= 64 KB)
  a.TP = 64;
  while (a.TP > 16 && (size_t)a.DG * 3 * a.K * a.TP * 4 > 32768) a.TP >>= 1;
  while (a.TP > 1 && (size_t)a.DG * 3 * a.K * a.TP * 4 > 65536) a.TP >>= 1;
  if ((size_t)a.DG * 3 * a.K * a.TP * 4 > 65536) return sr_fail(SR_EINVAL, "dcn: too many deformable groups x taps");
  return SR_OK;
}

// Input pixels along one axis that T output pixels can sample with offsets up to R: the undeformed receptive
// field, R pixels on each side and the far bilinear corners.
int footprint(int T, int stride, int k, int dil, int R) { return (T - 1) * stride + (k - 1) * dil + 2 * R + 2; }

// Scatter geometry of dcn_grad_x_kernel
XGeom grad_x_geom(const DcnArgs& a) {
  // largest (tile, halo) whose LDS footprint fits 64 KB; halo 0 still covers the
  // undeformed footprint, anything outside goes to global atomics
  static const int cfg[][2] = {{16, 4}, {16, 2}, {8, 4}, {8, 2}, {8, 0}, {4, 0}};
  // channels per pass: 8, or knob SR_DCN_CPP = 16 / 32 (A/B: fewer passes over dcols, a larger LDS image)
  const int cpp = sr_knob(K_DCN_CPP) == 16 || sr_knob(K_DCN_CPP) == 32 ? sr_knob(K_DCN_CPP) : 8;
  XGeom g;
  g.CPP = cpp;
  const size_t lim = cpp == 8 ? 65536 : 160 * 1024;
  for (const auto& c : cfg) {
    g.TT = c[0];
    g.R = c[1];
    g.RH = footprint(g.TT, a.sh, a.kh, a.dh, g.R);
    g.RW = footprint(g.TT, a.sw, a.kw, a.dw, g.R);
    if ((size_t)g.RH * g.RW * (g.CPP + 1) * 8 <= lim) return g;
  }
  g.CPP = 8;
  g.TT = 4; g.R = 0; g.RH = g.RW = 1;  // degenerate footprint: everything through global atomics
  return g;
}

// Ablation mask of dcn_fwd_win_kernel (SR_DCN_DBG, read per call; tools/dcn_ablate.py): 1 no global
// fallback, 2 constant offsets (no offset / mask reads), 4 no MFMA, 8 no window staging.  Results are
// wrong under any of them; 0 (unset) is the kernel.
int dcn_dbg() { return sr_knob(K_DCN_DBG) > 0 ? sr_knob(K_DCN_DBG) : 0; }

// x window of an 8 x 16 output tile in LDS (128 B per pixel): the largest margin R <= r0 with which the kernel's
// fixed LDS bytes and the window fit lim.
bool window_geom(const DcnArgs& a, int r0, size_t fixed, size_t lim, int* R, int* WH, int* WW, size_t* lds) {
  for (int r = r0; r >= 0; --r) {
    const int wh = footprint(DW_TH, a.sh, a.kh, a.dh, r), ww = footprint(DW_TW, a.sw, a.kw, a.dw, r);
    const size_t l = fixed + (size_t)wh * ww * 128;
    if (l <= lim) {
      *R = r; *WH = wh; *WW = ww; *lds = l;
      return true;
    }
  }
  return false;
}

// dcn_fwd_win_kernel: A tile, weight slice and window within 160 KB; R <= 2, or knob SR_DCN_R (0 .. 6)
bool win_geom(const DcnArgs& a, int* R, int* WH, int* WW, size_t* lds) {
  const int rk = sr_knob(K_DCN_R);
  return window_geom(a, rk >= 0 && rk <= 6 ? rk : 2, (size_t)(DF_TP + 64) * DF_RS * 2, 160 * 1024, R, WH, WW, lds);
}

// Shapes the fused forward takes (see dcn_fwd_mfma_kernel); SR_DCN_FUSED=0 turns it off (A/B).
bool dcn_fused_ok(const sr_dcn_desc* d, const DcnArgs& a, int cout) {
  const bool off = sr_knob(K_DCN_FUSED) == 0;
  return !off && d->dtype == SR_BF16 && a.G == 1 && a.C == 64 && a.Cp == 64 && a.cgp == 64 && cout >= 1 &&
         cout <= 64 && a.cpg % 8 == 0 && (size_t)a.H * a.W * a.Cp * 2 < 0x80000000ull;
}

// dcn_coord_win_kernel's shapes (as the fused forward's, any Cout) and window (R <= 2, LDS <= 80 KB
// so two blocks share a CU); SR_DCN_COORD_WIN=0 keeps dcn_coord_grad_kernel (A/B).
bool coord_win_ok(const sr_dcn_desc* d, const DcnArgs& a) {
  const bool off = sr_knob(K_DCN_COORD_WIN) == 0;
  return !off && d->dtype == SR_BF16 && a.G == 1 && a.C == 64 && a.Cp == 64 && a.cgp == 64 && a.cpg % 8 == 0 &&
         (size_t)a.H * a.W * a.Cp * 2 < 0x80000000ull;
}
bool coord_win_geom(const DcnArgs& a, int* R, int* WH, int* WW, size_t* lds) {
  return window_geom(a, 2, (size_t)3 * a.DG * DF_TP * 4, 80 * 1024, R, WH, WW, lds);
}

// Shapes and geometry of the fused backward: coord_win's shapes with Cout <= 64; the coordinate
// kernel's LDS (weight slices + window, R <= 2) and the scatter image (R <= 4 for the int32 image, <= 2 for
// the int64 one) each within 80 KB, two blocks per CU.  (The op layer's SR_DCN_BWD_FUSED=0 keeps the dcols path.)
// Scatter image (A/B): knob SR_DCN_GX_FX=64 the int64 fixed-point image, else int32
int gx_fx_env() { return sr_knob(K_DCN_GX_FX) == 64 ? 64 : 32; }
// Bits of one contribution: 18 (48), lowered so that the 256 K contributions a cell can receive stay below
// 2^30 (2^62): 30 - ceil(log2(256 K)) is 18 up to 16 taps, 17 at 25, 16 at 49.
int gx_fx_bits(int fx, int K) {
  int lg = 0;  // ceil(log2(256 K))
  while ((1ll << lg) < 256ll * K) ++lg;
  return fx == 64 ? std::min(48, 62 - lg) : std::min(18, 30 - lg);
}

bool bwd_fused_geom(const sr_dcn_desc* d, const DcnArgs& a, int cop, BwdGeom* bg) {
  if (!coord_win_ok(d, a) || cop < 8 || cop > 64 || cop % 8) return false;
  bg->fx = gx_fx_env();
  bg->fxe = gx_fx_bits(bg->fx, a.K);
  if (!window_geom(a, 2, (size_t)2 * 64 * DF_RS * 2, 80 * 1024, &bg->R1, &bg->WH, &bg->WW, &bg->lds1)) return false;
  const size_t esz = bg->fx == 64 ? 8 : 4;
  for (int r = bg->fx == 64 ? 2 : 4; r >= 0; --r) {
    const int rh = footprint(DX_TT, a.sh, a.kh, a.dh, r), rw = footprint(DX_TT, a.sw, a.kw, a.dw, r);
    const size_t l = (size_t)rh * rw * DX_ST * esz;
    if (l <= 80 * 1024) {
      bg->R2 = r; bg->RH = rh; bg->RW = rw; bg->lds2 = l;
      return true;
    }
  }
  return false;
}

}  // namespace

extern "C" {

int sr_dcn_fwd_fused_ok(const sr_dcn_desc* d, int cout) {
  DcnArgs a;
  if (make_args(d, a) != SR_OK) return 0;
  return dcn_fused_ok(d, a, cout) ? 1 : 0;
}

int sr_dcn_fwd_fused(const sr_dcn_desc* d, const void* x, int x_blocked, const float* offset, const float* mask,
                     const void* wf, int ldw, int wrows, int cout, const float* bias, float* y, void* cols,
                     void* stream) {
  DcnArgs a;
  int rc = make_args(d, a);
  if (rc) return rc;
  if (!dcn_fused_ok(d, a, cout)) return sr_fail(SR_EINVAL, "dcn_fwd_fused: unsupported shape (query sr_dcn_fwd_fused_ok)");
  if (!x || !offset || !wf || !y) return sr_fail(SR_EINVAL, "dcn_fwd_fused: null pointer");
  if (ldw < a.K * 64 || wrows < cout || (size_t)wrows * ldw * 2 >= 0x80000000ull)
    return sr_fail(SR_EINVAL, "dcn_fwd_fused: weight image must be [>= cout][>= K*64] bf16");
  int R, WH, WW;
  size_t lds;
  if (!x_blocked && win_geom(a, &R, &WH, &WW, &lds))
    return launch_fwd_win(a, x, offset, mask, wf, ldw, wrows, cout, bias, y, cols, R, WH, WW, lds, dcn_dbg(),
                          (hipStream_t)stream);
  return launch_fwd_mfma(a, x, x_blocked, offset, mask, wf, ldw, wrows, cout, bias, y, cols, (hipStream_t)stream);
}

int sr_dcn_im2col(const sr_dcn_desc* d, const void* x, const float* offset, const float* mask, void* cols,
                  void* stream) {
  DcnArgs a;
  int rc = make_args(d, a);
  if (rc) return rc;
  if (!x || !offset || !cols) return sr_fail(SR_EINVAL, "dcn_im2col: null pointer");
  if (d->dtype != SR_BF16 && d->dtype != SR_F32) return sr_fail(SR_EINVAL, "dcn_im2col: bad dtype");
  return launch_im2col(a, d->dtype == SR_BF16, x, offset, mask, cols, (hipStream_t)stream);
}

int sr_dcn_bwd_fused_ok(const sr_dcn_desc* d, int cout_p) {
  DcnArgs a;
  BwdGeom bg;
  if (make_args(d, a) != SR_OK) return 0;
  return bwd_fused_geom(d, a, cout_p, &bg) ? 1 : 0;
}

int sr_dcn_bwd_fused(const sr_dcn_desc* d, const void* dy, int ldy, const void* wd, int ldw, int cout_p, const void* x,
                     const float* offset, const float* mask, float* grad_x, int grad_x_nchw, float* grad_offset,
                     float* grad_mask, void* workspace, size_t ws_bytes, void* stream) {
  DcnArgs a;
  int rc = make_args(d, a);
  if (rc) return rc;
  BwdGeom bg;
  if (!bwd_fused_geom(d, a, cout_p, &bg))
    return sr_fail(SR_EINVAL, "dcn_bwd_fused: unsupported shape (query sr_dcn_bwd_fused_ok)");
  if (!dy || !wd || !x || !offset || !grad_x || !grad_offset) return sr_fail(SR_EINVAL, "dcn_bwd_fused: null pointer");
  if (grad_mask && !mask) return sr_fail(SR_EINVAL, "dcn_bwd_fused: grad_mask needs mask");
  if (ldy < cout_p || ldy % 8 || ldw < cout_p || ldw % 8)
    return sr_fail(SR_EINVAL, "dcn_bwd_fused: dy / weight image strides must be >= cout_p and multiples of 8");
  if ((size_t)a.Ho * a.Wo * ldy * 2 >= 0x80000000ull || (size_t)a.K * 64 * ldw * 2 >= 0x80000000ull)
    return sr_fail(SR_ETOOBIG, "dcn_bwd_fused: tensor >= 2 GiB per image");
  if (!workspace || ws_bytes < sr_dcn_col2im_workspace(d)) return sr_fail(SR_EINVAL, "dcn_bwd_fused: workspace too small");
  unsigned* amax = (unsigned*)workspace;
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(amax, 0, (size_t)a.N * sizeof(unsigned), s) != hipSuccess)
    return sr_fail(SR_ELAUNCH, "dcn_bwd_fused: memset failed");
  return launch_bwd_fused(a, bg, dy, ldy, wd, ldw, cout_p, x, offset, mask, grad_x, grad_x_nchw != 0, grad_offset,
                          grad_mask, amax, s);
}

size_t sr_dcn_col2im_workspace(const sr_dcn_desc* d) { return d ? (size_t)d->N * sizeof(unsigned) : 0; }

int sr_dcn_col2im(const sr_dcn_desc* d, const void* dcols, const void* x, const float* offset, const float* mask,
                  float* grad_x, float* grad_offset, float* grad_mask, void* workspace, size_t ws_bytes,
                  void* stream) {
  DcnArgs a;
  int rc = make_args(d, a);
  if (rc) return rc;
  if (!dcols || !x || !offset || !grad_x || !grad_offset) return sr_fail(SR_EINVAL, "dcn_col2im: null pointer");
  if (!workspace || ws_bytes < sr_dcn_col2im_workspace(d)) return sr_fail(SR_EINVAL, "dcn_col2im: workspace too small");
  unsigned* amax = (unsigned*)workspace;
  if (grad_mask && !mask) return sr_fail(SR_EINVAL, "dcn_col2im: grad_mask needs mask");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(amax, 0, (size_t)a.N * sizeof(unsigned), s) != hipSuccess)
    return sr_fail(SR_ELAUNCH, "dcn_col2im: memset failed");
  if (d->dtype != SR_BF16 && d->dtype != SR_F32) return sr_fail(SR_EINVAL, "dcn_col2im: bad dtype");
  const bool bf16 = d->dtype == SR_BF16;
  int R, WH, WW;
  size_t lds;
  const bool win = bf16 && coord_win_ok(d, a) && coord_win_geom(a, &R, &WH, &WW, &lds);
  if (win) {
    rc = launch_coord_win(a, dcols, x, offset, mask, grad_offset, grad_mask, amax, R, WH, WW, lds, s);
    if (rc) return rc;
  }
  return launch_col2im(a, grad_x_geom(a), bf16, dcols, x, offset, mask, grad_x, grad_offset, grad_mask, amax, s, !win);
}

}  // extern "C"
