// 3x3 / stride 1 / pad 1 convolution as an im2col-free implicit GEMM on CDNA4 MFMA.
//
// Replaces the cuDNN nn.Conv2d(C, C', 3, 1, 1) calls of the reference SR nets
// (basicsr/archs/arch_util.py:78-79, edsr_arch.py:44-48, rcan_arch.py:40-42,
// rrdbnet_arch.py:21-25): forward, data gradient (same kernel, flipped weights) and
// weight/bias gradient (split-K over pixels, deterministic slab reduction).
//
// GEMM view of the forward: rows m = output pixels (n, y, x) of the NHWC map, columns
// n = output channels, K = (tap, ci) with tap = ky*3 + kx.  The A tile of a K-step is a
// [BM pixels][128 B] slice of the input shifted by the tap (zeros outside the image come
// from the buffer range check), the B tile is [BN][128 B] of the weight rows; both are
// staged through registers into an XOR-swizzled LDS image (conflict-free ds_read_b128,
// tools/lds_banks.py) with one barrier per K-step and a double-buffered image.
// bf16 uses v_mfma_f32_16x16x32_bf16, fp32 (parity mode) v_mfma_f32_16x16x4_f32 on the
// same 16-byte chunk image.  The epilogue stages the fp32 tile through LDS and applies
// bias, activation, ReLU-mask gate, scale, residual, pixel-shuffle / NCHW store with
// 16-byte coalesced stores.
//
// This file is the host side: the kernel selection (every fwd_use_* / wg_use_* predicate, fwd_kind), the split plans,
// dispatch_fwd and the sr_conv3x3_* / sr_linear_ln_fwd entry points.  It has no kernel.  Every launch is a function
// next to its kernels, one source per kernel family; conv3x3_args.h declares the launchers and the predicates they call.
//   conv3x3_args.h            FwdArgs / WgArgs, epilogue bits, FwdKind, launcher and predicate declarations
//   conv3x3_dev.h             device helpers of more than one family (epilogue_tile, mfma_chunk, swz128, ...)
//   conv3x3_fwd_tile.hip      conv3x3_fwd_kernel, conv3x3_fwd_halo_kernel
//   conv3x3_fwd_pp.hip        conv3x3_fwd_big_kernel, conv3x3_fwd_pp_kernel, conv3x3_fwd_pph_kernel
//   conv3x3_fwd_band.hip      conv3x3_fwd_band_kernel
//   conv3x3_fwd_tail.hip      conv3x3_fwd_tail_kernel
//   conv3x3_linear.hip        linear_wk_kernel, conv3x3_lin_kernel, linear_wgrad_kernel
//   conv3x3_wgrad_tile.hip    conv3x3_wgrad_kernel, conv3x3_wgrad_big_kernel, conv3x3_wgrad_pp_kernel
//   conv3x3_wgrad_ring.hip    conv3x3_wgrad_ring_kernel, conv3x3_wgrad_row3_kernel
//   conv3x3_wgrad_reduce.hip  wgrad_reduce_kernel and its _narrow_ / _g_ / 4 / _tr_ forms
//   conv3x3_prep.hip          prep_kernel, prep_batch_kernel and the sr_conv_prep_* entry points
#include "conv3x3_args.h"

using namespace sr_conv;

namespace sr_conv __attribute__((visibility("hidden"))) {
namespace {
// set by sr_conv3x3_set_variant (tests / A-B timing): an sr_conv_variant of include/sr_hip.h
int g_variant = SR_VARIANT_AUTO;
}  // namespace
bool variant_is(int v) { return g_variant == v; }
// SR_VARIANT_TILE_ONLY: never a 256x256 kernel (nor any of the narrow-conv families)
bool tile_only() { return variant_is(SR_VARIANT_TILE_ONLY); }

// pph over 64-px column strips (STRIP): bf16, W a multiple of 64 above 128 (EDSR at LR 256: the body
// convs and their dgrads), H a multiple of 4, no pixel-shuffled input, no channel sums.
// SR_VARIANT_NO_PPH_STRIP: the pp kernel for them (A/B, tests).
bool fwd_use_pph_strip(const FwdArgs& a) {
  return !variant_is(SR_VARIANT_TWO_BARRIER) && !variant_is(SR_VARIANT_NO_PPH) && !variant_is(SR_VARIANT_NO_PPH_STRIP) &&
         a.W > 128 && a.W % 64 == 0 && a.H % 4 == 0 && a.Cin % 64 == 0 && a.in_ps == 0 && a.in_up == 1 && a.tap0 == 0 &&
         !a.colsum;
}
// Halo variant of the 256x256 kernel: whole-row tiles of W = 64 / 128 images, 64-channel chunks.
bool fwd_use_pph(const FwdArgs& a) {
  return !variant_is(SR_VARIANT_TWO_BARRIER) && !variant_is(SR_VARIANT_NO_PPH) &&
         ((a.W == 64 && a.H % 4 == 0) || (a.W == 128 && a.H % 2 == 0)) && a.Cin % 64 == 0 &&
         (a.in_ps == 0 || (a.fd_cps.d % 64 == 0 && !variant_is(SR_VARIANT_PPH_NO_PS))) && a.in_up == 1 && a.tap0 == 0;
}

// Grid of the persistent multi-tile form of the pph kernel (conv3x3_fwd_pph_kernel<4, 2, false, true>), 0:
// the one-tile form.  W 64 whole-row tiles (fwd_use_pph), Cout 256 (one full column tile), plain NHWC input and output,
// bias / activation / alpha and at most ONE of gate (modes 0, 1) and residual -- the EDSR / RCAN-style
// body convs and their dgrads -- and more tiles than G blocks (with one tile per block the form is the
// one-tile form).  G: the device's CU count, or knob SR_PPH_GRID (tests: several tiles per block at
// small shapes).  SR_VARIANT_PPH_ONE_TILE: the one-tile form for them (A/B, tests).
int pph_pers_grid(const FwdArgs& a) {
  if (variant_is(SR_VARIANT_PPH_ONE_TILE) || a.W != 64 || a.Cout != 256 || a.tiles_n != 1 || a.in_ps != 0 || a.out_ps != 0 || a.colsum || a.out_nchw ||
      a.aux || a.res2 || a.row_scale || a.dot || (a.gate && a.res) || (a.gate && a.gate_mode == 2) || a.M % 256)
    return 0;
  const int G = sr_knob(K_PPH_GRID) > 0 ? sr_knob(K_PPH_GRID) : sr_device_cus();
  return a.tiles > G ? G : 0;
}

// Narrow-conv halo kernel: bf16 3x3, W 64 or 128, whole-row 256-pixel tiles; Cout <= 64 in one
// block column, Cout 65..255 (RRDB dense-block dgrads) in 64-channel block columns.  (Round 4's
// one-row tiles for the wide W-256 convs measured slower than the pp / tile kernels and were removed
// in round 5: EDSR conv_last dgrad 1390 vs 550 us, profiles/r04/halo256/.)
bool fwd_use_halo(const FwdArgs& a, bool bf) {
  // pixel-shuffled input (the upsample convs' dgrads into 64 channels) when each 64-channel chunk lies
  // in one shuffle slot; SR_VARIANT_HALO_NO_PS: the tile kernel for those (A/B)
  const bool ps_ok = a.in_ps > 0 && a.fd_cps.d % 64 == 0 && a.W != 256 && !variant_is(SR_VARIANT_HALO_NO_PS);
  if (!bf || a.in_up != 1 || (a.in_ps != 0 && !ps_ok) || a.tap0 != 0 || tile_only()) return false;
  if (a.W == 256)  // HR-resolution tail convs (conv_last, Cout <= 16, NCHW store): one row per tile
    return a.Cout <= 16 && !variant_is(SR_VARIANT_NO_TAIL);
  return !a.out_nchw && a.Cout < 256 && (a.W == 64 || a.W == 128) && a.H % (256 / a.W) == 0;
}

// the bits of a compile-time epilogue code that the band and lin kernels share (EPI_*)
int epi_common(const FwdArgs& a) {
  int gate = 0;
  if (a.gate) gate = a.gate_mode == 2 ? 3 : (a.gate_mode == 1 ? 2 : 1);
  return a.act | (gate << EPI_GATE_SHIFT) | (a.res ? EPI_RES : 0) | (a.res2 ? EPI_RES2 : 0) | (a.aux ? EPI_AUX : 0);
}
// the band kernel's compile-time epilogue code (see conv3x3_fwd_band_kernel) for these arguments,
// -1 when it is not one of the instantiated ones
int band_epi(const FwdArgs& a, int grid) {
  const int e = epi_common(a) | (a.colsum || a.dot ? BAND_CS : 0) | (a.row_scale ? BAND_RSC : 0) |
                (a.dot ? BAND_DOT : 0);  // dot implies colsum
  if (a.row_scale) {  // the images of one band fit one wave's lanes
    const int rows = (a.N * a.H + grid - 1) / grid;
    if ((rows + a.H - 1) / a.H + 1 > 64) return -1;
  }
  switch (e) {
    case 0: case 1: case 2: case 4: case 16: case 20: case 28: case 48: case 72: case 128: case 304: return e;
    case 656: return a.Cin == 64 && a.Cout == 64 ? e : -1;  // RCAB conv1 dgrad + the CA dot partials
    default: return -1;
  }
}
// Blocks of a band launch over `rows` image rows (or strip rows): one block per CU (one wave per SIMD: the weights
// live in registers); SR_VARIANT_BAND_64 forces 64 blocks (long bands: ring wrap-around and image / strip crossings
// inside a band, for tests).  (Two bands per CU for the band_occ forms measured faster alone but slower in the RCAN
// step beside the side-stream weight gradients; the switch was removed in round 5.)
int band_grid(int rows) {
  const int gmax = variant_is(SR_VARIANT_BAND_64) ? 64 : 256;
  return rows < gmax ? rows : gmax;
}
bool band_off() { return tile_only() || variant_is(SR_VARIANT_NO_BAND); }  // the tile kernel instead (A/B, tests)
// row-streaming narrow conv: bf16 3x3, Cin 32 / 64, Cout 32 / 64 exactly, W 64 / 128, plain or
// channel-slice NHWC in and out
bool fwd_use_band(const FwdArgs& a, bool bf) {
  if (!(bf && a.tap0 == 0 && a.in_up == 1 && a.in_ps == 0 && !a.out_nchw && a.out_ps == 0 &&
        (a.W == 64 || a.W == 128) && (a.Cin == 32 || a.Cin == 64) && (a.Cout == 32 || a.Cout == 64) &&
        a.Cout_real == a.Cout && !band_off()))
    return false;
  return band_epi(a, band_grid(a.N * a.H)) >= 0;
}
// 64-channel-output convs on images wider than 128 px (W 256 / 512: the RRDBNet HR convs conv_up1 /
// conv_up2 / conv_hr, their dgrads and conv_last's dgrad from its 8 padded output channels), and W 128
// with the nearest x2 upsample folded in, as band launches over 128-px column strips (STRIP: E bit
// 10): Cin 64 with a plain, ReLU, LeakyReLU or lrelu-gate epilogue, Cin 8..32 plain or gated.
// SR_VARIANT_NO_BAND_STRIP: the generic tile kernel for them (A/B, tests).
bool fwd_use_band_strip(const FwdArgs& a, bool bf) {
  if (!(bf && a.tap0 == 0 && (a.in_up == 1 || a.in_up == 2) && a.in_ps == 0 && !a.out_nchw && a.out_ps == 0 &&
        a.W % 128 == 0 && (a.W > 128 || a.in_up == 2) && (a.Cin == 64 || (a.Cin <= 32 && a.Cin % 8 == 0)) &&
        (a.Cout == 64 || (a.Cin <= 32 && (a.Cout == 128 || a.Cout == 256))) && a.Cout_real == a.Cout &&
        !a.colsum && !a.dot && !a.row_scale && !a.res2 && !a.aux && !band_off() &&
        !variant_is(SR_VARIANT_NO_BAND_STRIP)))
    return false;
  const int e = band_epi(a, 256);
  if (a.Cout > 64) return e == 0;  // 8-channel input into 128 / 256 (EDSR's conv_last dgrad): one launch
  return a.Cin == 64 ? (e == 0 || e == 1 || e == 2 || e == 4) : (e == 0 || e == 4);
}
// the same from a narrow input (Cin 8..32) into 192 output channels (or 128 / 256 with an epilogue
// operand): 64-channel output-column slices, the narrow input re-read per slice.  (EDSR's conv_last
// dgrad, 8 -> 256 at HR, ran as four slices at 99 us each -- 2.7 TB/s, bound by the per-row latency of
// a band that stores 128 B per pixel -- and is now one CO 256 launch.)
bool fwd_use_band_strip_sliced(const FwdArgs& a, bool bf) {
  if (!(a.Cout > 64 && a.Cout <= 256 && a.Cout % 64 == 0 && a.Cin <= 32) || fwd_use_band_strip(a, bf)) return false;
  FwdArgs b = a;
  b.Cout = b.Cout_real = 64;
  return fwd_use_band_strip(b, bf);
}
// wider outputs (RRDB dense-block dgrads: Cout 96..192 from a 32- or 64-channel input) as
// band launches over 64-channel output column slices: the narrow input is re-read per slice
bool fwd_use_band_sliced(const FwdArgs& a, bool bf) {
  if (!(bf && a.tap0 == 0 && a.in_up == 1 && a.in_ps == 0 && !a.out_nchw && a.out_ps == 0 &&
        (a.W == 64 || a.W == 128) && (a.Cin == 32 || a.Cin == 64) && a.Cout > 64 && a.Cout < 256 &&
        a.Cout % 32 == 0 && a.Cout_real == a.Cout && !a.colsum && !band_off()))
    return false;
  return band_epi(a, band_grid(a.N * a.H)) >= 0;
}
// the lin kernel's compile-time epilogue code for these arguments (see conv3x3_lin_kernel), -1
// for the run-time-flag form; instantiated: plain (qkv fwd, proj dgrad), GELU' gate (fc2
// dgrad), residual (proj fwd), GELU + pre-activation (fc1 fwd), residual + row scale (proj
// fwd with stochastic depth)
int lin_epi(const FwdArgs& a) {
  const int e = epi_common(a) | (a.row_scale ? LIN_RSC : 0);
  if (a.row_scale && (a.H * a.W) % 128) return -1;  // row scale uniform per 128-token block
  if ((size_t)a.M * a.ldy * 2 >= 0x80000000ull) return -1;  // buffer-store offsets are 31-bit
  switch (e) {
    case 0: case 8: case 16: case 67: case 144: return e;
    default: return -1;
  }
}
// short-K 1x1 convs (linears): token tile staged once, all output channels swept.  K <= 192 on
// 128-token tiles; 192 < K <= 576 (SwinIR fc2 fwd 360 -> 184, fc1 / qkv dgrads 360 / 576 -> 184) on
// 64-token tiles, Cout <= 384 (SR_VARIANT_LIN_WIDE_BIG: those on the 256x256 pp kernel instead, for A/B)
bool fwd_use_lin(const FwdArgs& a, bool bf) {
  if (!(bf && a.tap0 == 4 && !a.out_nchw && a.out_ps == 0 && a.in_ps == 0 && a.in_up == 1 && !tile_only()))
    return false;
  if (a.Cin <= 192) return a.Cout <= 640;
  return a.Cin <= 576 && a.Cout <= 384 && !variant_is(SR_VARIANT_LIN_WIDE_BIG);
}
// linear_wk_kernel for the linears with K > SR_LWK_MINK (default 0: all; 192: only the wide-K ones,
// which the 64-token lin kernel took), K <= 576, 96 < Cout <= 576 and a plain / GELU' gate / GELU +
// pre-activation / residual / residual + row-scale epilogue; knob SR_LWK=0 or SR_VARIANT_NO_LINEAR_WK: the lin
// kernel (A/B, tests)
bool lin_use_wk(const FwdArgs& a) {
  const int mink = sr_knob(K_LWK) == 0 ? (1 << 30) : (sr_knob(K_LWK_MINK) > 0 ? sr_knob(K_LWK_MINK) : 0);
  if (variant_is(SR_VARIANT_NO_LINEAR_WK) || a.Cin <= mink || a.Cin > 576 || a.Cout > 576 || a.Cout <= 96) return false;
  const int e = lin_epi(a);
  return e == 0 || e == 8 || e == 16 || e == 67 || e == 144;
}
// HR tail convs: Cout <= 16 with the NCHW fp32 store, W >= 256 (32-px strips), Cin 64 / 128 / 256
bool fwd_use_tail(const FwdArgs& a, bool bf) {
  return bf && a.tap0 == 0 && a.in_up == 1 && a.in_ps == 0 && a.out_ps == 0 && a.out_nchw && a.Cout <= 16 &&
         a.W >= 256 && a.W % 32 == 0 && (a.Cin == 64 || a.Cin == 128 || a.Cin == 256) && !a.gate && !a.res && !a.res2 &&
         !a.aux && !a.colsum && !a.row_scale && !tile_only() && !variant_is(SR_VARIANT_NO_TAIL);
}
FwdKind fwd_kind(const FwdArgs& a, bool bf) {
  if (fwd_use_tail(a, bf)) return FK_TAIL;
  if (fwd_use_lin(a, bf)) return FK_LIN;
  if (fwd_use_band(a, bf) || fwd_use_band_strip(a, bf)) return FK_BAND;
  if (fwd_use_band_sliced(a, bf) || fwd_use_band_strip_sliced(a, bf)) return FK_BANDS;
  // 128 < Cout < 256 from Cin >= 128, K a multiple of 64 (SwinIR-M's 180 -> 180 convs with the GEMM K padded
  // to 192 on the host, ops/conv.py _kpad): the halo-row 256x256 kernel with a partial output tile rather
  // than the 64-channel halo kernel (SR_VARIANT_NO_BIG_PARTIAL: the halo kernel, A/B and tests)
  if (bf && a.Cout > 128 && a.Cout < 256 && a.Cin >= 128 && !a.out_nchw && a.out_ps == 0 && !a.colsum &&
      !a.dot && fwd_use_pph(a) && !tile_only() && !variant_is(SR_VARIANT_NO_BIG_PARTIAL))
    return FK_BIG;
  if (fwd_use_halo(a, bf)) return FK_HALO;
  // 1x1 convs with K > 192 (SwinIR fc2 fwd, qkv / fc1 dgrads: K 368 / 576 -> 184) on the 256x256
  // kernel with a partial N tile: x read once (vs twice by 128x128 tiles); 68 -> 57 us and 82 -> 65 us
  const bool lin_big = a.tap0 == 4 && a.Cin > 192 && a.Cout >= 128;
  if (bf && !a.out_nchw && (a.Cout >= 256 || lin_big) && a.in_up == 1 && !tile_only()) return FK_BIG;
  if (a.out_nchw || a.Cout <= 16) return FK_256_16;
  if (a.Cout <= 32) return FK_256_32;
  if (a.Cout <= 64) return FK_128_64;
  return FK_128_128;
}
// Rows per epilogue chunk and threads per block of each family: colsum has
// M / rows * threads / 64 partial rows.
void fwd_epi_geom(FwdKind k, int* rows, int* nt) {
  *rows = (k == FK_256_16 || k == FK_256_32) ? 256 : 128;
  *nt = k == FK_BIG ? 512 : 256;
}

// waves per band block: 8 at W 128, 4 at W 64.  With channel sums
// at Cout 32, 4: the partial rows per image (H x pixel waves) then match the tile and halo
// epilogues' (H W / 128 x 4), so the count does not depend on which of them a call lands on.
// Band-reduced channel sums: when the band grid splits the rows evenly and a band never crosses an
// image (rows per band divides H), each band leaves one partial row per pixel wave instead of one per
// row -- RCAN B 32: 16 instead of 128 partial rows per image, the count the standalone partials pass
// (sr_channel_partials) gives, so the channel-attention kernels that sum them stage 8x less.  Returns
// the rows per band, 0 when the sums stay per row.  SR_VARIANT_BAND_CS_ROWS: per-row sums (tests).
int band_cs_rows(const FwdArgs& a) {
  const int T = a.N * a.H, G = band_grid(T);
  if (variant_is(SR_VARIANT_BAND_CS_ROWS) || T % G || a.H % (T / G) || T / G < 2) return 0;
  return T / G;
}
int band_nwv(const FwdArgs& a) {
  return a.W == 128 && !(a.Cout == 32 && (a.colsum || a.dot)) ? 8 : 4;
}

hipError_t dispatch_fwd(const FwdArgs& a, bool bf, hipStream_t s) {
  const FwdKind k = fwd_kind(a, bf);
  switch (k) {
case FK_LIN: return launch_lin(a, s);
case FK_BAND: return launch_band(a, s);
case FK_BANDS: {
  // 64-channel output column slices (the last may be 32 wide), each a band launch with the
  // weight rows, bias, output / residual / gate columns and the gate / residual column
  // ranges shifted to the slice
  for (int n0 = 0; n0 < a.Cout; n0 += 64) {
    FwdArgs b = a;
    const int cw = a.Cout - n0 < 64 ? a.Cout - n0 : 64;
    b.Cout = b.Cout_real = cw;
    b.w = (const bf16_t*)a.w + (size_t)n0 * a.ldw;
    b.w_bytes = a.w_bytes - (uint32_t)((size_t)n0 * a.ldw * 2);
    if (a.bias) b.bias = a.bias + n0;
    b.ycoff = a.ycoff + n0;
    b.gcoff = a.gcoff + n0;
    b.rcoff = a.rcoff + n0;
    b.r2coff = a.r2coff + n0;
    b.gcol0 = a.gcol0 - n0;
    b.gcol1 = a.gcol1 - n0;
    b.rcols = a.rcols - n0;
    const hipError_t e = launch_band(b, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
case FK_TAIL: return launch_fwd_tail(a, s);
case FK_HALO: return launch_fwd_halo(a, s);
case FK_BIG: return launch_fwd_big(a, s);
default: return launch_fwd_tile(a, k, bf, s);
  }
}

inline int tile_for(int c) { return c <= 16 ? 16 : c <= 32 ? 32 : c <= 64 ? 64 : 128; }
// wgrad tile (co x ci): grow the larger side until 4 waves each own a 16x16 sub-tile.
void wg_tiles(int cout, int cin, int* bm, int* bn) {
  int m = tile_for(cout), n = tile_for(cin);
  while ((m / 16) * (n / 16) < 4) {
    if (m <= n) n *= 2; else m *= 2;
  }
  *bm = m;
  *bn = n;
}

// Weight gradients with >= 128 channels each side that are not multiples of 128 (SwinIR linears
// 184 / 368 / 576, its 184-channel 3x3 convs): the 256x256 phase-interleaved kernel with partial
// tiles (columns past Cout / Cin read neighbouring data that only feeds the discarded rows /
// columns of the tile) -- far fewer operand re-reads than 128x128 tiles.
bool wg_use_pp_partial(const sr_conv3x3_wgrad_desc* d) {
  return d->dtype == SR_BF16 && d->Cout >= 128 && d->Cin >= 128 && d->W % 64 == 0 &&
         d->in_up <= 1 && d->out_ps == 0 && !tile_only() && !variant_is(SR_VARIANT_TWO_BARRIER) &&
         !variant_is(SR_VARIANT_WG_NO_PARTIAL);
}

bool wg_use_big(const sr_conv3x3_wgrad_desc* d) {
  return (d->dtype == SR_BF16 && d->Cout >= 256 && d->Cin >= 256 && d->in_up <= 1 && !tile_only()) ||
         wg_use_pp_partial(d);
}

// Phase-interleaved wgrad kernel: W a multiple of 64, channel counts (and the pixel-shuffle
// slot width) multiples of 128.
bool wg_use_pp(const sr_conv3x3_wgrad_desc* d) {
  if (!wg_use_big(d) || variant_is(SR_VARIANT_TWO_BARRIER)) return false;
  if (wg_use_pp_partial(d)) return true;
  const int cps = d->out_ps > 0 ? d->Cout / (d->out_ps * d->out_ps) : 128;
  return d->W % 64 == 0 && d->Cout % 128 == 0 && d->Cin % 128 == 0 && cps % 128 == 0;
}

// Splits per bias-role block of the pp kernel (0: one bias block per split, interleaved with the
// tile blocks).  The bias role reads dy only, so a third of the CUs' worth of bias blocks can take
// three splits each and the tile blocks get more, shorter splits (EDSR-L body wgrad, 247 blocks:
// 176 -> 170 us).  3x3 convs only (the SwinIR linears' slabs are HBM traffic: more splits cost
// there).  (Groups of 2 and the interleaved layout were variants 51 / 53 until round 6.)
int wg_bias_group(const sr_conv3x3_wgrad_desc* d) {
  if (d->ksize == 1 || !wg_use_pp(d)) return 0;
  return 3;
}

// The pp kernel's bias gradient inside its centre-tap blocks: no bias-role blocks, so one 256-block
// wave holds floor(256 / tiles) splits.  Taken for Cout > 256 (the EDSR upsample convs, 36 tiles:
// 6 -> 7 splits, 677 -> 650 us at 64^2, 2614 -> 2517 us at 128^2); at one co tile the centre-tap
// blocks' extra MFMAs cost more than the split gained (EDSR body 170 -> 177 us, SwinIR 3x3 161 ->
// 173 us), so those keep the grouped bias blocks.
bool wg_bias_fused(const sr_conv3x3_wgrad_desc* d) {
  if (d->ksize == 1 || !wg_use_pp(d)) return false;
  return d->Cout > 256;
}

// Row-streaming wgrad over 64-channel output tiles of a wider conv (Cout above 64, the last tile
// partial): a block is (split, co tile, 64-ci chunk); at 80 KB of LDS two blocks share a CU, so the
// plan targets 512 blocks.  Taken where the 256x256 pp kernel is not at home -- channel counts that
// are not multiples of 128 (SwinIR's 184-channel convs: 164 -> 116 us at B 32, 64^2) or Cin < 128
// (the head convs); on the EDSR-L body shape it ties the pp kernel (193 vs 189 us; 256 blocks 256 us,
// 3 / 4 steps in flight 250-280 us: LDS for one block per CU), which stays there.
// knob SR_RING_WIDE: 0 = off, > 0 = on for every Cout > 64 shape with that block target (A/B);
// SR_VARIANT_RING_WIDE_ALL: on everywhere (parity tests).
int ring_wide_env() {
  const int x = sr_knob(K_RING_WIDE);
  return x >= -1 && x <= 4096 ? x : -1;
}
int ring_wide_target() {
  if (variant_is(SR_VARIANT_RING_WIDE_ALL)) return 512;
  const int v = ring_wide_env();
  return v < 0 ? 512 : v;
}
bool wg_ring_wide(const sr_conv3x3_wgrad_desc* d) {
  if (ring_wide_target() <= 0 || tile_only() || d->dtype != SR_BF16 || d->ksize == 1 || d->Cout <= 64 ||
      d->W % 64 || d->in_up > 2)
    return false;
  // pixel-shuffled dy: each 64-wide co tile inside one shuffle slot; SR_VARIANT_RING_NO_PS / knob SR_RING_PS=0: off (A/B)
  const bool ps_off = sr_knob(K_RING_PS) == 0 || variant_is(SR_VARIANT_RING_NO_PS);
  if (d->out_ps > 0 && (d->in_up > 1 || (d->Cout / (d->out_ps * d->out_ps)) % 64 != 0 || ps_off)) return false;
  if (variant_is(SR_VARIANT_RING_WIDE_ALL) || ring_wide_env() > 0) return true;
  return d->Cout % 128 != 0 || d->Cin % 128 != 0;
}
// Kernel-row wgrad (conv3x3_wgrad_row3_kernel): bf16 3x3, Cout % 256, Cin % 128, W % 64, no upsample,
// pixel-shuffled dy when a 256-co tile lies in one shuffle slot (the EDSR-L body and upsample convs).  Knob
// SR_WG_ROW3=0 or SR_VARIANT_NO_ROW3: the pp kernel (A/B, parity cross-check); SR_WG_ROW3=k > 0: bias-role
// blocks of k splits (default 2).
int wg_row3_bg() {
  const int k = sr_knob(K_WG_ROW3);
  return k > 0 && k <= 64 ? k : 2;
}
bool wg_use_row3(const sr_conv3x3_wgrad_desc* d) {
  if (sr_knob(K_WG_ROW3) == 0 || tile_only() || variant_is(SR_VARIANT_TWO_BARRIER) ||
      variant_is(SR_VARIANT_WG_NO_PARTIAL) || variant_is(SR_VARIANT_RING_WIDE_ALL) || variant_is(SR_VARIANT_NO_ROW3))
    return false;
  const bool ps_ok = d->out_ps == 0 || (d->Cout / (d->out_ps * d->out_ps)) % 256 == 0;  // a co tile in one slot
  return d->dtype == SR_BF16 && d->ksize != 1 && d->Cout % 256 == 0 && d->Cin % 128 == 0 && d->W % 64 == 0 &&
         ps_ok && d->in_up <= 1 && ring_wide_env() <= 0;
}
// 1x1 weight gradient on linear_wgrad_kernel (192x192 tiles): bf16 dense token rows, no pixel
// shuffle / upsample.  Knob SR_LWG=0 or SR_VARIANT_NO_LINEAR_WGRAD: off (the pp kernel, A/B and tests).
bool wg_use_lin(const sr_conv3x3_wgrad_desc* d) {
  const bool off = sr_knob(K_LWG) == 0 || variant_is(SR_VARIANT_NO_LINEAR_WGRAD);
  return !off && !tile_only() && d->dtype == SR_BF16 && d->ksize == 1 && d->in_up <= 1 &&
         d->out_ps == 0 && d->Cout >= 64 && d->Cin >= 64;
}
// Block target of its split plan: 128 (half the chip: it runs on the weight-gradient side stream beside
// the main stream, and half the splits halve its slab; SwinIR 35.74 -> 34.71 ms against 256, 160 / 96 / 64
// slower, round 5), or knob SR_LWG_T (A/B)
int lin_wg_target() {
  const int x = sr_knob(K_LWG_T);
  return x >= 16 && x <= 4096 ? x : 128;
}
// Row-streaming wgrad (conv3x3_wgrad_ring_kernel): bf16 3x3, Cout <= 64, W % 64 == 0, nearest upsample
// <= 2 (or over 64-channel output tiles, wg_ring_wide).
bool wg_use_halo(const sr_conv3x3_wgrad_desc* d) {
  if (wg_ring_wide(d)) return true;
  return d->dtype == SR_BF16 && d->ksize != 1 && d->Cout <= 64 && d->W % 64 == 0 && d->in_up <= 2 && d->out_ps == 0 &&
         !tile_only();
}

// Block target of the narrow ring wgrad split plan: 512, or knob SR_RING_SPLITS (A/B sweeps)
int ring_split_target() {
  const int x = sr_knob(K_RING_SPLITS);
  return x >= 16 && x <= 4096 ? x : 512;
}
// 16-channel co tiles per wave of the ring wgrad and its output-channel tiles
int ring_ct(const sr_conv3x3_wgrad_desc* d) { return wg_ring_wide(d) ? 4 : (d->Cout + 15) / 16; }
int ring_tiles_co(const sr_conv3x3_wgrad_desc* d) { return wg_ring_wide(d) ? (d->Cout + 63) / 64 : 1; }

// Split-K factor: enough blocks to cover the chip (~1 round of 256 one-per-CU blocks for the
// 256x256 kernel, ~2 rounds for the small ones), pixels per split a multiple of 64.
// S clamped to [1, maxS], pixels per split = ceil(M / S) rounded up to 64, splits = the ranges that leaves
void plan_splits(int M, int S, int maxS, int* splits, int* kper) {
  if (S > maxS) S = maxS;
  if (S < 1) S = 1;
  const int kp = ((M + S - 1) / S + 63) / 64 * 64;
  *splits = (M + kp - 1) / kp;
  *kper = kp;
}
// Most splits S of one 256-block wave: S x ntile tile blocks + ceil(S / bg) x tco bias-role blocks
int one_wave_splits(int ntile, int tco, int bg) {
  int S = (int)(256.0 / (ntile + (double)tco / bg));
  while (S > 1 && S * ntile + (S + bg - 1) / bg * tco > 256) --S;
  return S;
}
void wgrad_plan(const sr_conv3x3_wgrad_desc* d, int* splits, int* kper) {
  const int M = d->N * d->H * d->W;
  if (wg_use_halo(d)) {
    // ~2 blocks per CU, but at least 8 K-steps per block (the slab costs 8 B per tap-MAC row)
    // (A/B on RCAN / RRDB: twice or half as many splits are 6-12 % slower per step)
    const int chunks = (d->Cin + 63) / 64;
    int S = (wg_ring_wide(d) ? ring_wide_target() : ring_split_target()) / (chunks * ring_tiles_co(d));
    const int maxS = M / 512 > 1 ? M / 512 : 1;
    if (S > maxS) S = maxS;
    if (S < 1) S = 1;
    // whole image rows per split
    const int rows = d->N * d->H;
    const int rps = (rows + S - 1) / S;
    *splits = (rows + rps - 1) / rps;
    *kper = rps * d->W;
    return;
  }
  const int tco = (d->Cout + 255) / 256, tci = (d->Cin + 255) / 256;  // 256x256 tiles
  if (wg_use_lin(d)) {
    const int tiles = ((d->Cout + 191) / 192) * ((d->Cin + 191) / 192);
    return plan_splits(M, lin_wg_target() / tiles, (M + 63) / 64, splits, kper);
  }
  if (wg_use_row3(d))  // 256 x 128 tiles, one kernel row (3 taps) per block
    return plan_splits(M, one_wave_splits(3 * (d->Cout / 256) * (d->Cin / 128), d->Cout / 256, wg_row3_bg()), M / 64,
                       splits, kper);
  if (wg_bias_fused(d)) return plan_splits(M, 256 / (9 * tco * tci), (M + 255) / 256, splits, kper);
  if (wg_bias_group(d) > 0)  // pp kernel, bias-role blocks grouped (see conv3x3_wgrad_pp_kernel)
    return plan_splits(M, one_wave_splits(9 * tco * tci, tco, wg_bias_group(d)), (M + 255) / 256, splits, kper);
  const int taps = d->ksize == 1 ? 1 : 9;
  int S;
  if (wg_use_big(d)) {  // ~1 round of 256 blocks (512: 40.2 -> 41.7 ms EDSR step, round 2), a bias-role block per co tile
    S = 256 / (taps * tco * tci + tco);
  } else {
    int bm, bn;
    wg_tiles(d->Cout, d->Cin, &bm, &bn);
    const int tiles = taps * ((d->Cout + bm - 1) / bm) * ((d->Cin + bn - 1) / bn);
    S = (1024 + tiles / 2) / tiles;
  }
  plan_splits(M, S, (M + 255) / 256, splits, kper);  // at least 256 pixels per split
}

// Paired kernel-row wgrad (sr_conv3x3_wgrad_pair): the two convs of a residual block, one geometry, in one
// launch.  One 256-block wave then holds both problems' tiles, so each gets half the splits of its own launch
// (EDSR-L body: 20 instead of 39): the DMA prologue and the slab store are paid once per ~103 K-steps instead
// of ~52, the slab and its reduce traffic halve, and one reduce launch serves both.  Knob SR_WG_PAIR=0: off
// (sr_conv3x3_wgrad_pair_ok answers 0; A/B and tests); k > 0: bias-role blocks of k splits (default 3: S 20
// in 254 blocks; 2 gives S 19 in 248 and measured 0.24 ms slower per EDSR step, DESIGN note 40).  The plan is a
// function of the descriptor and the knobs alone.
int wg_pair_bg() {
  const int k = sr_knob(K_WG_PAIR);
  return k > 0 && k <= 64 ? k : 3;
}
bool wg_pair_ok(const sr_conv3x3_wgrad_desc* d) {
  if (!d || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cin <= 0 || d->Cout <= 0) return false;
  if (sr_knob(K_WG_PAIR) == 0 || !wg_use_row3(d) || d->out_ps != 0) return false;
  if (d->ldx % 8 || d->ldy % 8 || d->xcoff % 8 || d->ycoff % 8) return false;
  const int cin_real = d->Cin_real > 0 ? d->Cin_real : d->Cin;
  if (cin_real % 4) return false;  // the grouped slab reduce
  const int tco = d->Cout / 256;
  return 3 * tco * (d->Cin / 128) + tco <= 128;  // one split of both problems within one 256-block wave
}
// Largest S with 2 S ntile + 2 ceil(S / bg) tco <= 256, then whole 64-pixel steps per split as plan_splits
void wgrad_pair_plan(const sr_conv3x3_wgrad_desc* d, int* splits, int* kper, int* blocks) {
  const int M = d->N * d->H * d->W, tco = d->Cout / 256, ntile = 3 * tco * (d->Cin / 128), bg = wg_pair_bg();
  int S = 128 / ntile;
  while (S > 1 && S * ntile + (S + bg - 1) / bg * tco > 128) --S;
  plan_splits(M, S, M / 64, splits, kper);
  *blocks = 2 * (*splits * ntile + (*splits + bg - 1) / bg * tco);
}

// Shape / flag fields of FwdArgs from a descriptor (no pointers; validated by the caller).
FwdArgs fwd_shape(const sr_conv3x3_desc* d) {
  const int SZ = d->dtype == SR_BF16 ? 2 : 4;
  const int PER = 16 / SZ;
  const int taps = d->ksize == 1 ? 1 : 9;
  FwdArgs a{};
  a.N = d->N; a.H = d->H; a.W = d->W; a.M = d->N * d->H * d->W;
  a.Cin = d->Cin; a.ldx = d->ldx; a.xcoff = d->xcoff; a.in_ps = d->in_ps;
  a.cpt = d->Cin / PER; a.nkc = taps * a.cpt;
  a.tap0 = taps == 1 ? 4 : 0;
  a.gate_mode = d->gate_mode;
  a.gcol0 = d->gcol0; a.gcol1 = d->gcol1;
  a.Cout = d->Cout; a.Cout_real = d->Cout_real > 0 ? d->Cout_real : d->Cout; a.ldw = d->ldw;
  a.ldy = d->ldy; a.ycoff = d->ycoff; a.out_ps = d->out_ps; a.out_nchw = d->out_nchw;
  a.act = d->act; a.slope = d->slope; a.alpha = d->alpha;
  a.ldg = d->ldg; a.gcoff = d->gcoff; a.gate_slope = d->gate_slope;
  a.ldr = d->ldr; a.rcoff = d->rcoff; a.beta = d->beta;
  a.ldr2 = d->ldr2; a.r2coff = d->r2coff; a.beta2 = d->beta2;
  a.rcols = d->rcols > 0 ? d->rcols : d->Cout;
  a.in_up = d->in_up > 1 ? d->in_up : 1;
  a.fd_cpt = make_fastdiv(a.cpt > 0 ? a.cpt : 1);
  a.fd_W = make_fastdiv(d->W > 0 ? d->W : 1);
  a.fd_H = make_fastdiv(d->H > 0 ? d->H : 1);
  int cps = 1;
  if (d->in_ps > 0) cps = d->Cin / (d->in_ps * d->in_ps);
  if (d->out_ps > 0) cps = d->Cout / (d->out_ps * d->out_ps);
  a.fd_cps = make_fastdiv(cps > 0 ? cps : 1);
  a.fd_r = make_fastdiv(d->in_ps > 0 ? d->in_ps : 1);
  a.row_scale = d->row_scale;
  a.fd_hw = make_fastdiv(d->H * d->W > 0 ? d->H * d->W : 1);
  a.dot = d->dot; a.ldd = d->ldd; a.dcoff = d->dcoff;
  if (d->dot) {  // the dot epilogue comes with a residual: the pointer-free kind / parts / name queries
    static const char one = 1;  // see the launch's epilogue code (sr_conv3x3_fwd sets the real res)
    a.res = &one;
  }
  return a;
}

// Partial rows per image of the colsum output, or 0 when the call cannot produce it.
int colsum_parts(const sr_conv3x3_desc* d, const FwdArgs& a0) {
  static float one;
  FwdArgs a = a0;
  a.colsum = &one;  // the kernel choice of a call that asks for the sums
  const FwdKind k = fwd_kind(a, d->dtype == SR_BF16);
  if (d->out_ps || d->out_nchw || k == FK_LIN) return 0;
  if (k == FK_BAND) {  // (rows or bands) x pixel waves
    const int rpb = band_cs_rows(a);
    return (rpb ? d->H / rpb : d->H) * (band_nwv(a) / (d->Cout / 32));
  }
  int rows, nt;
  fwd_epi_geom(k, &rows, &nt);
  const int HW = d->H * d->W;
  if (HW % rows) return 0;
  return HW / rows * (nt / 64);
}
}  // namespace sr_conv

extern "C" {

int sr_conv3x3_fwd(const sr_conv3x3_desc* d, const void* x, const void* w, const float* bias,
                   const void* gate, const void* res, const void* res2, const float* aff_scale,
                   const float* aff_shift, void* y, void* aux, float* colsum, void* stream) {
  if (!d || !x || !w || !y) return sr_fail(SR_EINVAL, "conv3x3_fwd: null pointer");
  const int SZ = d->dtype == SR_BF16 ? 2 : 4;
  const int PER = 16 / SZ;
  if (d->Cin % 8 || d->ldx % PER || d->xcoff % PER || (!d->out_nchw && (d->Cout % 8)))
    return sr_fail(SR_EINVAL, "conv3x3_fwd: Cin/Cout/ld/coff must be multiples of 8 (pad channels)");
  const int taps = d->ksize == 1 ? 1 : 9;
  if (d->ksize != 0 && d->ksize != 1 && d->ksize != 3) return sr_fail(SR_EINVAL, "conv3x3_fwd: ksize must be 1 or 3");
  if (d->ldw < taps * d->Cin) return sr_fail(SR_EINVAL, "conv3x3_fwd: ldw < taps*Cin");
  if (aux && (d->out_ps || d->out_nchw)) return sr_fail(SR_EINVAL, "conv3x3_fwd: aux needs plain store");
  if ((gate || res || res2) && d->out_ps) return sr_fail(SR_EINVAL, "conv3x3_fwd: gate/res need plain store");
  const int up = d->in_up > 1 ? d->in_up : 1;
  if (up > 1 && (d->in_ps > 0 || d->H % up || d->W % up))
    return sr_fail(SR_EINVAL, "conv3x3_fwd: in_up needs H, W divisible by it and no in_ps");
  if (d->in_ps > 0 && d->out_ps > 0) return sr_fail(SR_EINVAL, "conv3x3_fwd: in_ps and out_ps exclusive");
  if (d->in_ps > 0 && (d->Cin / (d->in_ps * d->in_ps)) % PER)
    return sr_fail(SR_EINVAL, "conv3x3_fwd: shuffled channel count must be a multiple of 8");
  if (d->out_ps > 0 && (d->Cout / (d->out_ps * d->out_ps)) % PER)
    return sr_fail(SR_EINVAL, "conv3x3_fwd: shuffled channel count must be a multiple of 8");
  FwdArgs a = fwd_shape(d);
  if (colsum && colsum_parts(d, a) == 0)
    return sr_fail(SR_EINVAL, "conv3x3_fwd: colsum needs a plain store and H*W a multiple of the epilogue rows");
  const int M = a.M;
  const int r_in = d->in_ps > 0 ? d->in_ps : 1;
  const size_t xb = (size_t)M * r_in * r_in * (size_t)d->ldx * SZ / ((size_t)up * up);
  const size_t wb = (size_t)d->Cout * d->ldw * SZ;
  if (xb >= 0x80000000ull || wb >= 0x80000000ull)
    return sr_fail(SR_ETOOBIG, "conv3x3_fwd: tensor >= 2 GiB (split the batch)");
  a.x = x; a.w = w; a.bias = bias; a.gate = gate; a.res = res; a.res2 = res2;
  a.aff_scale = aff_scale; a.aff_shift = aff_shift; a.y = y; a.aux = aux; a.colsum = colsum;
  if (d->dot) {  // with every operand pointer set: the band kernel's epilogue code decides
    if (!colsum || !res || d->dtype != SR_BF16 || fwd_kind(a, true) != FK_BAND || d->ldd % 8 || d->dcoff % 8)
      return sr_fail(SR_EINVAL, "conv3x3_fwd: dot partials need colsum on the band kernel (bf16, 64 -> 64 ch)");
    const size_t db = (size_t)d->N * d->H * d->W * d->ldd * 2;
    if (db >= 0x80000000ull) return sr_fail(SR_ETOOBIG, "conv3x3_fwd: dot operand >= 2 GiB");
    a.d_bytes = (uint32_t)db;
  }
  a.x_bytes = (uint32_t)xb; a.w_bytes = (uint32_t)wb;
  a.g_bytes = gate ? (uint32_t)((size_t)M * d->ldg * SZ) : 0;
  a.r_bytes = res ? (uint32_t)((size_t)M * d->ldr * SZ) : 0;
  a.r2_bytes = res2 ? (uint32_t)((size_t)M * d->ldr2 * SZ) : 0;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = dispatch_fwd(a, d->dtype == SR_BF16, s);
  return sr_check(e, "conv3x3_fwd launch");
}

int sr_linear_ln_fwd(const sr_conv3x3_desc* d, const void* x, const float* ln_gamma, const float* ln_beta, int ln_C,
                     float eps, void* ln_out, float* ln_mean, float* ln_rstd, const void* w, const float* bias, void* y,
                     void* aux, void* stream) {
  if (!d || !x || !ln_gamma || !ln_beta || !ln_out || !ln_mean || !ln_rstd || !w || !y)
    return sr_fail(SR_EINVAL, "linear_ln_fwd: null pointer");
  if (d->dtype != SR_BF16 || d->ksize != 1 || d->Cin % 8 || d->Cout % 8 || d->ldx != d->Cin || d->xcoff != 0 ||
      ln_C <= 0 || ln_C > d->Cin || d->ldw < d->Cin)
    return sr_fail(SR_EINVAL, "linear_ln_fwd: bf16 1x1 conv over dense rows (ldx == Cin) with ln_C <= Cin");
  FwdArgs a = fwd_shape(d);
  if (!fwd_use_lin(a, true) || a.Cin > 192)
    return sr_fail(SR_EINVAL, "linear_ln_fwd: shape not on the lin kernel (Cin <= 192, Cout <= 640)");
  a.aux = aux;
  const int e = lin_epi(a);
  if (e != 0 && e != 67) return sr_fail(SR_EINVAL, "linear_ln_fwd: epilogue must be plain or GELU + pre-activation aux");
  const size_t xb = (size_t)a.M * d->ldx * 2, wb = (size_t)d->Cout * d->ldw * 2;
  if (xb >= 0x80000000ull || wb >= 0x80000000ull) return sr_fail(SR_ETOOBIG, "linear_ln_fwd: tensor >= 2 GiB");
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.x_bytes = (uint32_t)xb; a.w_bytes = (uint32_t)wb;
  a.ln_g = ln_gamma; a.ln_b = ln_beta; a.ln_out = ln_out; a.ln_mean = ln_mean; a.ln_rstd = ln_rstd;
  a.ln_C = ln_C; a.ln_eps = eps;
  a.tiles = (a.M + 127) / 128;
  hipStream_t s = (hipStream_t)stream;
  return launch_lin_ln(a, e, s);
}

// 1 when sr_conv3x3_fwd can fuse the dot partials (d->dot) into this conv with a residual operand:
// the band kernel's residual + colsum + dot epilogue (RCAB conv1 dgrad shapes).
int sr_conv3x3_fwd_dot_ok(const sr_conv3x3_desc* d) {
  if (!d || d->N <= 0 || d->H <= 0 || d->W <= 0 || d->dtype != SR_BF16) return 0;
  FwdArgs a = fwd_shape(d);
  static const char one = 1;
  a.res = &one;
  a.dot = &one;
  a.colsum = (float*)&one;
  sr_conv3x3_desc dd = *d;
  dd.dot = &one;
  return fwd_kind(a, true) == FK_BAND && colsum_parts(&dd, a) > 0 ? 1 : 0;
}

int sr_conv3x3_fwd_colsum_parts(const sr_conv3x3_desc* d) {
  if (!d || d->N <= 0 || d->H <= 0 || d->W <= 0) return 0;
  return colsum_parts(d, fwd_shape(d));
}

// Name of the kernel instantiation sr_conv3x3_fwd / sr_conv3x3_wgrad will launch for a
// descriptor (bench.py traces and rocprof summaries are matched on these names).
const char* sr_conv3x3_fwd_kernel_name(const sr_conv3x3_desc* d) {
  const bool bf = d->dtype == SR_BF16;
  const FwdArgs a = fwd_shape(d);
  switch (fwd_kind(a, bf)) {
    case FK_LIN: return lin_use_wk(a) ? "linear_wk_kernel" : "conv3x3_lin_kernel";
    case FK_HALO: return "conv3x3_fwd_halo_kernel";
    case FK_BAND: return "conv3x3_fwd_band_kernel";
    case FK_TAIL: return "conv3x3_fwd_tail_kernel";
    case FK_BANDS: return "conv3x3_fwd_band_kernel";
    case FK_BIG: {
      if (variant_is(SR_VARIANT_TWO_BARRIER)) return "conv3x3_fwd_big_kernel";
      return fwd_use_pph(a) || fwd_use_pph_strip(a) ? "conv3x3_fwd_pph_kernel" : "conv3x3_fwd_pp_kernel";
    }
    case FK_256_16: return bf ? "conv3x3_fwd_kernel<bf16,256,16>" : "conv3x3_fwd_kernel<f32,256,16>";
    case FK_256_32: return bf ? "conv3x3_fwd_kernel<bf16,256,32>" : "conv3x3_fwd_kernel<f32,256,32>";
    case FK_128_64: return bf ? "conv3x3_fwd_kernel<bf16,128,64>" : "conv3x3_fwd_kernel<f32,128,64>";
    default: return bf ? "conv3x3_fwd_kernel<bf16,128,128>" : "conv3x3_fwd_kernel<f32,128,128>";
  }
}

int sr_conv3x3_fwd_launches(const sr_conv3x3_desc* d) {
  if (!d) return 0;
  const FwdArgs a = fwd_shape(d);
  return fwd_kind(a, d->dtype == SR_BF16) == FK_BANDS ? (a.Cout + 63) / 64 : 1;
}

const char* sr_conv3x3_wgrad_kernel_name(const sr_conv3x3_wgrad_desc* d) {
  if (wg_use_halo(d)) return "conv3x3_wgrad_ring_kernel";
  if (wg_use_lin(d)) return "linear_wgrad_kernel";
  if (wg_use_row3(d)) return "conv3x3_wgrad_row3_kernel";
  if (wg_use_pp(d)) return "conv3x3_wgrad_pp_kernel";
  if (wg_use_big(d)) return "conv3x3_wgrad_big_kernel";
  return d->dtype == SR_BF16 ? "conv3x3_wgrad_kernel<bf16>" : "conv3x3_wgrad_kernel<f32>";
}

// Kernel-variant switch for the parity tests' cross-checks: an sr_conv_variant (include/sr_hip.h lists them, each
// with the family it routes back to the kernel it replaced).  The measured-slower paths and the timing ablations
// were removed in round 6 (git history).
int sr_conv3x3_set_variant(int variant) {
  bool ok = false;
#define SR_VARIANT_OK(name, value) ok = ok || variant == name;
  SR_CONV_VARIANTS(SR_VARIANT_OK)
#undef SR_VARIANT_OK
  if (!ok) return sr_fail(SR_EINVAL, "conv3x3_set_variant: not a parity cross-check variant");
  g_variant = variant;
  return SR_OK;
}

int sr_conv3x3_get_variant(void) { return g_variant; }

// Diagnostics: the band kernel writes 16 clock values per block (wave 0: start, weights loaded,
// end, rows, cycles summed over rows in the row wait / barrier / MFMA / epilogue phases, then
// LDS zeroed, weight loads issued) into buf while it is set; null turns it off.
int sr_conv3x3_set_stamps(void* buf) {
  g_sr_stamps = (unsigned long long*)buf;
  return SR_OK;
}

size_t sr_conv3x3_wgrad_workspace(const sr_conv3x3_wgrad_desc* d) {
  int S, kp;
  wgrad_plan(d, &S, &kp);
  const int taps = d->ksize == 1 ? 1 : 9;
  return ((size_t)S * taps * d->Cout * d->Cin + (size_t)S * d->Cout) * sizeof(float) + 256;
}

int sr_conv3x3_wgrad(const sr_conv3x3_wgrad_desc* d, const void* dy, const void* x, void* workspace,
                     size_t ws_bytes, float* dw, float* db, const int* co_map, const int* ci_map, void* stream) {
  if (!d || !dy || !x || !workspace || !dw) return sr_fail(SR_EINVAL, "conv3x3_wgrad: null pointer");
  const int SZ = d->dtype == SR_BF16 ? 2 : 4;
  const int PER = 16 / SZ;
  if (d->Cin % 8 || d->Cout % 8 || d->ldx % PER || d->ldy % PER || d->xcoff % PER || d->ycoff % PER)
    return sr_fail(SR_EINVAL, "conv3x3_wgrad: channel counts / strides must be multiples of 8");
  if (ws_bytes < sr_conv3x3_wgrad_workspace(d)) return sr_fail(SR_EINVAL, "conv3x3_wgrad: workspace too small");
  const int M = d->N * d->H * d->W;
  const int r = d->out_ps > 0 ? d->out_ps : 1;
  const int up = d->in_up > 1 ? d->in_up : 1;
  if (up > 1 && (d->H % up || d->W % up)) return sr_fail(SR_EINVAL, "conv3x3_wgrad: H, W must divide by in_up");
  const size_t xb = (size_t)M * d->ldx * SZ / ((size_t)up * up);
  const size_t dyb2 = (size_t)M * r * r * (size_t)d->ldy * SZ;
  if (xb >= 0x80000000ull || dyb2 >= 0x80000000ull)
    return sr_fail(SR_ETOOBIG, "conv3x3_wgrad: tensor >= 2 GiB (split the batch)");
  WgArgs a{};
  a.dy = dy; a.x = x;
  int S, kp;
  wgrad_plan(d, &S, &kp);
  a.ws = (float*)workspace;
  const int taps = d->ksize == 1 ? 1 : 9;
  a.taps = taps;
  a.tap0 = taps == 1 ? 4 : 0;
  a.wsb = db ? a.ws + (size_t)S * taps * d->Cout * d->Cin : nullptr;
  a.dy_bytes = (uint32_t)dyb2; a.x_bytes = (uint32_t)xb;
  a.N = d->N; a.H = d->H; a.W = d->W; a.M = M;
  a.Cin = d->Cin; a.ldx = d->ldx; a.xcoff = d->xcoff;
  a.Cout = d->Cout; a.ldy = d->ldy; a.ycoff = d->ycoff; a.out_ps = d->out_ps;
  a.in_up = up;
  a.splits = S; a.kper = kp;
  a.fd_W = make_fastdiv(d->W); a.fd_H = make_fastdiv(d->H);
  int cps = d->out_ps > 0 ? d->Cout / (d->out_ps * d->out_ps) : 1;
  if (d->out_ps > 0 && cps % PER)
    return sr_fail(SR_EINVAL, "conv3x3_wgrad: shuffled channel count must be a multiple of 8");
  a.fd_cps = make_fastdiv(cps);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  a.stamps = g_sr_stamps;
  if (wg_use_halo(d)) e = launch_wg_ring(a, d, s);
  else if (wg_use_lin(d)) e = launch_wg_lin(a, s);
  else if (wg_use_row3(d)) e = launch_wg_row3(a, s);
  else if (wg_use_big(d)) e = launch_wg_big(a, d, s);
  else e = launch_wg_tile(a, d->dtype == SR_BF16, s);
  if (e != hipSuccess) return sr_check(e, "conv3x3_wgrad launch");
  if (d->accumulate & 2) return SR_OK;  // bit 1: slab only (sr_conv3x3_wgrad_reduce later, e.g. on another stream)
  return wgrad_reduce_launch(d, S, taps, a.ws, a.wsb, dw, db, co_map, ci_map, s);
}

int sr_conv3x3_wgrad_reduce(const sr_conv3x3_wgrad_desc* d, void* workspace, size_t ws_bytes, float* dw, float* db,
                            const int* co_map, const int* ci_map, void* stream) {
  if (!d || !workspace || !dw) return sr_fail(SR_EINVAL, "conv3x3_wgrad_reduce: null pointer");
  if (ws_bytes < sr_conv3x3_wgrad_workspace(d)) return sr_fail(SR_EINVAL, "conv3x3_wgrad_reduce: workspace too small");
  int S, kp;
  wgrad_plan(d, &S, &kp);
  const int taps = d->ksize == 1 ? 1 : 9;
  float* ws = (float*)workspace;
  float* wsb = db ? ws + (size_t)S * taps * d->Cout * d->Cin : nullptr;
  return wgrad_reduce_launch(d, S, taps, ws, wsb, dw, db, co_map, ci_map, (hipStream_t)stream);
}

int sr_conv3x3_wgrad_pair_ok(const sr_conv3x3_wgrad_desc* d) { return wg_pair_ok(d) ? 1 : 0; }

int sr_conv3x3_wgrad_pair_plan(const sr_conv3x3_wgrad_desc* d, int* splits, int* kper, int* blocks) {
  if (!d || !splits || !kper || !blocks) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair_plan: null pointer");
  if (!wg_pair_ok(d)) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair_plan: descriptor not on the paired kernel-row wgrad");
  wgrad_pair_plan(d, splits, kper, blocks);
  return SR_OK;
}

// two slabs [S][9][Cout][Cin] + [S][Cout], item 1's after item 0's
size_t sr_conv3x3_wgrad_pair_workspace(const sr_conv3x3_wgrad_desc* d) {
  if (!wg_pair_ok(d)) return 0;
  int S, kp, nb;
  wgrad_pair_plan(d, &S, &kp, &nb);
  return 2 * ((size_t)S * 9 * d->Cout * d->Cin + (size_t)S * d->Cout) * sizeof(float) + 256;
}

int sr_conv3x3_wgrad_pair(const sr_conv3x3_wgrad_desc* d, const sr_conv3x3_wgrad_item* items, void* workspace,
                          size_t ws_bytes, void* stream) {
  if (!d || !items || !workspace) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair: null pointer");
  if (!wg_pair_ok(d)) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair: descriptor not on the paired kernel-row wgrad");
  if (d->accumulate & 2) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair: no slab-only form (accumulate bit 1)");
  for (int i = 0; i < 2; ++i)
    if (!items[i].dy || !items[i].x || !items[i].dw) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair: null item pointer");
  if (!items[0].db != !items[1].db) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair: both db or neither");
  if (ws_bytes < sr_conv3x3_wgrad_pair_workspace(d)) return sr_fail(SR_EINVAL, "conv3x3_wgrad_pair: workspace too small");
  const int M = d->N * d->H * d->W;
  const size_t xb = (size_t)M * d->ldx * 2, dyb = (size_t)M * d->ldy * 2;
  if (xb >= 0x80000000ull || dyb >= 0x80000000ull)
    return sr_fail(SR_ETOOBIG, "conv3x3_wgrad_pair: tensor >= 2 GiB (split the batch)");
  int S, kp, nb;
  wgrad_pair_plan(d, &S, &kp, &nb);
  const bool bias = items[0].db != nullptr;
  const size_t slab = (size_t)S * 9 * d->Cout * d->Cin, per = slab + (size_t)S * d->Cout;
  float* ws0 = (float*)workspace;
  float* ws1 = ws0 + per;
  WgArgs a{};
  a.dy = items[0].dy; a.x = items[0].x; a.ws = ws0; a.wsb = bias ? ws0 + slab : nullptr;
  a.dy1 = items[1].dy; a.x1 = items[1].x; a.ws1 = ws1; a.wsb1 = bias ? ws1 + slab : nullptr;
  a.dy_bytes = a.dy1_bytes = (uint32_t)dyb; a.x_bytes = a.x1_bytes = (uint32_t)xb;
  a.taps = 9; a.tap0 = 0;
  a.N = d->N; a.H = d->H; a.W = d->W; a.M = M;
  a.Cin = d->Cin; a.ldx = d->ldx; a.xcoff = d->xcoff;
  a.Cout = d->Cout; a.ldy = d->ldy; a.ycoff = d->ycoff; a.out_ps = 0;
  a.in_up = 1;
  a.splits = S; a.kper = kp;
  a.fd_W = make_fastdiv(d->W); a.fd_H = make_fastdiv(d->H);
  a.fd_cps = make_fastdiv(1);
  a.stamps = g_sr_stamps;
  hipStream_t s = (hipStream_t)stream;
  const hipError_t e = launch_wg_row3_pair(a, wg_pair_bg(), s);
  if (e != hipSuccess) return sr_check(e, "conv3x3_wgrad_pair launch");
  sr_conv3x3_wgrad_desc d0 = *d;
  d0.scale = items[0].scale;
  const WgReduce2 p2{a.ws1, a.wsb1, items[1].dw, items[1].db, items[1].scale};
  return wgrad_reduce_launch(&d0, S, 9, a.ws, a.wsb, items[0].dw, items[0].db, nullptr, nullptr, s, &p2);
}

}  // extern "C"
