// What the conv3x3 translation units share on the host side: the kernel argument structs, the compile-time
// epilogue bits, the forward kernel families, the launchers of the family files and the selection predicates
// of conv3x3.hip that a launcher calls.
#pragma once
#include "sr_common.h"
#include "sr_internal.h"

// hidden visibility: none of these names is part of the library's ABI
namespace sr_conv __attribute__((visibility("hidden"))) {

// Bits of the compile-time epilogue code E of the band, lin and linear_wk kernels (a template argument, so
// the values are part of the kernel names): bits 0-1 act, 2-3 gate (0 none, 1 pre-residual (g > 0 ? 1 :
// gate_slope), 2 pre-residual GELU'(g), 3 post-residual mask on columns gcol0..gcol1), then one bit per operand.
// Bit 7 is the channel sums in the band kernel and the per-image row scale in the lin kernels.
enum : int { EPI_ACT = 3, EPI_GATE_SHIFT = 2, EPI_GATE = 3, EPI_RES = 16, EPI_RES2 = 32, EPI_AUX = 64 };
enum : int { BAND_CS = 128, BAND_RSC = 256, BAND_DOT = 512, BAND_STRIP = 1024 };
enum : int { LIN_RSC = 128 };

struct FwdArgs {
  const void* x;
  const void* w;
  const float* bias;
  const void* gate;
  const void* res;
  const float* aff_scale;
  const float* aff_shift;
  void* y;
  uint32_t x_bytes, w_bytes, g_bytes, r_bytes;
  int N, H, W, M;
  int Cin, ldx, xcoff, in_ps, cpt;  // cpt: 16-byte chunks per tap
  int Cout, Cout_real, ldw, nkc;    // nkc: total K chunks (9*cpt)
  int ldy, ycoff, out_ps, out_nchw;
  int act;
  float slope, alpha;
  int ldg, gcoff;
  float gate_slope;
  int ldr, rcoff;
  float beta;
  const void* res2;
  uint32_t r2_bytes;
  int ldr2, r2coff, rcols;
  float beta2;
  int in_up;  // nearest-neighbour upsample factor folded into the A gather (1 = none)
  int tap0;   // 4 for 1x1 (linear) convs: the single tap is the centre one
  int gate_mode;  // 0: v *= (gate > 0 ? 1 : gate_slope); 1: v *= GELU'(gate); 2: post-residual, gcol0..gcol1
  int gcol0, gcol1;
  void* aux;      // optional store of the pre-activation value (same layout as y)
  float* colsum;  // optional per-(wave, row chunk) column sums of the stored y (see epilogue_tile)
  int tiles_n, tiles;
  FastDiv fd_cpt, fd_W, fd_H, fd_cps;  // fd_cps: divide by C' (channels per shuffle slot)
  FastDiv fd_r;                        // divide by in_ps (1 when none)
  unsigned long long* stamps;  // diagnostics: per-row clock stamps of the band kernel (null = off)
  const float* row_scale;  // optional per-image factor on alpha (SwinIR stochastic depth)
  FastDiv fd_hw;           // divide by H*W (pixel -> image)
  // LayerNorm of the input rows fused into the lin kernel's prologue (sr_linear_ln_fwd)
  const float* ln_g;
  const float* ln_b;
  void* ln_out;  // the normalised rows [M][Cin] (bf16), for the weight gradient and backward
  float* ln_mean;
  float* ln_rstd;
  int ln_C;      // channels normalised (the rest of the Cin padded columns are written as zeros)
  float ln_eps;
  const void* dot;  // band kernel, with colsum: partial sums of y * dot (sr_conv3x3_desc.dot)
  uint32_t d_bytes;
  int ldd, dcoff;
  int cs_band;  // band kernel: colsum / dot partial rows summed over the band's rows (band_cs_rows), 0: per row
  int strip64;  // pph kernel over 64-px column strips of a wider image: 256-row tiles are 4 rows x 64 px
};

// ------------------------------------------------------------------------------------
// Weight gradient.  GEMM per tap: C[co][ci] = sum_p dy[p][co] * x[p + tap][ci] over a
// K-range of pixels (split-K).  LDS images are [pixels][cols] (rows = K); MFMA operands
// need 8 consecutive K per lane, read with ds_read_b64_tr_b16 (bf16) or ds_read_b32
// (f32).  Partial tiles go to an fp32 slab ws[split][tap][co][ci]; blocks of the centre
// tap and first ci tile also emit the bias-gradient partial sums.
// ------------------------------------------------------------------------------------
struct WgArgs {
  const void* dy;
  const void* x;
  float* ws;    // [S][9][Cout][Cin]
  float* wsb;   // [S][Cout]
  uint32_t dy_bytes, x_bytes;
  int N, H, W, M;
  int Cin, ldx, xcoff;
  int Cout, ldy, ycoff, out_ps;
  int in_up;  // nearest upsample factor of the x gather (1 = none)
  int taps, tap0;  // 9 / 0 for 3x3, 1 / 4 for 1x1 (linear)
  int tiles_co, tiles_ci, splits, kper;  // kper: pixels per split (multiple of KSTEP)
  int bias_group;  // pp kernel: > 0 = the bias-role blocks come after all tile blocks, each doing this many splits
  int bias_fused;  // pp kernel: no bias-role blocks; the centre-tap, first-ci-tile blocks sum dy as well
  FastDiv fd_W, fd_H, fd_cps;
  unsigned long long* stamps;  // diagnostics (SR_BAND_STAMPS builds): per-block phase cycles
  // Kernel-row wgrad over TWO problems of one geometry in one grid (sr_conv3x3_wgrad_pair): pair_nt > 0 is
  // the tile-block count of each problem (splits x tiles) and the grid is [tiles 0][tiles 1][bias 0][bias 1];
  // the operands above are problem 0's, these problem 1's.  0: one problem, the fields are unused.
  int pair_nt;
  uint32_t dy1_bytes, x1_bytes;
  const void* dy1;
  const void* x1;
  float* ws1;
  float* wsb1;
};

// Second item of a paired slab reduce (wgrad_reduce_g_kernel, grid y = 1): its slab, outputs and scale.
struct WgReduce2 {
  const float* ws;
  const float* wsb;
  float* dw;
  float* db;
  float scale;
};

// Kernel family sr_conv3x3_fwd launches for a call (dispatch, kernel names and the
// epilogue geometry behind colsum all follow this one choice).
enum FwdKind { FK_HALO, FK_BIG, FK_256_16, FK_256_32, FK_128_64, FK_128_128, FK_LIN, FK_BAND, FK_TAIL, FK_BANDS };

// The variant set by sr_conv3x3_set_variant; conv3x3.hip keeps it.
bool variant_is(int v);
bool tile_only();

// Selection predicates that a launcher calls (all defined in conv3x3.hip).
bool fwd_use_pph_strip(const FwdArgs& a);
bool fwd_use_pph(const FwdArgs& a);
int pph_pers_grid(const FwdArgs& a);
int band_epi(const FwdArgs& a, int grid);
int band_grid(int rows);
int band_cs_rows(const FwdArgs& a);
int band_nwv(const FwdArgs& a);
int lin_epi(const FwdArgs& a);
bool lin_use_wk(const FwdArgs& a);
void wg_tiles(int cout, int cin, int* bm, int* bn);
bool wg_use_halo(const sr_conv3x3_wgrad_desc* d);
bool wg_use_pp(const sr_conv3x3_wgrad_desc* d);
int wg_bias_group(const sr_conv3x3_wgrad_desc* d);
bool wg_bias_fused(const sr_conv3x3_wgrad_desc* d);
int wg_row3_bg();
int ring_ct(const sr_conv3x3_wgrad_desc* d);
int ring_tiles_co(const sr_conv3x3_wgrad_desc* d);

// Launchers, each defined in the file of its kernels.  The weight-gradient launchers take the arguments with the
// split plan filled in (splits, kper, taps) and set the tile counts of their kernel.
hipError_t launch_fwd_tile(const FwdArgs& a, FwdKind k, bool bf16, hipStream_t s);  // conv3x3_fwd_tile.hip
hipError_t launch_fwd_big(const FwdArgs& a0, hipStream_t s);                         // conv3x3_fwd_pp.hip
hipError_t launch_lin(const FwdArgs& a, hipStream_t s);                              // conv3x3_linear.hip
int launch_lin_ln(const FwdArgs& a, int e, hipStream_t s);                           // conv3x3_linear.hip
hipError_t launch_wg_lin(WgArgs a, hipStream_t s);                                   // conv3x3_linear.hip
hipError_t launch_fwd_halo(const FwdArgs& a0, hipStream_t s);                        // conv3x3_fwd_tile.hip
hipError_t launch_band(const FwdArgs& a, hipStream_t s);                             // conv3x3_fwd_band.hip
hipError_t launch_fwd_tail(const FwdArgs& a, hipStream_t s);                         // conv3x3_fwd_tail.hip
hipError_t launch_wg_tile(const WgArgs& a, bool bf16, hipStream_t s);                // conv3x3_wgrad_tile.hip
hipError_t launch_wg_big(WgArgs a, const sr_conv3x3_wgrad_desc* d, hipStream_t s);   // conv3x3_wgrad_tile.hip
hipError_t launch_wg_ring(WgArgs a, const sr_conv3x3_wgrad_desc* d, hipStream_t s);  // conv3x3_wgrad_ring.hip
hipError_t launch_wg_row3(WgArgs a, hipStream_t s);                                  // conv3x3_wgrad_ring.hip
hipError_t launch_wg_row3_pair(WgArgs a, int bias_group, hipStream_t s);             // conv3x3_wgrad_ring.hip
// (second: the other item of a pair, reduced by the same launch with d->scale for the first; no maps)
int wgrad_reduce_launch(const sr_conv3x3_wgrad_desc* d, int S, int taps, const float* ws, const float* wsb, float* dw,
                        float* db, const int* co_map, const int* ci_map, hipStream_t s,
                        const WgReduce2* second = nullptr);  // conv3x3_wgrad_reduce.hip

}  // namespace sr_conv
