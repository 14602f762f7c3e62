// What the deformable-conv translation units share on the host side: the kernel argument struct, the
// geometries that dcn.hip works out and a launcher is given, the tile constants and the launchers of the
// family files.
#pragma once
#include "sr_common.h"
#include "sr_internal.h"

// hidden visibility: none of these names is part of the library's ABI
namespace sr_dcn __attribute__((visibility("hidden"))) {

struct DcnArgs {
  int N, C, H, W, Cp, Ho, Wo;
  int kh, kw, sh, sw, ph, pw, dh, dw;
  int G, DG, cg, cgp, cpg;  // conv groups, deformable groups, channels per conv group (+pad), per deform group
  int K, L, TP;             // taps, column row length (G*K*cgp), pixels per tile
};

// Scatter geometry of dcn_grad_x_kernel (dcn_cols.hip)
struct XGeom {
  int TT, R, RH, RW, CPP;  // output tile edge, halo, footprint rows / cols, channels per pass
};

// Geometry of the fused backward (dcn_bwd_win.hip): the coordinate kernel's window (R1, WH, WW) and the
// scatter kernel's footprint (R2, RH, RW), with the LDS bytes of each.
struct BwdGeom {
  int R1, WH, WW, R2, RH, RW;
  size_t lds1, lds2;
  int fx;   // fixed-point bits of the scatter image (64 / 32)
  int fxe;  // bits of one contribution in it (gx_fx_bits)
};

constexpr int DF_TP = 128, DF_RS = 72;  // fused forward: pixels per block; LDS row stride in bf16 (144 B)
constexpr int DW_TH = 8, DW_TW = 16, DW_NT = 512;  // windowed kernels: output tile, threads
constexpr int DC8_NT = 256;  // dcn_coord_dy8_kernel: 4 waves, an 8 x 16 tile, two rows per wave
constexpr int DX_TT = 16, DX_CPP = 16, DX_ST = DX_CPP + 1;  // tile edge, channels per pass, LDS pixel stride
constexpr int GX_PD = 1;  // taps of operands in flight in the scatter kernel (3: 394 vs 354 us)

// Launchers, each defined in the file of its kernels.  dcn.hip validates the call and works out every geometry;
// a launcher sets the LDS attribute where the kernel needs more than 64 KB, launches, and returns the status.
int launch_im2col(const DcnArgs& a, bool bf16, const void* x, const float* off, const float* msk, void* cols,
                  hipStream_t s);  // dcn_cols.hip
// (coord = false: the coordinate pass, and amax, ran already: dcn_coord_win_kernel)
int launch_col2im(const DcnArgs& a, const XGeom& xg, bool bf16, const void* dcols, const void* x, const float* off,
                  const float* msk, float* gx, float* goff, float* gmsk, unsigned* amax, hipStream_t s,
                  bool coord = true);  // dcn_cols.hip
int launch_fwd_mfma(const DcnArgs& a, const void* x, int x_blocked, const float* off, const float* msk, const void* wf,
                    int ldw, int wrows, int cout, const float* bias, float* y, void* cols,
                    hipStream_t s);  // dcn_fwd_fused.hip
int launch_fwd_win(const DcnArgs& a, const void* x, const float* off, const float* msk, const void* wf, int ldw,
                   int wrows, int cout, const float* bias, float* y, void* cols, int R, int WH, int WW, size_t lds,
                   int dbg, hipStream_t s);  // dcn_fwd_fused.hip
int launch_coord_win(const DcnArgs& a, const void* dcols, const void* x, const float* off, const float* msk,
                     float* goff, float* gmsk, unsigned* amax, int R, int WH, int WW, size_t lds,
                     hipStream_t s);  // dcn_bwd_win.hip
int launch_bwd_fused(const DcnArgs& a, const BwdGeom& bg, const void* dy, int ldy, const void* wd, int ldw, int cop,
                     const void* x, const float* off, const float* msk, float* gx, bool nchw, float* goff,
                     float* gmsk, unsigned* amax, hipStream_t s);  // dcn_bwd_win.hip

}  // namespace sr_dcn
