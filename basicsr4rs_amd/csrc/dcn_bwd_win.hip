// Deformable convolution, the backward kernels on the forward's 8 x 16 output tile and LDS x window (bf16, one
// conv group, C = 64), and the 16 x 16 scatter that goes with them.
//   dcn_coord_win_kernel : the offset / mask gradients of sr_dcn_col2im from the dcols matrix (the scatter of
//                          that path is dcn_grad_x_kernel, dcn_cols.hip).
//   dcn_coord_dy8_kernel, dcn_gradx_dy8_kernel : sr_dcn_bwd_fused, see below.
#include "dcn_dev.h"

namespace sr_dcn {
namespace {

// Offset / mask gradients with the forward's LDS x window (bf16, one conv group, C = 64): the
// block owns an 8 x 16 output tile and stages its x window once (as dcn_fwd_win_kernel); per tap
// it stages the tap's offsets and masks for the tile in LDS (coalesced 16-pixel row segments),
// then item (pixel, channel vector v) reads its 16-B dcols piece (8 consecutive lanes = one
// pixel's 128-B row), its four corners from the window (global memory past it), and sums
// d bilinear / d h, / d w and the un-masked sample against dcols over its 8 channels; lanes of one
// deformable group combine by xor-shuffles and the group's first lane writes the three results
// over the LDS words it read, which are then stored coalesced.  Per-image max |mask * dcols| for
// the scatter's fixed-point scale as dcn_coord_grad_kernel.  Same math as that kernel (the
// reference's col2im_coord, deform_conv_cuda_kernel.cu:696-770); the channel sums run 8 per lane
// then across lanes.
__global__ void __launch_bounds__(DW_NT, 2) dcn_coord_win_kernel(DcnArgs a, const bf16_t* __restrict__ dcols,
                                                                 const bf16_t* __restrict__ x,
                                                                 const float* __restrict__ off,
                                                                 const float* __restrict__ msk,
                                                                 float* __restrict__ goff, float* __restrict__ gmsk,
                                                                 unsigned* __restrict__ amax, int R, int WH, int WW) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float* sO = (float*)s_raw;                                  // [3 * DG][DF_TP]: dh, dw per group, then masks
  unsigned char* sX = s_raw + (size_t)3 * a.DG * DF_TP * 4;  // [WH * WW][8 slots][16 B]
  const int HWo = a.Ho * a.Wo;
  const int64_t HWo64 = HWo;
  const int tw = (a.Wo + DW_TW - 1) / DW_TW, th = (a.Ho + DW_TH - 1) / DW_TH;
  const int bid = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int n = bid / (tw * th), t = bid - n * (tw * th);
  const int ho0 = (t / tw) * DW_TH, wo0 = (t - (t / tw) * tw) * DW_TW;
  const int y0 = ho0 * a.sh - a.ph - R, x0 = wo0 * a.sw - a.pw - R;
  const int tid = threadIdx.x;
  const int v = tid & 7, pxl = tid >> 3;  // channel vector; pixel (and pixel + 64)
  const uint32_t pxb = (uint32_t)a.Cp * 2u;
  const auto xr = make_rsrc(x + (int64_t)n * a.H * a.W * a.Cp, (uint32_t)((size_t)a.H * a.W * a.Cp * 2));
  const int nwin = WH * WW * 8;
  for (int b0 = 0; b0 < nwin; b0 += 4 * DW_NT) {
    u32x4 val[4];
    int dst[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = b0 + u * DW_NT + tid;
      const int pix = i >> 3, vv = i & 7;
      const int wy = pix / WW, wx = pix - wy * WW;
      const int yy = y0 + wy, xx = x0 + wx;
      const bool in = i < nwin && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      val[u] = buf_load16(xr, in ? (uint32_t)(yy * a.W + xx) * pxb + (uint32_t)vv * 16u : SR_OOB);
      dst[u] = i < nwin ? pix * 128 + ((vv ^ (pix & 7)) << 4) : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (dst[u] >= 0) *(u32x4*)(sX + dst[u]) = val[u];
  }
  const int gl = a.cpg / 8;             // lanes per deformable group (1, 2, 4 or 8)
  const int dgi = v * 8 / a.cpg;
  const int nrow = 3 * a.DG;            // staged rows per tap
  const int64_t obase = (int64_t)n * a.DG * 2 * a.K * HWo64, mbase = (int64_t)n * a.DG * a.K * HWo64;
  float vmax = 0.f;
  for (int k = 0; k < a.K; ++k) {
    // stage this tap's offsets and masks: row r < 2*DG is (group r/2, component r%2), then masks
    // (loading the next tap's a tap ahead in registers measured slower: 445 vs 421 us)
    for (int i = tid; i < nrow * DF_TP; i += DW_NT) {
      const int r = i / DF_TP, q = i - r * DF_TP;
      const int ho = ho0 + (q >> 4), wo = wo0 + (q & 15);
      float val = 0.f;
      if (ho < a.Ho && wo < a.Wo) {
        const int64_t pp = (int64_t)ho * a.Wo + wo;
        if (r < 2 * a.DG) val = off[obase + (int64_t)((r >> 1) * 2 * a.K + 2 * k + (r & 1)) * HWo64 + pp];
        else val = msk ? msk[mbase + (int64_t)((r - 2 * a.DG) * a.K + k) * HWo64 + pp] : 1.f;
      }
      sO[i] = val;
    }
    __syncthreads();
    const int ti = k / a.kw, tj = k - ti * a.kw;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int px = pxl + 64 * j;
      const int ho = ho0 + (px >> 4), wo = wo0 + (px & 15);
      const bool pv = ho < a.Ho && wo < a.Wo;
      const int p = pv ? ho * a.Wo + wo : 0;
      u32x4 dcu = u32x4{0u, 0u, 0u, 0u};
      if (pv) dcu = *(const u32x4*)(dcols + ((int64_t)n * HWo64 + p) * a.L + k * 64 + v * 8);
      float* ph = &sO[(2 * dgi) * DF_TP + px];
      float* pw = &sO[(2 * dgi + 1) * DF_TP + px];
      float* pm = &sO[(2 * a.DG + dgi) * DF_TP + px];
      const float m = *pm;
      const float h = (float)(ho * a.sh - a.ph + ti * a.dh) + *ph;
      const float w = (float)(wo * a.sw - a.pw + tj * a.dw) + *pw;
      const Sample s = make_sample(h, w, a.H, a.W);
      const bool ok = pv && s.valid;
      float acc_h = 0.f, acc_w = 0.f, acc_m = 0.f;
      if (ok) {
        const int ly = (int)floorf(h) - y0, lx = (int)floorf(w) - x0;
        u32x4 cv[4];
        if (ly >= 0 && ly + 1 < WH && lx >= 0 && lx + 1 < WW) {
          const int q0 = ly * WW + lx;
          const int qs[4] = {q0, q0 + 1, q0 + WW, q0 + WW + 1};
#pragma unroll
          for (int q = 0; q < 4; ++q) cv[q] = *(const u32x4*)(sX + qs[q] * 128 + ((v ^ (qs[q] & 7)) << 4));
        } else {
          const uint32_t cb16 = (uint32_t)v * 16u;
          cv[0] = buf_load16(xr, s.o1 >= 0 ? (uint32_t)s.o1 * pxb + cb16 : SR_OOB);
          cv[1] = buf_load16(xr, s.o2 >= 0 ? (uint32_t)s.o2 * pxb + cb16 : SR_OOB);
          cv[2] = buf_load16(xr, s.o3 >= 0 ? (uint32_t)s.o3 * pxb + cb16 : SR_OOB);
          cv[3] = buf_load16(xr, s.o4 >= 0 ? (uint32_t)s.o4 * pxb + cb16 : SR_OOB);
        }
        const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const auto f = [&](uint32_t w32) { return (e & 1) ? bf_hi(w32) : bf_lo(w32); };
          const float v1 = f(cv[0][e >> 1]), v2 = f(cv[1][e >> 1]), v3 = f(cv[2][e >> 1]), v4 = f(cv[3][e >> 1]);
          const float dc = f(dcu[e >> 1]);
          const float wh = -s.hw * v1 - s.lw * v2 + s.hw * v3 + s.lw * v4;
          const float ww = -s.hh * v1 + s.hh * v2 - s.lh * v3 + s.lh * v4;
          acc_h += wh * dc * m;
          acc_w += ww * dc * m;
          acc_m += dc * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
          vmax = fmaxf(vmax, fabsf(dc * m));
          if (!(fabsf(dc * m) <= 3.0e38f)) vmax = __builtin_inff();
        }
      }
      // combine the group's lanes (consecutive: v is the lane's low 3 bits)
      for (int o = 1; o < gl; o <<= 1) {
        acc_h += __shfl_xor(acc_h, o);
        acc_w += __shfl_xor(acc_w, o);
        acc_m += __shfl_xor(acc_m, o);
      }
      __builtin_amdgcn_wave_barrier();
      if ((v & (gl - 1)) == 0) {  // every lane of the group has read these words (same wave)
        *ph = acc_h;
        *pw = acc_w;
        *pm = acc_m;
      }
    }
    __syncthreads();
    for (int i = tid; i < nrow * DF_TP; i += DW_NT) {
      const int r = i / DF_TP, q = i - r * DF_TP;
      const int ho = ho0 + (q >> 4), wo = wo0 + (q & 15);
      if (ho >= a.Ho || wo >= a.Wo) continue;
      const int64_t pp = (int64_t)ho * a.Wo + wo;
      if (r < 2 * a.DG) goff[obase + (int64_t)((r >> 1) * 2 * a.K + 2 * k + (r & 1)) * HWo64 + pp] = sO[i];
      else if (gmsk) gmsk[mbase + (int64_t)((r - 2 * a.DG) * a.K + k) * HWo64 + pp] = sO[i];
    }
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
  if ((tid & 63) == 0 && vmax > 0.f) atomicMax(amax + n, __float_as_uint(vmax));
}

// ---------------------------------------------------------------------------------------------
// Fused backward (round 4; bf16, one conv group, C = 64, Cout <= 64): the column gradient
// dcols = dy . W (the reference's per-image addmm into columns, deform_conv_cuda.cpp:640-660) is
// never stored.  Both kernels form each tap's dcols tile on MFMA from the dy tile, transposed:
// dcols^T[ci][px] = sum_co wd[k*64 + ci][co] * dy[px][co] (v_mfma_f32_16x16x32_bf16 with the
// weight rows as A and a pixel row of dy as B), rounded to bf16 as the dcols path's GEMM stores it,
// so both paths sample the same values.
//   dcn_coord_dy8_kernel : offset / mask gradients (col2im_coord, deform_conv_cuda_kernel.cu:696-770)
//                          on dcn_coord_win_kernel's 8 x 16 tile and x window, the tap's 64 x 64 weight
//                          slice double-buffered in LDS; per-image max |mask * dcols|.
//   dcn_gradx_dy8_kernel : the bilinear scatter (col2im, :635-693) into the fixed-point LDS image of a
//                          16 x 16 tile's footprint, 16 channels per pass (one MFMA tile), weight
//                          fragments from L2 a tap ahead, offsets / masks a tap ahead.
// Both use the eight-channel lane layout of own8 (dcn_dev.h).
//
// Offsets / masks read per lane a tap ahead (16 consecutive pixels of one plane per 16 lanes) and the
// gradients stored per lane, so no offset staging and ONE barrier per tap (the weight slices are
// double-buffered in LDS).  gxz (optional): the NCHW grad_x of the call, zeroed by the blocks after
// their last tap (the scatter kernel that follows accumulates into it).
__global__ void __launch_bounds__(DC8_NT, 2) dcn_coord_dy8_kernel(DcnArgs a, const bf16_t* __restrict__ dy, int ldy,
                                                                 const bf16_t* __restrict__ wd, int ldw, int cop,
                                                                 const bf16_t* __restrict__ x,
                                                                 const float* __restrict__ off,
                                                                 const float* __restrict__ msk,
                                                                 float* __restrict__ goff, float* __restrict__ gmsk,
                                                                 unsigned* __restrict__ amax, int R, int WH, int WW,
                                                                 float* __restrict__ gxz, int64_t gxn4) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  bf16_t* sW = (bf16_t*)s_raw;                                 // [2][64 ci][DF_RS]: wd rows of taps k, k + 1
  unsigned char* sX = s_raw + 2 * 64 * DF_RS * 2;             // [WH * WW][8 slots][16 B]
  const int HWo = a.Ho * a.Wo;
  const int64_t HWo64 = HWo;
  const int tw = (a.Wo + DW_TW - 1) / DW_TW, th = (a.Ho + DW_TH - 1) / DW_TH;
  const int bid = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int n = bid / (tw * th), t = bid - n * (tw * th);
  const int ho0 = (t / tw) * DW_TH, wo0 = (t - (t / tw) * tw) * DW_TW;
  const int y0 = ho0 * a.sh - a.ph - R, x0 = wo0 * a.sw - a.pw - R;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, pl = lane & 15;
  const int ho = ho0 + 2 * wv + (g & 1), wo = wo0 + pl;  // this lane's pixel
  const bool pv = ho < a.Ho && wo < a.Wo;
  const int p = pv ? ho * a.Wo + wo : 0;
  const uint32_t pxb = (uint32_t)a.Cp * 2u;
  const auto xr = make_rsrc(x + (int64_t)n * a.H * a.W * a.Cp, (uint32_t)((size_t)a.H * a.W * a.Cp * 2));
  const auto dyr = make_rsrc(dy + (int64_t)n * HWo64 * ldy, (uint32_t)((size_t)HWo * ldy * 2));
  const auto wr = make_rsrc(wd, (uint32_t)((size_t)a.K * 64 * ldw * 2));
  u32x4 dyf[2][2];  // B fragments of both rows
#pragma unroll
  for (int uu = 0; uu < 2; ++uu) {
    const int hu = ho0 + 2 * wv + uu;
    const bool v = hu < a.Ho && wo < a.Wo;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int co = 32 * kk + 8 * g;
      dyf[uu][kk] = buf_load16(dyr, v && co < cop ? (uint32_t)((hu * a.Wo + wo) * ldy + co) * 2u : SR_OOB);
    }
  }
  auto wload = [&](int k, u32x4 (&wp)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = tid + DC8_NT * j, row = q >> 3, pc = q & 7;
      wp[j] = buf_load16(wr, 8 * pc < cop ? (uint32_t)((k * 64 + row) * ldw + 8 * pc) * 2u : SR_OOB);
    }
  };
  auto wstore = [&](int buf, const u32x4 (&wp)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = tid + DC8_NT * j, row = q >> 3, pc = q & 7;
      *(u32x4*)&sW[(buf * 64 + row) * DF_RS + 8 * pc] = wp[j];
    }
  };
  const int64_t obase = (int64_t)n * a.DG * 2 * a.K * HWo64, mbase = (int64_t)n * a.DG * a.K * HWo64;
  int dgc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) dgc[cb] = (16 * cb + 8 * (g >> 1)) / a.cpg;
  auto load_om = [&](int k, float (&o)[4][3]) {
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      const int dgi = dgc[cb];
      o[cb][0] = pv ? off[obase + (int64_t)(dgi * 2 * a.K + 2 * k) * HWo64 + p] : 0.f;
      o[cb][1] = pv ? off[obase + (int64_t)(dgi * 2 * a.K + 2 * k + 1) * HWo64 + p] : 0.f;
      o[cb][2] = pv ? (msk ? msk[mbase + (int64_t)(dgi * a.K + k) * HWo64 + p] : 1.f) : 0.f;
    }
  };
  u32x4 wp[2];
  wload(0, wp);
  float om[4][3], om1[4][3];  // taps k and k + 1 (the loads run two taps ahead)
  load_om(0, om);
  if (a.K > 1) load_om(1, om1);
  const int nwin = WH * WW * 8;
  for (int b0 = 0; b0 < nwin; b0 += 4 * DC8_NT) {
    u32x4 val[4];
    int dst[4];
#pragma unroll
    for (int uq = 0; uq < 4; ++uq) {
      const int i = b0 + uq * DC8_NT + tid;
      const int pix = i >> 3, vv = i & 7;
      const int wy = pix / WW, wx = pix - wy * WW;
      const int yy = y0 + wy, xx = x0 + wx;
      const bool in = i < nwin && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
      val[uq] = buf_load16(xr, in ? (uint32_t)(yy * a.W + xx) * pxb + (uint32_t)vv * 16u : SR_OOB);
      dst[uq] = i < nwin ? pix * 128 + ((vv ^ (pix & 7)) << 4) : -1;
    }
#pragma unroll
    for (int uq = 0; uq < 4; ++uq)
      if (dst[uq] >= 0) *(u32x4*)(sX + dst[uq]) = val[uq];
  }
  wstore(0, wp);
  if (a.K > 1) wload(1, wp);
  __syncthreads();
  float vmax = 0.f;
  const int gv = a.cpg / 8;  // channel vectors per deformable group
  for (int k = 0; k < a.K; ++k) {
    float omn[4][3];
    if (k + 2 < a.K) load_om(k + 2, omn);
    f32x4 acc[2][4];
#pragma unroll
    for (int uu = 0; uu < 2; ++uu)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[uu][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bf16_t* sWk = sW + (k & 1) * 64 * DF_RS;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const u32x4 af = *(const u32x4*)&sWk[(16 * cb + pl) * DF_RS + 32 * kk + 8 * g];
        mfma_bf16(af, dyf[0][kk], acc[0][cb]);
        mfma_bf16(af, dyf[1][kk], acc[1][cb]);
      }
    if (k + 1 < a.K) {  // the other buffer's last readers (tap k - 1) are past this tap's barrier
      wstore((k + 1) & 1, wp);
      if (k + 2 < a.K) wload(k + 2, wp);
    }
    const int ti = k / a.kw, tj = k - ti * a.kw;
    const float hk = (float)(ho * a.sh - a.ph + ti * a.dh), wk = (float)(wo * a.sw - a.pw + tj * a.dw);
    float rh[4], rw[4], rm[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
      float dc[8];
      own8(acc[0][cb], acc[1][cb], g, dc);
      const int v = 2 * cb + (g >> 1);
      const float m = om[cb][2];
      const float h = hk + om[cb][0], w = wk + om[cb][1];
      const Sample s = make_sample(h, w, a.H, a.W);
      float ah = 0.f, aw = 0.f, am = 0.f;
      if (pv && s.valid) {
        const int ly = (int)floorf(h) - y0, lx = (int)floorf(w) - x0;
        u32x4 cv[4];
        if (ly >= 0 && ly + 1 < WH && lx >= 0 && lx + 1 < WW) {
          const int q0 = ly * WW + lx;
          const int qs[4] = {q0, q0 + 1, q0 + WW, q0 + WW + 1};
#pragma unroll
          for (int q = 0; q < 4; ++q) cv[q] = *(const u32x4*)(sX + qs[q] * 128 + ((v ^ (qs[q] & 7)) << 4));
        } else {
          const uint32_t cb16 = (uint32_t)v * 16u;
          cv[0] = buf_load16(xr, s.o1 >= 0 ? (uint32_t)s.o1 * pxb + cb16 : SR_OOB);
          cv[1] = buf_load16(xr, s.o2 >= 0 ? (uint32_t)s.o2 * pxb + cb16 : SR_OOB);
          cv[2] = buf_load16(xr, s.o3 >= 0 ? (uint32_t)s.o3 * pxb + cb16 : SR_OOB);
          cv[3] = buf_load16(xr, s.o4 >= 0 ? (uint32_t)s.o4 * pxb + cb16 : SR_OOB);
        }
        const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const auto f = [&](uint32_t w32) { return (e & 1) ? bf_hi(w32) : bf_lo(w32); };
          const float v1 = f(cv[0][e >> 1]), v2 = f(cv[1][e >> 1]), v3 = f(cv[2][e >> 1]), v4 = f(cv[3][e >> 1]);
          const float wh = -s.hw * v1 - s.lw * v2 + s.hw * v3 + s.lw * v4;
          const float ww = -s.hh * v1 + s.hh * v2 - s.lh * v3 + s.lh * v4;
          ah += wh * dc[e] * m;
          aw += ww * dc[e] * m;
          am += dc[e] * (w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4);
          vmax = fmaxf(vmax, fabsf(dc[e] * m));
          if (!(fabsf(dc[e] * m) <= 3.0e38f)) vmax = __builtin_inff();
        }
      }
      rh[cb] = ah; rw[cb] = aw; rm[cb] = am;
    }
    // a group's vectors: cb pairs (cpg 32) or all four (cpg 64) of the lane, then the lanes ^ 32
    if (gv >= 4) {
      rh[0] += rh[1]; rw[0] += rw[1]; rm[0] += rm[1];
      rh[2] += rh[3]; rw[2] += rw[3]; rm[2] += rm[3];
    }
    if (gv >= 8) { rh[0] += rh[2]; rw[0] += rw[2]; rm[0] += rm[2]; }
    if (gv >= 2) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        rh[cb] += __shfl_xor(rh[cb], 32); rw[cb] += __shfl_xor(rw[cb], 32); rm[cb] += __shfl_xor(rm[cb], 32);
      }
    }
    if (pv) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const int v = 2 * cb + (g >> 1);
        if (v % gv == 0) {  // the lane holding the group's first vector
          const int dgi = dgc[cb];
          goff[obase + (int64_t)(dgi * 2 * a.K + 2 * k) * HWo64 + p] = rh[cb];
          goff[obase + (int64_t)(dgi * 2 * a.K + 2 * k + 1) * HWo64 + p] = rw[cb];
          if (gmsk) gmsk[mbase + (int64_t)(dgi * a.K + k) * HWo64 + p] = rm[cb];
        }
      }
    }
    __syncthreads();  // the next tap's weight slice is in LDS
    if (k + 1 < a.K) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          om[cb][e] = om1[cb][e];
          om1[cb][e] = omn[cb][e];
        }
    }
  }
  for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
  if (lane == 0 && vmax > 0.f) atomicMax(amax + n, __float_as_uint(vmax));
  for (int64_t i = (int64_t)blockIdx.x * DC8_NT + tid; i < gxn4; i += (int64_t)gridDim.x * DC8_NT)
    ((f32x4*)gxz)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// The scatter kernel.  FXB 64: the int64 fixed-point LDS image of the
// round-3 kernel (scale 2^(FXE - e) for a per-image max |mask * dcols| below 2^e, FXE = 48); FXB 32: int32
// fixed point, FXE = 18.  The bound this relies on: every (pixel, tap) sample of the 16 x 16 tile adds at most
// one corner to a cell, so a cell sums at most 256 K contributions of magnitude below 2^FXE each, and
// FXE <= 30 - ceil(log2(256 K)) (62 - ... for int64) keeps the sum below 2^30 (2^62): gx_fx_bits() (dcn.hip) lowers
// FXE past 16 (64) taps -- at 49 taps 256 x 49 x 2^18 = 3.3e9 would wrap the int32 cell when the samples
// converge with one sign.  The quantum is 2^-FXE of the image's max |mask * dcols| (the
// dcols themselves carry bf16 rounding, 2^-9 of each value).  The float -> int64 conversion is ~12 VALU
// instructions per corner and channel, the int32 one two -- the kernel is VALU-bound on them -- and
// the int32 image is half the LDS (a wider halo fits).  fp32 LDS atomics are ~25x slower on gfx950.
// NCHW: grad_x as fp32 [N][C][H][W] (the op's output layout: no NHWC -> NCHW pass), else NHWC
// [N][H][W][Cp]; the flush then walks pixels fastest, so the atomics of a wave are row-contiguous.
// OCC: 8-wave blocks per CU the registers are budgeted for (launch bounds count waves per SIMD; at 3
// the int32 kernel spills 22 VGPRs and ran 1.10 vs 1.01 ms for the C5 op fwd + bwd)
template <int FXB, bool NCHW, int OCC = 2>
__global__ void __launch_bounds__(DW_NT, 2 * OCC) dcn_gradx_dy8_kernel(DcnArgs a, int R, int RH, int RW, int FXE,
                                                                 const bf16_t* __restrict__ dy, int ldy,
                                                                 const bf16_t* __restrict__ wd, int ldw, int cop,
                                                                 const float* __restrict__ off,
                                                                 const float* __restrict__ msk,
                                                                 const unsigned* __restrict__ amax,
                                                                 float* __restrict__ gx) {
  extern __shared__ unsigned long long s_acc[];  // [RH * RW][DX_ST]: u64 (FXB 64) or u32
  unsigned* s_acc32 = (unsigned*)s_acc;
  const int HWo = a.Ho * a.Wo;
  const int64_t HWo64 = HWo;
  const int tw = (a.Wo + DX_TT - 1) / DX_TT, th = (a.Ho + DX_TT - 1) / DX_TT;
  const int bid = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int n = bid / (tw * th), t = bid - n * (tw * th);
  const float mx = __uint_as_float(amax[n]);
  if (mx == 0.f) return;  // nothing of this image is scattered (uniform per block)
  const bool direct = !(mx <= 3.0e38f);
  int ex = 0;
  frexpf(direct ? 1.f : mx, &ex);
  const int e = min(127, FXE - ex);
  const float sc = ldexpf(1.f, e), isc = ldexpf(1.f, -e);
  const int ho0 = (t / tw) * DX_TT, wo0 = (t - (t / tw) * tw) * DX_TT;
  const int ry0 = ho0 * a.sh - a.ph - R, rx0 = wo0 * a.sw - a.pw - R;
  const int RP = RH * RW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, g = lane >> 4, pl = lane & 15;
  const int64_t HW64 = (int64_t)a.H * a.W;
  float* gim = gx + (int64_t)n * HW64 * (NCHW ? a.C : a.Cp);
  // element (pixel o, channel c) of this image's grad_x, and the step between channels
  auto gaddr = [&](int64_t o, int c) { return NCHW ? gim + c * HW64 + o : gim + o * a.Cp + c; };
  const int64_t cstep = NCHW ? HW64 : 1;
  const auto dyr = make_rsrc(dy + (int64_t)n * HWo64 * ldy, (uint32_t)((size_t)HWo * ldy * 2));
  const auto wr = make_rsrc(wd, (uint32_t)((size_t)a.K * 64 * ldw * 2));
  const int ho = ho0 + 2 * wv + (g & 1), wo = wo0 + pl;  // this lane's pixel
  const bool pv = ho < a.Ho && wo < a.Wo;
  const int p = pv ? ho * a.Wo + wo : 0;
  u32x4 dyf[2][2];
#pragma unroll
  for (int uu = 0; uu < 2; ++uu) {
    const int hu = ho0 + 2 * wv + uu;
    const bool v = hu < a.Ho && wo < a.Wo;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int co = 32 * kk + 8 * g;
      dyf[uu][kk] = buf_load16(dyr, v && co < cop ? (uint32_t)((hu * a.Wo + wo) * ldy + co) * 2u : SR_OOB);
    }
  }
  const float* offn = off + (int64_t)n * a.DG * 2 * a.K * HWo64;
  const float* mskn = msk ? msk + (int64_t)n * a.DG * a.K * HWo64 : nullptr;
  for (int c0 = 0; c0 < a.C; c0 += DX_CPP) {
    const int c = c0 + 8 * (g >> 1), dgi = c / a.cpg;  // this lane's 8 channels
    auto load_w = [&](int k, u32x4 (&wa)[2]) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int co = 32 * kk + 8 * g;
        wa[kk] = buf_load16(wr, co < cop ? (uint32_t)((k * 64 + c0 + pl) * ldw + co) * 2u : SR_OOB);
      }
    };
    auto load_om = [&](int k, float (&o)[3]) {
      o[0] = pv ? offn[(int64_t)(dgi * 2 * a.K + 2 * k) * HWo64 + p] : 0.f;
      o[1] = pv ? offn[(int64_t)(dgi * 2 * a.K + 2 * k + 1) * HWo64 + p] : 0.f;
      o[2] = pv ? (mskn ? mskn[(int64_t)(dgi * a.K + k) * HWo64 + p] : 1.f) : 0.f;
    };
    // operands GX_PD taps ahead (a tap's work is ~0.3 us per wave, an HBM load several times that):
    // slot d holds tap k + d; the slots shift down one per tap (register moves)
    u32x4 wa[GX_PD][2];
    float om[GX_PD][3];
#pragma unroll
    for (int d = 0; d < GX_PD; ++d)
      if (d < a.K) {
        load_w(d, wa[d]);
        load_om(d, om[d]);
      }
    for (int i = tid; i < RP * DX_ST; i += DW_NT) {
      if (FXB == 64) s_acc[i] = 0ull;
      else s_acc32[i] = 0u;
    }
    __syncthreads();
    for (int k = 0; k < a.K; ++k) {
      u32x4 wn[2];
      float omn[3];
      if (k + GX_PD < a.K) {
        load_w(k + GX_PD, wn);
        load_om(k + GX_PD, omn);
      }
      f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
      mfma_bf16(wa[0][0], dyf[0][0], acc0);
      mfma_bf16(wa[0][1], dyf[0][1], acc0);
      mfma_bf16(wa[0][0], dyf[1][0], acc1);
      mfma_bf16(wa[0][1], dyf[1][1], acc1);
      float dm[8];
      own8(acc0, acc1, g, dm);
      const int ti = k / a.kw, tj = k - ti * a.kw;
      const float h = (float)(ho * a.sh - a.ph + ti * a.dh) + om[0][0];
      const float w = (float)(wo * a.sw - a.pw + tj * a.dw) + om[0][1];
      const Sample s = make_sample(h, w, a.H, a.W);
      if (pv && s.valid) {
#pragma unroll
        for (int e2 = 0; e2 < 8; ++e2) dm[e2] *= om[0][2];
        const int hl = (int)floorf(h), wl = (int)floorf(w);
        const float wt[4] = {s.hh * s.hw, s.hh * s.lw, s.lh * s.hw, s.lh * s.lw};
        const int oo[4] = {s.o1, s.o2, s.o3, s.o4};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (oo[q] < 0) continue;
          const int ly = hl + (q >> 1) - ry0, lx = wl + (q & 1) - rx0;
          if (!direct && ly >= 0 && ly < RH && lx >= 0 && lx < RW) {
            const int base = (ly * RW + lx) * DX_ST + 8 * (g >> 1);
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) {
              if (FXB == 64) atomicAdd(s_acc + base + e2, (unsigned long long)__float2ll_rn(wt[q] * dm[e2] * sc));
              else atomicAdd(s_acc32 + base + e2, (unsigned)__float2int_rn(wt[q] * dm[e2] * sc));
            }
          } else {
            float* dst = gaddr(oo[q], c);
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) unsafeAtomicAdd(dst + e2 * cstep, wt[q] * dm[e2]);
          }
        }
      }
#pragma unroll
      for (int d = 0; d + 1 < GX_PD; ++d) {
        wa[d][0] = wa[d + 1][0]; wa[d][1] = wa[d + 1][1];
        om[d][0] = om[d + 1][0]; om[d][1] = om[d + 1][1]; om[d][2] = om[d + 1][2];
      }
      wa[GX_PD - 1][0] = wn[0]; wa[GX_PD - 1][1] = wn[1];
      om[GX_PD - 1][0] = omn[0]; om[GX_PD - 1][1] = omn[1]; om[GX_PD - 1][2] = omn[2];
    }
    __syncthreads();
    for (int i = tid; i < RP * DX_CPP; i += DW_NT) {
      const int ch = NCHW ? i / RP : i % DX_CPP, pix = NCHW ? i - ch * RP : i / DX_CPP;
      const int yy = ry0 + pix / RW, xx = rx0 + pix % RW;
      if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W) continue;
      const float v = FXB == 64 ? (float)(long long)s_acc[pix * DX_ST + ch] * isc : (float)(int)s_acc32[pix * DX_ST + ch] * isc;
      if (v != 0.f) unsafeAtomicAdd(gaddr((int64_t)yy * a.W + xx, c0 + ch), v);
    }
    __syncthreads();
  }
}

}  // namespace

int launch_coord_win(const DcnArgs& a, const void* dcols, const void* x, const float* off, const float* msk,
                     float* goff, float* gmsk, unsigned* amax, int R, int WH, int WW, size_t lds, hipStream_t s) {
  const int wt = ((a.Ho + DW_TH - 1) / DW_TH) * ((a.Wo + DW_TW - 1) / DW_TW);
  if (lds > 65536 &&
      hipFuncSetAttribute((const void*)dcn_coord_win_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
          hipSuccess)
    return sr_fail(SR_ELAUNCH, "dcn_col2im: LDS attribute");
  hipLaunchKernelGGL(dcn_coord_win_kernel, dim3((unsigned)(a.N * wt)), dim3(DW_NT), lds, s, a, (const bf16_t*)dcols,
                     (const bf16_t*)x, off, msk, goff, gmsk, amax, R, WH, WW);
  if (hipGetLastError() != hipSuccess) return sr_fail(SR_ELAUNCH, "dcn_coord_win launch");
  return SR_OK;
}

int launch_bwd_fused(const DcnArgs& a, const BwdGeom& bg, const void* dy, int ldy, const void* wd, int ldw, int cop,
                     const void* x, const float* off, const float* msk, float* gx, bool nchw, float* goff,
                     float* gmsk, unsigned* amax, hipStream_t s) {
  // the scatter kernel of this call, chosen once for the attribute and the launch
  const auto k2 = bg.fx == 64 ? (nchw ? dcn_gradx_dy8_kernel<64, true> : dcn_gradx_dy8_kernel<64, false>)
                              : (nchw ? dcn_gradx_dy8_kernel<32, true> : dcn_gradx_dy8_kernel<32, false>);
  if (bg.lds1 > 65536 && hipFuncSetAttribute((const void*)dcn_coord_dy8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)bg.lds1) != hipSuccess)
    return sr_fail(SR_ELAUNCH, "dcn_bwd_fused: LDS attribute");
  if (bg.lds2 > 65536 &&
      hipFuncSetAttribute((const void*)k2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bg.lds2) != hipSuccess)
    return sr_fail(SR_ELAUNCH, "dcn_bwd_fused: LDS attribute");
  // NCHW grad_x is written in full: the coordinate kernel zeroes it (C H W a multiple of 4: C = 64)
  const int64_t gxn4 = nchw ? (int64_t)a.N * a.C * a.H * a.W / 4 : 0;
  const int wt = ((a.Ho + DW_TH - 1) / DW_TH) * ((a.Wo + DW_TW - 1) / DW_TW);
  hipLaunchKernelGGL(dcn_coord_dy8_kernel, dim3((unsigned)(a.N * wt)), dim3(DC8_NT), bg.lds1, s, a, (const bf16_t*)dy,
                     ldy, (const bf16_t*)wd, ldw, cop, (const bf16_t*)x, off, msk, goff, gmsk, amax, bg.R1, bg.WH,
                     bg.WW, nchw ? gx : nullptr, gxn4);
  if (hipGetLastError() != hipSuccess) return sr_fail(SR_ELAUNCH, "dcn_coord_dy8 launch");
  const int xt = ((a.Ho + DX_TT - 1) / DX_TT) * ((a.Wo + DX_TT - 1) / DX_TT);
  hipLaunchKernelGGL(k2, dim3((unsigned)(a.N * xt)), dim3(DW_NT), bg.lds2, s, a, bg.R2, bg.RH, bg.RW, bg.fxe,
                     (const bf16_t*)dy, ldy, (const bf16_t*)wd, ldw, cop, off, msk, (const unsigned*)amax, gx);
  return sr_check(hipGetLastError(), "dcn_gradx_dy8 launch");
}

}  // namespace sr_dcn
