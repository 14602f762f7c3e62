// Kernels of the Real-ESRGAN second-order degradation (basicsr/models/realesrgan_model.py:68-185), which the
// reference runs on the device inside feed_data with about a hundred stock launches per step.  Images are NCHW fp32
// planes; all arithmetic is fp32; no floating-point atomics, fixed summation orders: two runs give identical bits.
//
//   filter2d_kernel<K>    : reflect-padded correlation of every plane with a per-sample or shared K x K kernel
//                           (img_process_util.py:7-31).  A 32 x 64 output tile plus its halo is staged in LDS once, the
//                           K * K weights sit in LDS (broadcast reads); a thread owns 8 rows of one column and walks
//                           the kernel columns with the K + 7 inputs of that column in registers.
//   blur_row_kernel, blur_col_kernel<M> : one 1-D reflect-padded pass of an r-tap filter (r odd <= 51) along rows /
//                           columns; a thread owns 4 consecutive outputs along the filter axis and consumes the line
//                           in 4-value chunks (16 FMAs per chunk, taps from a zero-padded LDS copy as two 16-byte
//                           broadcasts).  Column-pass epilogues M: 1 = residual = img - blur and the mask
//                           |residual| * 255 > threshold; 2 = the USM blend with the blurred mask.  USMSharp
//                           (img_process_util.py:63-83) is row, column<1>, row, column<2>: four launches.
//   resize_kernel<MODE>   : F.interpolate area / bilinear / bicubic (A = -0.75), align_corners=False, no antialias,
//                           with the two coordinate scales given by the caller; a thread owns 4 outputs of a row.
//   gaussian_apply_kernel, level_presence_kernel, poisson_rate_kernel, poisson_apply_kernel : the noise of
//                           data/degradations.py:460-553, 609-723 with the draws passed in; the count of distinct
//                           8-bit levels per sample comes from a 256-bit presence map (LDS bitmap, integer atomicOr
//                           to global) instead of torch.unique on the host.
//   jpeg_kernel           : DiffJPEG.forward (diffjpeg.py:449-491): one block per 16 x 16 macroblock; colour
//                           conversion, chroma averaging, separable 8-point DCT, quantisation, IDCT and the way back
//                           stay in LDS and registers.
//
// Nothing allocates or synchronises.
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int DG_T = 256;

SR_DEV int reflect_idx(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

// clamp(rint(255 v), 0, 255) / 255 with a true division (realesrgan_model.py:168)
SR_DEV float round255_f(float v) { return __fdiv_rn(fminf(fmaxf(rintf(__fmul_rn(v, 255.f)), 0.f), 255.f), 255.f); }

// ------------------------------------------------------------------------------------------------ filter2d

constexpr int F_TH = 32, F_TW = 64, F_R = 8;  // output tile; rows per thread (F_TH = 4 * F_R, F_TW = one wave)

template <int K>
__global__ void __launch_bounds__(DG_T)
filter2d_kernel(const float* __restrict__ x, const float* __restrict__ kern, int kernel_batch, int C, int H, int W,
                int round255, float* __restrict__ y) {
  constexpr int P = K / 2, LH = F_TH + K - 1, LW = F_TW + K - 1, LS = LW | 1;
  __shared__ float s[LH * LS];
  __shared__ float wt[K * K];
  const int tid = threadIdx.x;
  const int plane = blockIdx.z, n = plane / C;
  const float* kp = kern + (kernel_batch ? (size_t)n * K * K : 0);
  for (int i = tid; i < K * K; i += DG_T) wt[i] = kp[i];
  const int y0 = blockIdx.y * F_TH, x0 = blockIdx.x * F_TW;
  const float* xp = x + (size_t)plane * H * W;
  for (int i = tid; i < LH * LW; i += DG_T) {
    const int ly = i / LW, lx = i - ly * LW;
    const int gy = y0 - P + ly, gx = x0 - P + lx;
    float v = 0.f;  // positions no output of the image reads
    if (gy < H + P && gx < W + P) v = xp[(size_t)reflect_idx(gy, H) * W + reflect_idx(gx, W)];
    s[ly * LS + lx] = v;
  }
  __syncthreads();
  const int col = tid & 63, r0 = (tid >> 6) * F_R;
  float acc[F_R];
#pragma unroll
  for (int j = 0; j < F_R; ++j) acc[j] = 0.f;
#pragma unroll 1
  for (int kx = 0; kx < K; ++kx) {
    float c[K + F_R - 1];
#pragma unroll
    for (int j = 0; j < K + F_R - 1; ++j) c[j] = s[(r0 + j) * LS + col + kx];
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const float w = wt[ky * K + kx];
#pragma unroll
      for (int j = 0; j < F_R; ++j) acc[j] = fmaf(w, c[ky + j], acc[j]);
    }
  }
  const int gx = x0 + col;
  if (gx >= W) return;
  float* yp = y + (size_t)plane * H * W;
#pragma unroll
  for (int j = 0; j < F_R; ++j) {
    const int gy = y0 + r0 + j;
    if (gy < H) yp[(size_t)gy * W + gx] = round255 ? round255_f(acc[j]) : acc[j];
  }
}

template <int K>
void filter2d_launch(dim3 grid, hipStream_t s, const float* x, const float* kern, int kb, int C, int H, int W, int r255,
                     float* y) {
  hipLaunchKernelGGL(filter2d_kernel<K>, grid, dim3(DG_T), 0, s, x, kern, kb, C, H, W, r255, y);
}

// ------------------------------------------------------------------------------------------ separable blur

constexpr int BL_MAXR = 51;
constexpr int BL_NCH = (BL_MAXR + 3 + 3) / 4;  // 4-value chunks a thread's 4 outputs read at most
constexpr int BR_TW = 128, BR_TH = 8, BR_LS = BR_TW - 4 + 4 * BL_NCH + 4;  // row pass: tile, LDS row stride
constexpr int BC_TW = 32, BC_TH = 32, BC_LH = BC_TH - 4 + 4 * BL_NCH;      // column pass: tile, LDS rows

struct BlurArgs {
  const float* x;     // the plane the pass filters
  const float* taps;  // [r]
  const float* img;   // modes 1, 2: the image
  const float* res;   // mode 2: the residual
  float* y;           // mode 0: the filtered plane; mode 1: the residual; mode 2: the sharpened image
  float* mask;        // mode 1
  int H, W, r, vec;
  float weight, threshold;
};

// acc[j] += sum over the chunk's 4 values v[e] of tap[4 m + e - j] v[e]; w8 = taps 4 m - 4 .. 4 m + 3
SR_DEV void blur_chunk(const f32x4 wa, const f32x4 wb, const float (&v)[4], float (&acc)[4]) {
  const float w8[8] = {wa[0], wa[1], wa[2], wa[3], wb[0], wb[1], wb[2], wb[3]};
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaf(w8[4 + e - j], v[e], acc[j]);
}

SR_DEV void blur_load_taps(float* wp, const float* taps, int r) {
  for (int i = threadIdx.x; i < 4 * (BL_NCH + 1); i += DG_T) {
    const int t = i - 4;
    wp[i] = (t >= 0 && t < r) ? taps[t] : 0.f;
  }
}

__global__ void __launch_bounds__(DG_T) blur_row_kernel(BlurArgs a) {
  __shared__ __attribute__((aligned(16))) float s[BR_TH * BR_LS];
  __shared__ __attribute__((aligned(16))) float wp[4 * (BL_NCH + 1)];
  const int tid = threadIdx.x, p = a.r / 2, nch = (a.r + 6) / 4;
  const int lw = BR_TW - 4 + 4 * nch;
  blur_load_taps(wp, a.taps, a.r);
  const int y0 = blockIdx.y * BR_TH, x0 = blockIdx.x * BR_TW;
  const size_t po = (size_t)blockIdx.z * a.H * a.W;
  for (int i = tid; i < BR_TH * lw; i += DG_T) {
    const int ly = i / lw, lx = i - ly * lw;
    const int gy = y0 + ly, gx = x0 - p + lx;
    float v = 0.f;
    if (gy < a.H && gx < a.W + p) v = a.x[po + (size_t)gy * a.W + reflect_idx(gx, a.W)];
    s[ly * BR_LS + lx] = v;
  }
  __syncthreads();
  const int tx = tid & 31, ty = tid >> 5;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const f32x4* w4 = (const f32x4*)wp;
  const f32x4* line = (const f32x4*)(s + ty * BR_LS + 4 * tx);
  for (int m = 0; m < nch; ++m) {
    const f32x4 c = line[m];
    const float v[4] = {c[0], c[1], c[2], c[3]};
    blur_chunk(w4[m], w4[m + 1], v, acc);
  }
  const int gy = y0 + ty, gx = x0 + 4 * tx;
  if (gy >= a.H || gx >= a.W) return;
  float* yp = a.y + po + (size_t)gy * a.W + gx;
  if (a.vec) {  // W % 4 == 0 and a 16-byte aligned base: the four are inside the row
    f32x4 o = {acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)yp = o;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (gx + j < a.W) yp[j] = acc[j];
  }
}

template <int MODE>
__global__ void __launch_bounds__(DG_T) blur_col_kernel(BlurArgs a) {
  __shared__ float s[BC_LH * BC_TW];
  __shared__ __attribute__((aligned(16))) float wp[4 * (BL_NCH + 1)];
  const int tid = threadIdx.x, p = a.r / 2, nch = (a.r + 6) / 4;
  const int lh = BC_TH - 4 + 4 * nch;
  blur_load_taps(wp, a.taps, a.r);
  const int y0 = blockIdx.y * BC_TH, x0 = blockIdx.x * BC_TW;
  const size_t po = (size_t)blockIdx.z * a.H * a.W;
  for (int i = tid; i < lh * BC_TW; i += DG_T) {
    const int ly = i / BC_TW, lx = i - ly * BC_TW;
    const int gy = y0 - p + ly, gx = x0 + lx;
    float v = 0.f;
    if (gy < a.H + p && gx < a.W) v = a.x[po + (size_t)reflect_idx(gy, a.H) * a.W + gx];
    s[i] = v;
  }
  __syncthreads();
  const int tx = tid & 31, tg = tid >> 5;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const f32x4* w4 = (const f32x4*)wp;
  const float* line = s + (4 * tg) * BC_TW + tx;
  for (int m = 0; m < nch; ++m) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = line[(4 * m + e) * BC_TW];
    blur_chunk(w4[m], w4[m + 1], v, acc);
  }
  const int gx = x0 + tx;
  if (gx >= a.W) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int gy = y0 + 4 * tg + j;
    if (gy >= a.H) continue;
    const size_t o = po + (size_t)gy * a.W + gx;
    if (MODE == 0) {
      a.y[o] = acc[j];
    } else if (MODE == 1) {
      const float res = __fsub_rn(a.img[o], acc[j]);
      a.y[o] = res;
      a.mask[o] = __fmul_rn(fabsf(res), 255.f) > a.threshold ? 1.f : 0.f;
    } else {
      const float img = a.img[o], soft = acc[j];
      const float sharp = fminf(fmaxf(__fadd_rn(img, __fmul_rn(a.weight, a.res[o])), 0.f), 1.f);
      a.y[o] = __fadd_rn(__fmul_rn(soft, sharp), __fmul_rn(__fsub_rn(1.f, soft), img));
    }
  }
}

// ------------------------------------------------------------------------------------------------- resize

enum { RS_AREA = 0, RS_BILINEAR = 1, RS_BICUBIC = 2 };

struct ResizeArgs {
  const float* x;
  float* y;
  int Hin, Win, Hout, Wout, gpr, vec;  // gpr: groups of 4 outputs per row
  uint32_t groups;                     // planes * Hout * gpr
  float sh, sw;
};

SR_DEV float cubic1(float x) {  // |x| <= 1, A = -0.75
  return ((-0.75f + 2.f) * x - (-0.75f + 3.f)) * x * x + 1.f;
}
SR_DEV float cubic2(float x) {  // 1 < |x| < 2
  return ((-0.75f * x - 5.f * -0.75f) * x + 8.f * -0.75f) * x - 4.f * -0.75f;
}

template <int MODE>
SR_DEV float resize_one(const float* __restrict__ xp, const ResizeArgs& a, int oy, int ox) {
  if (MODE == RS_AREA) {
    const int ys = (int)(((int64_t)oy * a.Hin) / a.Hout), ye = (int)(((int64_t)(oy + 1) * a.Hin + a.Hout - 1) / a.Hout);
    const int xs = (int)(((int64_t)ox * a.Win) / a.Wout), xe = (int)(((int64_t)(ox + 1) * a.Win + a.Wout - 1) / a.Wout);
    float sum = 0.f;
    for (int iy = ys; iy < ye; ++iy)
      for (int ix = xs; ix < xe; ++ix) sum += xp[(size_t)iy * a.Win + ix];
    return __fdiv_rn(sum, (float)((ye - ys) * (xe - xs)));
  } else if (MODE == RS_BILINEAR) {
    const float sy = fmaxf(a.sh * ((float)oy + 0.5f) - 0.5f, 0.f), sx = fmaxf(a.sw * ((float)ox + 0.5f) - 0.5f, 0.f);
    const int iy = min((int)sy, a.Hin - 1), ix = min((int)sx, a.Win - 1);
    const int iy1 = min(iy + 1, a.Hin - 1), ix1 = min(ix + 1, a.Win - 1);
    const float ly = sy - (float)iy, lx = sx - (float)ix, hy = 1.f - ly, hx = 1.f - lx;
    const float* r0 = xp + (size_t)iy * a.Win;
    const float* r1 = xp + (size_t)iy1 * a.Win;
    return hy * (hx * r0[ix] + lx * r0[ix1]) + ly * (hx * r1[ix] + lx * r1[ix1]);
  } else {
    const float sy = a.sh * ((float)oy + 0.5f) - 0.5f, sx = a.sw * ((float)ox + 0.5f) - 0.5f;
    const float fy = floorf(sy), fx = floorf(sx);
    const float ty = sy - fy, tx = sx - fx;
    const int iy = (int)fy, ix = (int)fx;
    const float wy[4] = {cubic2(ty + 1.f), cubic1(ty), cubic1(1.f - ty), cubic2(2.f - ty)};
    const float wx[4] = {cubic2(tx + 1.f), cubic1(tx), cubic1(1.f - tx), cubic2(2.f - tx)};
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = min(max(ix - 1 + j, 0), a.Win - 1);
    float out = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* r = xp + (size_t)min(max(iy - 1 + i, 0), a.Hin - 1) * a.Win;
      float row = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) row = fmaf(wx[j], r[xs[j]], row);
      out = fmaf(wy[i], row, out);
    }
    return out;
  }
}

template <int MODE>
__global__ void __launch_bounds__(DG_T) resize_kernel(ResizeArgs a) {
  for (uint32_t g = blockIdx.x * DG_T + threadIdx.x; g < a.groups; g += gridDim.x * DG_T) {
    const uint32_t row = g / (uint32_t)a.gpr, gx = g - row * (uint32_t)a.gpr;
    const uint32_t plane = row / (uint32_t)a.Hout, oy = row - plane * (uint32_t)a.Hout;
    const float* xp = a.x + (size_t)plane * a.Hin * a.Win;
    float* yp = a.y + ((size_t)plane * a.Hout + oy) * a.Wout + 4 * gx;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ox = (int)(4 * gx) + j;
      o[j] = ox < a.Wout ? resize_one<MODE>(xp, a, (int)oy, ox) : 0.f;
    }
    if (a.vec) {  // Wout % 4 == 0 and a 16-byte aligned base
      f32x4 v = {o[0], o[1], o[2], o[3]};
      *(f32x4*)yp = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((int)(4 * gx) + j < a.Wout) yp[j] = o[j];
    }
  }
}

// -------------------------------------------------------------------------------------------------- noise

struct NoiseArgs {
  const float* img;     // [B][3][H][W]
  const float* na;      // gaussian: normal [B][3][H][W]; poisson: colour draws
  const float* nb;      // gaussian: normal_gray [H][W] or null; poisson: gray draws [B][H][W] or null
  const float* vals;    // poisson: [B][2] (colour, gray)
  const float* amp;     // [B]: sigma (gaussian) or scale (poisson)
  const float* gray;    // [B] 0 / 1, or null
  float* out;
  int HW, finish;
  uint32_t total;       // B * 3 * HW
};

SR_DEV float level255(float v) { return fminf(fmaxf(rintf(__fmul_rn(v, 255.f)), 0.f), 255.f); }
// torchvision's rgb_to_grayscale: (0.2989 r + 0.587 g) + 0.114 b with every operation rounded
SR_DEV float gray_of(float r, float g, float b) {
  return __fadd_rn(__fadd_rn(__fmul_rn(0.2989f, r), __fmul_rn(0.587f, g)), __fmul_rn(0.114f, b));
}
// finish flags of the noise entries: 1 = round to 8 bits, 2 = no clip, 4 = the noise alone (the image is not added)
SR_DEV float noise_finish(float img, float noise, int finish) {
  const float v = (finish & 4) ? noise : __fadd_rn(img, noise);
  if (finish & 1) return (finish & 2) ? __fdiv_rn(rintf(__fmul_rn(v, 255.f)), 255.f) : round255_f(v);
  return (finish & 2) ? v : fminf(fmaxf(v, 0.f), 1.f);
}

__global__ void __launch_bounds__(DG_T) gaussian_apply_kernel(NoiseArgs a) {
  for (uint32_t i = blockIdx.x * DG_T + threadIdx.x; i < a.total; i += gridDim.x * DG_T) {
    const uint32_t plane = i / (uint32_t)a.HW, pix = i - plane * (uint32_t)a.HW, n = plane / 3u;
    const float sig = a.amp[n];
    float noise = __fdiv_rn(__fmul_rn(a.na[i], sig), 255.f);
    if (a.nb && a.gray) {
      const float g = a.gray[n];
      const float ng = __fdiv_rn(__fmul_rn(a.nb[pix], sig), 255.f);
      noise = __fadd_rn(__fmul_rn(noise, __fsub_rn(1.f, g)), __fmul_rn(ng, g));
    }
    a.out[i] = noise_finish(a.img[i], noise, a.finish);
  }
}

constexpr int LP_BLOCKS = 32;  // blocks per sample of the presence pass

// bitmap [B][2][8] words (colour levels, gray levels), zeroed by the caller
__global__ void __launch_bounds__(DG_T) level_presence_kernel(const float* __restrict__ img, int HW, unsigned* bitmap) {
  __shared__ unsigned bm[16];
  if (threadIdx.x < 16) bm[threadIdx.x] = 0u;
  __syncthreads();
  const float* p = img + (size_t)blockIdx.y * 3 * HW;
  for (int i = blockIdx.x * DG_T + threadIdx.x; i < HW; i += gridDim.x * DG_T) {
    const float r = p[i], g = p[HW + i], b = p[2 * HW + i];
    const int qr = (int)level255(r), qg = (int)level255(g), qb = (int)level255(b);
    const int qy = (int)level255(gray_of(r, g, b));
    atomicOr(&bm[qr >> 5], 1u << (qr & 31));
    atomicOr(&bm[qg >> 5], 1u << (qg & 31));
    atomicOr(&bm[qb >> 5], 1u << (qb & 31));
    atomicOr(&bm[8 + (qy >> 5)], 1u << (qy & 31));
  }
  __syncthreads();
  if (threadIdx.x < 16 && bm[threadIdx.x]) atomicOr(&bitmap[blockIdx.y * 16 + threadIdx.x], bm[threadIdx.x]);
}

// 2^ceil(log2(count of set bits)) of 8 words
SR_DEV float vals_of(const unsigned* w) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) c += __popc(w[i]);
  const int e = c <= 1 ? 0 : 32 - __clz(c - 1);
  return (float)(1 << e);
}

// rate_c [B][3][HW] = q / 255 * vals_c, rate_g [B][HW] = q_gray / 255 * vals_g, vals [B][2]
__global__ void __launch_bounds__(DG_T)
poisson_rate_kernel(const float* __restrict__ img, const unsigned* __restrict__ bitmap, int HW, float* rate_c,
                    float* rate_g, float* vals) {
  const int n = blockIdx.y;
  const float vc = vals_of(bitmap + n * 16), vg = vals_of(bitmap + n * 16 + 8);
  if (blockIdx.x == 0 && threadIdx.x == 0) vals[2 * n] = vc, vals[2 * n + 1] = vg;
  const float* p = img + (size_t)n * 3 * HW;
  float* rc = rate_c + (size_t)n * 3 * HW;
  for (int i = blockIdx.x * DG_T + threadIdx.x; i < HW; i += gridDim.x * DG_T) {
    const float r = p[i], g = p[HW + i], b = p[2 * HW + i];
    rc[i] = __fmul_rn(__fdiv_rn(level255(r), 255.f), vc);
    rc[HW + i] = __fmul_rn(__fdiv_rn(level255(g), 255.f), vc);
    rc[2 * HW + i] = __fmul_rn(__fdiv_rn(level255(b), 255.f), vc);
    rate_g[(size_t)n * HW + i] = __fmul_rn(__fdiv_rn(level255(gray_of(r, g, b)), 255.f), vg);
  }
}

__global__ void __launch_bounds__(DG_T) poisson_apply_kernel(NoiseArgs a) {
  for (uint32_t i = blockIdx.x * DG_T + threadIdx.x; i < a.total; i += gridDim.x * DG_T) {
    const uint32_t plane = i / (uint32_t)a.HW, pix = i - plane * (uint32_t)a.HW, n = plane / 3u;
    const float v = a.img[i];
    float noise = __fsub_rn(__fdiv_rn(a.na[i], a.vals[2 * n]), __fdiv_rn(level255(v), 255.f));
    if (a.nb && a.gray) {
      const float* p = a.img + (size_t)n * 3 * a.HW + pix;
      const float y = gray_of(p[0], p[a.HW], p[2 * a.HW]);
      const float ng = __fsub_rn(__fdiv_rn(a.nb[(size_t)n * a.HW + pix], a.vals[2 * n + 1]), __fdiv_rn(level255(y), 255.f));
      const float g = a.gray[n];
      noise = __fadd_rn(__fmul_rn(noise, __fsub_rn(1.f, g)), __fmul_rn(ng, g));
    }
    a.out[i] = noise_finish(v, __fmul_rn(noise, a.amp[n]), a.finish);
  }
}

// --------------------------------------------------------------------------------------------------- JPEG

// cos(m pi / 16), m = 0 .. 31
__device__ __constant__ float JPEG_COS[32] = {
    1.0f,
    0.98078528040323043f,
    0.92387953251128674f,
    0.83146961230254524f,
    0.70710678118654757f,
    0.55557023301960229f,
    0.38268343236508984f,
    0.19509032201612833f,
    0.0f,
    -0.19509032201612833f,
    -0.38268343236508984f,
    -0.55557023301960229f,
    -0.70710678118654757f,
    -0.83146961230254524f,
    -0.92387953251128674f,
    -0.98078528040323043f,
    -1.0f,
    -0.98078528040323043f,
    -0.92387953251128674f,
    -0.83146961230254524f,
    -0.70710678118654757f,
    -0.55557023301960229f,
    -0.38268343236508984f,
    -0.19509032201612833f,
    0.0f,
    0.19509032201612833f,
    0.38268343236508984f,
    0.55557023301960229f,
    0.70710678118654757f,
    0.83146961230254524f,
    0.92387953251128674f,
    0.98078528040323043f,
};
// the luminance table of diffjpeg.py:14-18 BEFORE its transpose (the kernel indexes it [v][u]) and the 4 x 4 corner
// of the chroma table (symmetric; 99 elsewhere)
__device__ __constant__ float JPEG_Y[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                            14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                            18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                            49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__device__ __constant__ float JPEG_C[16] = {17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99};

// cos((2 j + 1) u pi / 16)
SR_DEV float jcos(int j, int u) { return JPEG_COS[((2 * j + 1) * u) & 31]; }

struct JpegArgs {
  const float* x;
  const float* quality;  // [B]
  float* y;
  float* coef;  // null, or Y [B][H16/8][W16/8][8][8] then Cb, Cr [B][H16/16][W16/16][8][8] each
  int H, W, mbx, mby, differentiable, round255;
};

__global__ void __launch_bounds__(DG_T) jpeg_kernel(JpegArgs a) {
  __shared__ float A[6][8][9];   // Y blocks 0..3 (block row-major), Cb 4, Cr 5
  __shared__ float T[6][8][9];
  __shared__ float CH[2][16][17];
  const int tid = threadIdx.x, px = tid & 15, py = tid >> 4;
  const int n = blockIdx.z, gy = blockIdx.y * 16 + py, gx = blockIdx.x * 16 + px;
  const size_t HW = (size_t)a.H * a.W;
  const bool inside = gy < a.H && gx < a.W;
  {
    float r = 0.f, g = 0.f, b = 0.f;  // the zero pad to the right and bottom enters before the x 255
    if (inside) {
      const float* p = a.x + (size_t)n * 3 * HW + (size_t)gy * a.W + gx;
      r = p[0] * 255.f, g = p[HW] * 255.f, b = p[2 * HW] * 255.f;
    }
    const float yy = fmaf(b, 0.114f, fmaf(g, 0.587f, r * 0.299f));
    const float cb = fmaf(b, 0.5f, fmaf(g, -0.331264f, r * -0.168736f)) + 128.f;
    const float cr = fmaf(b, -0.081312f, fmaf(g, -0.418688f, r * 0.5f)) + 128.f;
    A[(py >> 3) * 2 + (px >> 3)][py & 7][px & 7] = yy - 128.f;
    CH[0][py][px] = cb;
    CH[1][py][px] = cr;
  }
  __syncthreads();
  if (tid < 128) {
    const int c = tid >> 6, i = (tid >> 3) & 7, j = tid & 7;
    const float sum = (CH[c][2 * i][2 * j] + CH[c][2 * i][2 * j + 1]) + (CH[c][2 * i + 1][2 * j] + CH[c][2 * i + 1][2 * j + 1]);
    A[4 + c][i][j] = sum * 0.25f - 128.f;
  }
  __syncthreads();
  // forward DCT, rows: T[blk][i][v] = sum_j A[blk][i][j] cos((2 j + 1) v pi / 16)
  for (int w = tid; w < 384; w += DG_T) {
    const int blk = w >> 6, i = (w >> 3) & 7, v = w & 7;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(A[blk][i][j], jcos(j, v), acc);
    T[blk][i][v] = acc;
  }
  __syncthreads();
  // columns, scale, quantise, dequantise, the IDCT's alpha: A[blk][u][v]
  {
    const float q = a.quality[n];
    const float f = __fdiv_rn(q < 50.f ? __fdiv_rn(5000.f, q) : __fsub_rn(200.f, __fmul_rn(q, 2.f)), 100.f);
    for (int w = tid; w < 384; w += DG_T) {
      const int blk = w >> 6, u = (w >> 3) & 7, v = w & 7;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = fmaf(T[blk][i][v], jcos(i, u), acc);
      // alpha_u alpha_v and 0.25 alpha_u alpha_v as the reference's fp32 tables: 0.5, 0.70710678, 1 and a quarter of them
      const float scale = (u == 0 && v == 0) ? 0.5f : ((u == 0 || v == 0) ? 0.70710678118654757f : 1.f);
      const float sc = (u == 0 && v == 0) ? 0.125f : ((u == 0 || v == 0) ? 0.17677669529663687f : 0.25f);
      const float tab = blk < 4 ? JPEG_Y[v * 8 + u] : ((u < 4 && v < 4) ? JPEG_C[u * 4 + v] : 99.f);
      const float tf = __fmul_rn(tab, f);
      const float pre = __fdiv_rn(__fmul_rn(sc, acc), tf);
      float r = rintf(pre);
      if (a.differentiable) {
        const float d = __fsub_rn(pre, r);
        r = __fadd_rn(r, __fmul_rn(__fmul_rn(d, d), d));
      }
      if (a.coef) {
        const size_t ny = (size_t)gridDim.z * a.mby * a.mbx * 256, nc = ny / 4;
        size_t o;
        if (blk < 4) {
          const int by = blockIdx.y * 2 + (blk >> 1), bx = blockIdx.x * 2 + (blk & 1);
          o = (((size_t)n * (2 * a.mby) + by) * (2 * a.mbx) + bx) * 64;
        } else {
          o = ny + (size_t)(blk - 4) * nc + (((size_t)n * a.mby + blockIdx.y) * a.mbx + blockIdx.x) * 64;
        }
        a.coef[o + u * 8 + v] = r;
      }
      A[blk][u][v] = __fmul_rn(__fmul_rn(r, tf), scale);
    }
  }
  __syncthreads();
  // inverse, rows: T[blk][u][y] = sum_v A[blk][u][v] cos((2 y + 1) v pi / 16)
  for (int w = tid; w < 384; w += DG_T) {
    const int blk = w >> 6, u = (w >> 3) & 7, yv = w & 7;
    float acc = 0.f;
#pragma unroll
    for (int v = 0; v < 8; ++v) acc = fmaf(A[blk][u][v], jcos(yv, v), acc);
    T[blk][u][yv] = acc;
  }
  __syncthreads();
  for (int w = tid; w < 384; w += DG_T) {
    const int blk = w >> 6, xv = (w >> 3) & 7, yv = w & 7;
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = fmaf(T[blk][u][yv], jcos(xv, u), acc);
    A[blk][xv][yv] = fmaf(0.25f, acc, 128.f);
  }
  __syncthreads();
  if (!inside) return;
  const float yy = A[(py >> 3) * 2 + (px >> 3)][py & 7][px & 7];
  const float cb = A[4][py >> 1][px >> 1] - 128.f, cr = A[5][py >> 1][px >> 1] - 128.f;
  float o[3] = {fmaf(cr, 1.402f, yy), fmaf(cr, -0.714136f, fmaf(cb, -0.344136f, yy)), fmaf(cb, 1.772f, yy)};
  float* p = a.y + (size_t)n * 3 * HW + (size_t)gy * a.W + gx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = __fdiv_rn(fminf(fmaxf(o[c], 0.f), 255.f), 255.f);
    p[c * HW] = a.round255 ? round255_f(v) : v;
  }
}

// ---------------------------------------------------------------------------------------------- host side

int dg_fail(const char* what, int code, const char* why) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", what, why);
  return sr_fail(code, msg);
}

bool dg_al4(const void* p) { return !((uintptr_t)p & 3); }
bool dg_al16(const void* p) { return !((uintptr_t)p & 15); }

// planes of H x W fp32 addressed with 32-bit element counts
bool dg_fits(int64_t planes, int64_t H, int64_t W) { return planes * H * W < 0x7fffffffll; }

unsigned dg_grid(uint32_t items, int cap) {
  const uint32_t g = (items + DG_T - 1) / DG_T;
  return g > (uint32_t)cap ? (unsigned)cap : (g < 1 ? 1u : g);
}

int blur_check(const char* what, const float* x, int planes, int H, int W, const float* taps, int r, const float* tmp,
               const float* y) {
  if (!x || !taps || !tmp || !y) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(x) || !dg_al4(taps) || !dg_al4(tmp) || !dg_al4(y)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (planes <= 0 || planes > 65535 || H <= 0 || W <= 0) return dg_fail(what, SR_EINVAL, "bad arguments (1 to 65535 planes)");
  if (r < 1 || r > BL_MAXR || r % 2 == 0) return dg_fail(what, SR_EINVAL, "the filter length must be odd and at most 51");
  if (r / 2 >= H || r / 2 >= W) return dg_fail(what, SR_EINVAL, "image smaller than the reflect pad (pad < size)");
  if (tmp == x || tmp == y) return dg_fail(what, SR_EINVAL, "the row-pass buffer must not alias the input or the output");
  if (!dg_fits(planes, H, W)) return dg_fail(what, SR_ETOOBIG, "tensor too large");
  return SR_OK;
}

BlurArgs blur_args(const float* x, const float* taps, int r, int H, int W, float* y) {
  BlurArgs a = {};
  a.x = x, a.taps = taps, a.y = y, a.H = H, a.W = W, a.r = r;
  a.vec = W % 4 == 0 && dg_al16(y);
  return a;
}

dim3 blur_row_grid(int planes, int H, int W) { return dim3((W + BR_TW - 1) / BR_TW, (H + BR_TH - 1) / BR_TH, planes); }
dim3 blur_col_grid(int planes, int H, int W) { return dim3((W + BC_TW - 1) / BC_TW, (H + BC_TH - 1) / BC_TH, planes); }

int noise_check(const char* what, const float* img, const float* na, const float* amp, const float* out, int B, int H,
                int W) {
  if (!img || !na || !amp || !out) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(img) || !dg_al4(na) || !dg_al4(amp) || !dg_al4(out)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return dg_fail(what, SR_EINVAL, "bad arguments (1 to 65535 samples)");
  if (!dg_fits((int64_t)B * 3, H, W)) return dg_fail(what, SR_ETOOBIG, "tensor too large");
  return SR_OK;
}

}  // namespace

extern "C" {

int sr_filter2d(const float* x, int B, int C, int H, int W, const float* kernel, int kernel_batch, int k, int round255,
                float* y, void* stream) {
  const char* what = "filter2d";
  if (!x || !kernel || !y) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(x) || !dg_al4(kernel) || !dg_al4(y)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (k % 2 == 0 || k < 3 || k > 21) return dg_fail(what, SR_EINVAL, "the kernel size must be odd, 3 to 21");
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (int64_t)B * C > 65535)
    return dg_fail(what, SR_EINVAL, "bad arguments (1 to 65535 planes)");
  if (k / 2 >= H || k / 2 >= W) return dg_fail(what, SR_EINVAL, "image smaller than the reflect pad (pad < size)");
  if (x == y) return dg_fail(what, SR_EINVAL, "in-place filtering is not supported");
  if (!dg_fits((int64_t)B * C, H, W)) return dg_fail(what, SR_ETOOBIG, "tensor too large");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((W + F_TW - 1) / F_TW, (H + F_TH - 1) / F_TH, B * C);
  const int kb = kernel_batch ? 1 : 0, r = round255 ? 1 : 0;
  switch (k) {
    case 3: filter2d_launch<3>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 5: filter2d_launch<5>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 7: filter2d_launch<7>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 9: filter2d_launch<9>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 11: filter2d_launch<11>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 13: filter2d_launch<13>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 15: filter2d_launch<15>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 17: filter2d_launch<17>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    case 19: filter2d_launch<19>(grid, s, x, kernel, kb, C, H, W, r, y); break;
    default: filter2d_launch<21>(grid, s, x, kernel, kb, C, H, W, r, y); break;
  }
  return sr_check(hipGetLastError(), "filter2d launch");
}

int sr_sep_blur(const float* x, int planes, int H, int W, const float* taps, int r, float* tmp, float* y, void* stream) {
  if (int rc = blur_check("sep_blur", x, planes, H, W, taps, r, tmp, y)) return rc;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(blur_row_kernel, blur_row_grid(planes, H, W), dim3(DG_T), 0, s, blur_args(x, taps, r, H, W, tmp));
  hipLaunchKernelGGL(blur_col_kernel<0>, blur_col_grid(planes, H, W), dim3(DG_T), 0, s, blur_args(tmp, taps, r, H, W, y));
  return sr_check(hipGetLastError(), "sep_blur launch");
}

int sr_usm_sharp_launches(void) { return 4; }

int sr_usm_sharp(const float* x, int planes, int H, int W, const float* taps, int r, float weight, float threshold,
                 float* tmp, float* residual, float* mask, float* y, void* stream) {
  const char* what = "usm_sharp";
  if (int rc = blur_check(what, x, planes, H, W, taps, r, tmp, y)) return rc;
  if (!residual || !mask) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(residual) || !dg_al4(mask)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (residual == x || residual == tmp || mask == x || mask == tmp || mask == residual || y == x || y == mask ||
      y == residual)
    return dg_fail(what, SR_EINVAL, "the buffers must be distinct");
  hipStream_t s = (hipStream_t)stream;
  const dim3 rg = blur_row_grid(planes, H, W), cg = blur_col_grid(planes, H, W);
  hipLaunchKernelGGL(blur_row_kernel, rg, dim3(DG_T), 0, s, blur_args(x, taps, r, H, W, tmp));
  BlurArgs a = blur_args(tmp, taps, r, H, W, residual);
  a.img = x, a.mask = mask, a.threshold = threshold;
  hipLaunchKernelGGL(blur_col_kernel<1>, cg, dim3(DG_T), 0, s, a);
  hipLaunchKernelGGL(blur_row_kernel, rg, dim3(DG_T), 0, s, blur_args(mask, taps, r, H, W, tmp));
  BlurArgs b = blur_args(tmp, taps, r, H, W, y);
  b.img = x, b.res = residual, b.weight = weight;
  hipLaunchKernelGGL(blur_col_kernel<2>, cg, dim3(DG_T), 0, s, b);
  return sr_check(hipGetLastError(), "usm_sharp launch");
}

int sr_resize(const float* x, int planes, int Hin, int Win, int Hout, int Wout, int mode, float scale_h, float scale_w,
              float* y, void* stream) {
  const char* what = "resize";
  if (!x || !y) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(x) || !dg_al4(y)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (planes <= 0 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0) return dg_fail(what, SR_EINVAL, "bad arguments");
  if (mode != RS_AREA && mode != RS_BILINEAR && mode != RS_BICUBIC)
    return dg_fail(what, SR_EINVAL, "mode must be 0 (area), 1 (bilinear) or 2 (bicubic)");
  if (mode != RS_AREA && !(scale_h > 0.f && scale_w > 0.f)) return dg_fail(what, SR_EINVAL, "the coordinate scales must be positive");
  if (!dg_fits(planes, Hin, Win) || !dg_fits(planes, Hout, (int64_t)Wout + 3)) return dg_fail(what, SR_ETOOBIG, "tensor too large");
  ResizeArgs a = {};
  a.x = x, a.y = y, a.Hin = Hin, a.Win = Win, a.Hout = Hout, a.Wout = Wout, a.sh = scale_h, a.sw = scale_w;
  a.gpr = (Wout + 3) / 4;
  a.groups = (uint32_t)((int64_t)planes * Hout * a.gpr);
  a.vec = Wout % 4 == 0 && dg_al16(y);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(dg_grid(a.groups, 4096));
  if (mode == RS_AREA)
    hipLaunchKernelGGL(resize_kernel<RS_AREA>, grid, dim3(DG_T), 0, s, a);
  else if (mode == RS_BILINEAR)
    hipLaunchKernelGGL(resize_kernel<RS_BILINEAR>, grid, dim3(DG_T), 0, s, a);
  else
    hipLaunchKernelGGL(resize_kernel<RS_BICUBIC>, grid, dim3(DG_T), 0, s, a);
  return sr_check(hipGetLastError(), "resize launch");
}

int sr_gaussian_apply(const float* img, const float* normal, const float* normal_gray, const float* sigma,
                      const float* gray, int B, int H, int W, int finish, float* out, void* stream) {
  const char* what = "gaussian_apply";
  if (int rc = noise_check(what, img, normal, sigma, out, B, H, W)) return rc;
  if ((normal_gray == nullptr) != (gray == nullptr)) return dg_fail(what, SR_EINVAL, "normal_gray and gray go together");
  if (!dg_al4(normal_gray) || !dg_al4(gray)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  NoiseArgs a = {};
  a.img = img, a.na = normal, a.nb = normal_gray, a.amp = sigma, a.gray = gray, a.out = out;
  a.HW = H * W, a.finish = finish & 7, a.total = (uint32_t)((int64_t)B * 3 * H * W);
  hipLaunchKernelGGL(gaussian_apply_kernel, dim3(dg_grid(a.total, 2048)), dim3(DG_T), 0, (hipStream_t)stream, a);
  return sr_check(hipGetLastError(), "gaussian_apply launch");
}

int sr_level_presence(const float* img, int B, int H, int W, unsigned* bitmap, void* stream) {
  const char* what = "level_presence";
  if (!img || !bitmap) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(img) || !dg_al4(bitmap)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return dg_fail(what, SR_EINVAL, "bad arguments (1 to 65535 samples)");
  if (!dg_fits((int64_t)B * 3, H, W)) return dg_fail(what, SR_ETOOBIG, "tensor too large");
  const dim3 grid(dg_grid((uint32_t)(H * W), LP_BLOCKS), B);
  hipLaunchKernelGGL(level_presence_kernel, grid, dim3(DG_T), 0, (hipStream_t)stream, img, H * W, bitmap);
  return sr_check(hipGetLastError(), "level_presence launch");
}

int sr_poisson_rate(const float* img, const unsigned* bitmap, int B, int H, int W, float* rate_c, float* rate_g,
                    float* vals, void* stream) {
  const char* what = "poisson_rate";
  if (!img || !bitmap || !rate_c || !rate_g || !vals) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(img) || !dg_al4(bitmap) || !dg_al4(rate_c) || !dg_al4(rate_g) || !dg_al4(vals))
    return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return dg_fail(what, SR_EINVAL, "bad arguments (1 to 65535 samples)");
  if (!dg_fits((int64_t)B * 3, H, W)) return dg_fail(what, SR_ETOOBIG, "tensor too large");
  const dim3 grid(dg_grid((uint32_t)(H * W), 256), B);
  hipLaunchKernelGGL(poisson_rate_kernel, grid, dim3(DG_T), 0, (hipStream_t)stream, img, bitmap, H * W, rate_c, rate_g, vals);
  return sr_check(hipGetLastError(), "poisson_rate launch");
}

int sr_poisson_apply(const float* img, const float* draw_c, const float* draw_g, const float* vals, const float* scale,
                     const float* gray, int B, int H, int W, int finish, float* out, void* stream) {
  const char* what = "poisson_apply";
  if (int rc = noise_check(what, img, draw_c, scale, out, B, H, W)) return rc;
  if (!vals) return dg_fail(what, SR_EINVAL, "null pointer");
  if ((draw_g == nullptr) != (gray == nullptr)) return dg_fail(what, SR_EINVAL, "draw_g and gray go together");
  if (!dg_al4(draw_g) || !dg_al4(gray) || !dg_al4(vals)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  NoiseArgs a = {};
  a.img = img, a.na = draw_c, a.nb = draw_g, a.vals = vals, a.amp = scale, a.gray = gray, a.out = out;
  a.HW = H * W, a.finish = finish & 7, a.total = (uint32_t)((int64_t)B * 3 * H * W);
  hipLaunchKernelGGL(poisson_apply_kernel, dim3(dg_grid(a.total, 2048)), dim3(DG_T), 0, (hipStream_t)stream, a);
  return sr_check(hipGetLastError(), "poisson_apply launch");
}

int sr_jpeg(const float* x, int B, int H, int W, const float* quality, int differentiable, int round255, float* y,
            float* coef, void* stream) {
  const char* what = "jpeg";
  if (!x || !quality || !y) return dg_fail(what, SR_EINVAL, "null pointer");
  if (!dg_al4(x) || !dg_al4(quality) || !dg_al4(y) || !dg_al4(coef)) return dg_fail(what, SR_EINVAL, "pointers must be 4-byte aligned");
  if (B <= 0 || B > 65535 || H <= 0 || W <= 0) return dg_fail(what, SR_EINVAL, "bad arguments (1 to 65535 samples)");
  const int mbx = (W + 15) / 16, mby = (H + 15) / 16;
  if (mby > 65535 || !dg_fits((int64_t)B * 3, mby * 16, mbx * 16)) return dg_fail(what, SR_ETOOBIG, "tensor too large");
  JpegArgs a = {};
  a.x = x, a.quality = quality, a.y = y, a.coef = coef, a.H = H, a.W = W, a.mbx = mbx, a.mby = mby;
  a.differentiable = differentiable ? 1 : 0, a.round255 = round255 ? 1 : 0;
  hipLaunchKernelGGL(jpeg_kernel, dim3(mbx, mby, B), dim3(DG_T), 0, (hipStream_t)stream, a);
  return sr_check(hipGetLastError(), "jpeg launch");
}

}  // extern "C"
