// Deformable convolution, the any-shape column path (sr_dcn_im2col, sr_dcn_col2im): two batched HBM-bound
// passes around MFMA GEMMs (the GEMMs are the 1x1 path of the conv code).
//   dcn_im2col_kernel     : cols[p][g][tap][ci] = mask * bilinear(x, p + tap + offset), all images in one
//                           launch, pixel-major rows so the GEMM reads them as a K-contiguous operand; x is
//                           NHWC so each bilinear corner is a 16-byte channel vector.
//   dcn_coord_grad_kernel : col2im_coord, the offset and mask gradients: one item per (pixel, tap,
//                           deformable group) reducing over the group's channels in registers, no atomics.
//   dcn_grad_x_kernel     : col2im, the bilinear scatter accumulated in an LDS image of the output tile's
//                           input footprint, flushed with channel-contiguous atomics.
// Offsets and masks are staged through LDS per pixel tile so their NCHW reads and writes stay coalesced
// while the item loop runs deformable-group-fastest (adjacent lanes touch adjacent channel vectors of the
// same pixel).
#include "dcn_dev.h"

namespace sr_dcn {
namespace {

template <typename T, int V>
__global__ void __launch_bounds__(256) dcn_im2col_kernel(DcnArgs a, const T* __restrict__ x,
                                                         const float* __restrict__ off, const float* __restrict__ msk,
                                                         T* __restrict__ cols) {
  extern __shared__ float s_lds[];
  float* s_off = s_lds;
  float* s_msk = s_lds + a.DG * 2 * a.K * a.TP;
  const int HWo = a.Ho * a.Wo;
  const int tiles = (HWo + a.TP - 1) / a.TP;
  const int n = blockIdx.x / tiles, p0 = (blockIdx.x - n * tiles) * a.TP;
  const int np = min(a.TP, HWo - p0);
  load_tile(s_off, s_msk, off, msk, a, n, p0, np);
  __syncthreads();
  const T* xim = x + (int64_t)n * a.H * a.W * a.Cp;
  const int items = np * a.K * a.DG;
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int dgi = it % a.DG, t2 = it / a.DG, tap = t2 % a.K, px = t2 / a.K;
    const int p = p0 + px, ho = p / a.Wo, wo = p - ho * a.Wo;
    const int i = tap / a.kw, j = tap - i * a.kw;
    const float oh = s_off[(dgi * 2 * a.K + 2 * tap) * a.TP + px];
    const float ow = s_off[(dgi * 2 * a.K + 2 * tap + 1) * a.TP + px];
    const float m = s_msk[(dgi * a.K + tap) * a.TP + px];
    const float h = (float)(ho * a.sh - a.ph + i * a.dh) + oh;
    const float w = (float)(wo * a.sw - a.pw + j * a.dw) + ow;
    const Sample s = make_sample(h, w, a.H, a.W);
    const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
    T* row = cols + ((int64_t)n * HWo + p) * a.L;
    for (int c = dgi * a.cpg; c < (dgi + 1) * a.cpg; c += V) {
      float v1[V], v2[V], v3[V], v4[V], r[V];
#pragma unroll
      for (int e = 0; e < V; ++e) v1[e] = v2[e] = v3[e] = v4[e] = 0.f;
      if (s.o1 >= 0) Vec<T, V>::load(xim + (int64_t)s.o1 * a.Cp + c, v1);
      if (s.o2 >= 0) Vec<T, V>::load(xim + (int64_t)s.o2 * a.Cp + c, v2);
      if (s.o3 >= 0) Vec<T, V>::load(xim + (int64_t)s.o3 * a.Cp + c, v3);
      if (s.o4 >= 0) Vec<T, V>::load(xim + (int64_t)s.o4 * a.Cp + c, v4);
#pragma unroll
      for (int e = 0; e < V; ++e) r[e] = (w1 * v1[e] + w2 * v2[e] + w3 * v3[e] + w4 * v4[e]) * m;
      const int g = c / a.cg, ci = c - g * a.cg;
      Vec<T, V>::store(row + (g * a.K + tap) * a.cgp + ci, r);
    }
  }
  if (a.cgp != a.cg) {  // zero the per-group channel padding of the column rows
    const int padc = a.cgp - a.cg, per = a.G * a.K * padc;
    for (int it = threadIdx.x; it < np * per; it += blockDim.x) {
      const int px = it / per, r = it - px * per, gt = r / padc, ci = a.cg + r - gt * padc;
      cols[((int64_t)n * HWo + p0 + px) * a.L + gt * a.cgp + ci] = Elt<T>::from_f(0.f);
    }
  }
}

// Offset / mask gradients (col2im_coord, deform_conv_cuda_kernel.cu:696-770): one item
// per (pixel, tap, deformable group) walks the group's channels once and reduces in
// registers; results replace the item's own LDS words and are stored coalesced.
template <typename T, int V>
__global__ void __launch_bounds__(256) dcn_coord_grad_kernel(DcnArgs a, const T* __restrict__ dcols,
                                                             const T* __restrict__ x, const float* __restrict__ off,
                                                             const float* __restrict__ msk, float* __restrict__ goff,
                                                             float* __restrict__ gmsk, unsigned* __restrict__ amax) {
  extern __shared__ float s_lds[];
  float* s_off = s_lds;
  float* s_msk = s_lds + a.DG * 2 * a.K * a.TP;
  const int HWo = a.Ho * a.Wo;
  const int tiles = (HWo + a.TP - 1) / a.TP;
  const int n = blockIdx.x / tiles, p0 = (blockIdx.x - n * tiles) * a.TP;
  const int np = min(a.TP, HWo - p0);
  load_tile(s_off, s_msk, off, msk, a, n, p0, np);
  __syncthreads();
  const T* xim = x + (int64_t)n * a.H * a.W * a.Cp;
  const int items = np * a.K * a.DG;
  float vmax = 0.f;  // max |mask * dcols| over the samples this block scatters (grad_x scale)
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int dgi = it % a.DG, t2 = it / a.DG, tap = t2 % a.K, px = t2 / a.K;
    const int p = p0 + px, ho = p / a.Wo, wo = p - ho * a.Wo;
    const int i = tap / a.kw, j = tap - i * a.kw;
    float* ph = &s_off[(dgi * 2 * a.K + 2 * tap) * a.TP + px];
    float* pw = &s_off[(dgi * 2 * a.K + 2 * tap + 1) * a.TP + px];
    float* pm = &s_msk[(dgi * a.K + tap) * a.TP + px];
    const float m = *pm;
    const float h = (float)(ho * a.sh - a.ph + i * a.dh) + *ph;
    const float w = (float)(wo * a.sw - a.pw + j * a.dw) + *pw;
    const Sample s = make_sample(h, w, a.H, a.W);
    float acc_h = 0.f, acc_w = 0.f, acc_m = 0.f;
    if (s.valid) {
      const float w1 = s.hh * s.hw, w2 = s.hh * s.lw, w3 = s.lh * s.hw, w4 = s.lh * s.lw;
      const T* row = dcols + ((int64_t)n * HWo + p) * a.L;
      for (int c = dgi * a.cpg; c < (dgi + 1) * a.cpg; c += V) {
        float v1[V], v2[V], v3[V], v4[V], dc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) v1[e] = v2[e] = v3[e] = v4[e] = 0.f;
        const int g = c / a.cg, ci = c - g * a.cg;
        Vec<T, V>::load(row + (g * a.K + tap) * a.cgp + ci, dc);
        if (s.o1 >= 0) Vec<T, V>::load(xim + (int64_t)s.o1 * a.Cp + c, v1);
        if (s.o2 >= 0) Vec<T, V>::load(xim + (int64_t)s.o2 * a.Cp + c, v2);
        if (s.o3 >= 0) Vec<T, V>::load(xim + (int64_t)s.o3 * a.Cp + c, v3);
        if (s.o4 >= 0) Vec<T, V>::load(xim + (int64_t)s.o4 * a.Cp + c, v4);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          // d bilinear / d h and d w (dmcn_get_coordinate_weight, :527-569) and the
          // un-masked sample for the mask gradient
          const float wh = -s.hw * v1[e] - s.lw * v2[e] + s.hw * v3[e] + s.lw * v4[e];
          const float ww = -s.hh * v1[e] + s.hh * v2[e] - s.lh * v3[e] + s.lh * v4[e];
          acc_h += wh * dc[e] * m;
          acc_w += ww * dc[e] * m;
          acc_m += dc[e] * (w1 * v1[e] + w2 * v2[e] + w3 * v3[e] + w4 * v4[e]);
          vmax = fmaxf(vmax, fabsf(dc[e] * m));
          if (!(fabsf(dc[e] * m) <= 3.0e38f)) vmax = __builtin_inff();  // NaN / inf: grad_x falls back
        }
      }
    }
    // each item owns exactly the LDS words it read: overwrite them with its gradients
    *ph = acc_h;
    *pw = acc_w;
    *pm = acc_m;
  }
  // block max -> per-image max (non-negative floats order like their bit patterns)
  for (int o = 32; o > 0; o >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, o));
  if ((threadIdx.x & 63) == 0 && vmax > 0.f) atomicMax(amax + n, __float_as_uint(vmax));
  __syncthreads();
  const int noff = a.DG * 2 * a.K, nm = a.DG * a.K;
  for (int q = threadIdx.x; q < (noff + nm) * a.TP; q += blockDim.x) {
    const int ch = q / a.TP, px = q - ch * a.TP;
    if (px >= np) continue;
    if (ch < noff) goff[((int64_t)n * noff + ch) * HWo + p0 + px] = s_off[ch * a.TP + px];
    else if (gmsk) gmsk[((int64_t)n * nm + ch - noff) * HWo + p0 + px] = s_msk[(ch - noff) * a.TP + px];
  }
}

// grad_x (col2im, :636-694): scatter mask * dcols to the four bilinear corners.  The
// workgroup owns a 2-D output tile; every corner that falls into the tile's input
// footprint (+ a halo of R pixels for the offsets) accumulates in an LDS image of CPP
// channels, and the footprint is flushed once per channel pass with channel-contiguous
// (coalesced) global fp32 atomics.  Corners outside the footprint (offsets larger than the
// halo) go straight to global atomics, so the result never depends on the offset range.
//
// LDS accumulation is int64 fixed point (ds_add_u64): fp32 LDS atomics run at ~1/25 of
// the integer rate on gfx950 (tools/lds_atomic_bench.hip, tools/atomic_bench2.hip).  The
// per-image scale 2^e puts max |mask * dcols| (from the coordinate kernel) below 2^48, so a
// cell sum of <= 2^14 contributions cannot overflow and the in-block sum is exact to
// 2^-48 of the largest term (finer than fp32 accumulation) and order independent.
// Non-finite gradients (max = inf) use direct fp32 atomics to propagate NaN / inf.
template <typename T, int V>
__global__ void __launch_bounds__(256) dcn_grad_x_kernel(DcnArgs a, XGeom xg, const T* __restrict__ dcols,
                                                         const float* __restrict__ off, const float* __restrict__ msk,
                                                         const unsigned* __restrict__ amax, float* __restrict__ gx) {
  extern __shared__ unsigned long long s_acc[];  // [RH*RW][CPP+1]
  const int HWo = a.Ho * a.Wo;
  const int tw = (a.Wo + xg.TT - 1) / xg.TT, th = (a.Ho + xg.TT - 1) / xg.TT;
  const int n = blockIdx.x / (tw * th), t = blockIdx.x - n * (tw * th);
  const float mx = __uint_as_float(amax[n]);
  if (mx == 0.f) return;  // nothing of this image is scattered (uniform per block)
  const bool direct = !(mx <= 3.0e38f);
  int ex = 0;
  frexpf(direct ? 1.f : mx, &ex);
  const int e = min(127, 48 - ex);
  const float sc = ldexpf(1.f, e), isc = ldexpf(1.f, -e);
  const int ho0 = (t / tw) * xg.TT, wo0 = (t - (t / tw) * tw) * xg.TT;
  const int ry0 = ho0 * a.sh - a.ph - xg.R, rx0 = wo0 * a.sw - a.pw - xg.R;
  const int RP = xg.RH * xg.RW, ST = xg.CPP + 1;
  const int npx = xg.TT * xg.TT, nvec = xg.CPP / V;
  float* gim = gx + (int64_t)n * a.H * a.W * a.Cp;
  for (int c0 = 0; c0 < a.C; c0 += xg.CPP) {
    for (int i = threadIdx.x; i < RP * ST; i += blockDim.x) s_acc[i] = 0ull;
    __syncthreads();
    const int items = npx * nvec * a.K;
    for (int it = threadIdx.x; it < items; it += blockDim.x) {
      const int px = it % npx, r = it / npx, cv = r % nvec, tap = r / nvec;
      const int ho = ho0 + px / xg.TT, wo = wo0 + px % xg.TT;
      const int c = c0 + cv * V;
      if (ho >= a.Ho || wo >= a.Wo || c >= a.C) continue;
      const int p = ho * a.Wo + wo;
      const int dgi = c / a.cpg, g = c / a.cg, ci = c - g * a.cg;
      const int i = tap / a.kw, j = tap - i * a.kw;
      const float oh = off[(((int64_t)n * a.DG + dgi) * 2 * a.K + 2 * tap) * HWo + p];
      const float ow = off[(((int64_t)n * a.DG + dgi) * 2 * a.K + 2 * tap + 1) * HWo + p];
      const float m = msk ? msk[(((int64_t)n * a.DG + dgi) * a.K + tap) * HWo + p] : 1.f;
      const float h = (float)(ho * a.sh - a.ph + i * a.dh) + oh;
      const float w = (float)(wo * a.sw - a.pw + j * a.dw) + ow;
      const Sample s = make_sample(h, w, a.H, a.W);
      if (!s.valid) continue;
      float dc[V];
      Vec<T, V>::load(dcols + ((int64_t)n * HWo + p) * a.L + (g * a.K + tap) * a.cgp + ci, dc);
      const int hl = (int)floorf(h), wl = (int)floorf(w);
      const float wt[4] = {s.hh * s.hw, s.hh * s.lw, s.lh * s.hw, s.lh * s.lw};
      const int oo[4] = {s.o1, s.o2, s.o3, s.o4};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (oo[q] < 0) continue;
        const int ly = hl + (q >> 1) - ry0, lx = wl + (q & 1) - rx0;
        if (!direct && ly >= 0 && ly < xg.RH && lx >= 0 && lx < xg.RW) {
          unsigned long long* dst = s_acc + (ly * xg.RW + lx) * ST + cv * V;
#pragma unroll
          for (int e2 = 0; e2 < V; ++e2)
            atomicAdd(dst + e2, (unsigned long long)__float2ll_rn(wt[q] * (dc[e2] * m) * sc));
        } else {
          float* dst = gim + (int64_t)oo[q] * a.Cp + c;
#pragma unroll
          for (int e2 = 0; e2 < V; ++e2) unsafeAtomicAdd(dst + e2, wt[q] * (dc[e2] * m));
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < RP * xg.CPP; i += blockDim.x) {
      const int pix = i / xg.CPP, ch = i - pix * xg.CPP;
      const int yy = ry0 + pix / xg.RW, xx = rx0 + pix % xg.RW;
      if (yy < 0 || yy >= a.H || xx < 0 || xx >= a.W || c0 + ch >= a.C) continue;
      const long long v = (long long)s_acc[pix * ST + ch];
      if (v != 0) unsafeAtomicAdd(gim + ((int64_t)yy * a.W + xx) * a.Cp + c0 + ch, (float)v * isc);
    }
    __syncthreads();
  }
}

// vector width: 16-byte channel vectors when every group boundary is vector aligned
template <typename T> int vec_width(const DcnArgs& a) {
  const int v = Elt<T>::PER16;
  return (a.cpg % v == 0 && a.cg % v == 0) ? v : 1;
}

// The launches at vector width V (Elt<T>::PER16 or 1); the launchers below choose it once per call.
template <typename T, int V>
int im2col(const DcnArgs& a, const void* x, const float* off, const float* msk, void* cols, hipStream_t s) {
  const int tiles = (a.Ho * a.Wo + a.TP - 1) / a.TP;
  const size_t lds = (size_t)a.DG * 3 * a.K * a.TP * 4;
  hipLaunchKernelGGL((dcn_im2col_kernel<T, V>), dim3((unsigned)(a.N * tiles)), dim3(256), lds, s, a, (const T*)x, off,
                     msk, (T*)cols);
  return sr_check(hipGetLastError(), "dcn_im2col launch");
}

template <typename T, int V>
int col2im(const DcnArgs& a, const XGeom& xg, const void* dcols, const void* x, const float* off, const float* msk,
           float* gx, float* goff, float* gmsk, unsigned* amax, hipStream_t s, bool coord) {
  if (coord) {  // else the coordinate pass (and amax) ran already (dcn_coord_win_kernel)
    const int tiles = (a.Ho * a.Wo + a.TP - 1) / a.TP;
    const size_t lds = (size_t)a.DG * 3 * a.K * a.TP * 4;
    hipLaunchKernelGGL((dcn_coord_grad_kernel<T, V>), dim3((unsigned)(a.N * tiles)), dim3(256), lds, s, a,
                       (const T*)dcols, (const T*)x, off, msk, goff, gmsk, amax);
    if (hipGetLastError() != hipSuccess) return sr_fail(SR_ELAUNCH, "dcn_coord_grad launch");
  }
  const auto kernel = dcn_grad_x_kernel<T, V>;
  const int xt = ((a.Ho + xg.TT - 1) / xg.TT) * ((a.Wo + xg.TT - 1) / xg.TT);
  const size_t xlds = (size_t)xg.RH * xg.RW * (xg.CPP + 1) * 8;
  if (xlds > 65536 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)xlds) != hipSuccess)
    return sr_fail(SR_ELAUNCH, "dcn_col2im: LDS attribute");
  hipLaunchKernelGGL(kernel, dim3((unsigned)(a.N * xt)), dim3(256), xlds, s, a, xg, (const T*)dcols, off, msk, amax,
                     gx);
  return sr_check(hipGetLastError(), "dcn_col2im launch");
}

}  // namespace

int launch_im2col(const DcnArgs& a, bool bf16, const void* x, const float* off, const float* msk, void* cols,
                  hipStream_t s) {
  if (bf16) return (vec_width<bf16_t>(a) > 1 ? im2col<bf16_t, 8> : im2col<bf16_t, 1>)(a, x, off, msk, cols, s);
  return (vec_width<float>(a) > 1 ? im2col<float, 4> : im2col<float, 1>)(a, x, off, msk, cols, s);
}

int launch_col2im(const DcnArgs& a, const XGeom& xg, bool bf16, const void* dcols, const void* x, const float* off,
                  const float* msk, float* gx, float* goff, float* gmsk, unsigned* amax, hipStream_t s, bool coord) {
  const auto f = bf16 ? (vec_width<bf16_t>(a) > 1 ? col2im<bf16_t, 8> : col2im<bf16_t, 1>)
                      : (vec_width<float>(a) > 1 ? col2im<float, 4> : col2im<float, 1>);
  return f(a, xg, dcols, x, off, msk, gx, goff, gmsk, amax, s, coord);
}

}  // namespace sr_dcn
