// NIQE on the device: the block moments of metrics/niqe.py:niqe_moments for P planes of one fp32 NCHW
// batch in nominal [-1, 1].  Everything up to the per-block sums is streaming image work and runs here;
// the AGGD fits, the Gaussian model and the score stay on the host (metrics/niqe.py:niqe_from_moments).
//
//   sr_niqe_moments  six launches for all planes together:
//     niqe_plane_kernel    quantise to ubyte (sr_internal.h:quantise, the host's pixel values), one band or
//                          the BT.601 Y of three (in the host's precisions: fp32 / 255, float64 dot,
//                          / 255 -> fp32, * 255), border crop, round, top-left truncation to 96 x 96 blocks
//     niqe_mscn_kernel     scale 1: 7 x 7 window with replicate borders from an LDS tile with a 3-pixel halo,
//                          49 products summed in float64 in the window's raster order, mu, filter(img^2),
//                          sigma and n rounded to fp32 where the host rounds
//     niqe_half_kernel x2  half-size antialiased bicubic (8 exact taps, reflected borders): the pass along
//                          the height, fp32 store, then the pass along the width, * 255
//     niqe_mscn_kernel     scale 2
//     niqe_moments_kernel  a workgroup per (plane, scale, block): the block staged in LDS, the five maps
//                          (the block and its products with its circular rolls, by LDS indexing), float64
//                          sums and integer counts, reduced within a wave, then across the waves through
//                          LDS in a fixed order.  No atomics: two launches give identical bytes.
//
// The plane equals the host's exactly.  mu, sigma and n follow the host's operation order with individually
// rounded operations (no contraction), so they differ from the host's only where numpy's own summation
// order does (it has none here: one product per tap, added in turn).
#include "sr_common.h"
#include "sr_internal.h"

// Every product and sum below is rounded on its own, as numpy rounds them: no fused multiply-add.  The
// arithmetic is written with plain operators because the pragma governs the operations that are spelled in
// this file; the __fmul_rn / __dadd_rn family are header functions compiled with contraction allowed, and
// once inlined their product and sum may still fuse.
#pragma clang fp contract(off)

namespace {

constexpr int NQ_BLOCK = 96;    // block edge at scale 1 (48 at scale 2)
constexpr int NQ_MAXP = 64;     // planes per call (their descriptors travel in the kernel arguments)
constexpr int NQ_T = 32;        // MSCN tile edge
constexpr int NQ_HALO = 3;
constexpr int NQ_TP = NQ_T + 2 * NQ_HALO;  // staged tile edge (38)
constexpr int NQ_THREADS = 256;

struct NqPlanes {
  int n[NQ_MAXP];
  int c[NQ_MAXP][3];  // c[1] < 0: the single band c[0]
};

struct NqPlaneArgs {
  const float* x;
  int C, H, W, crop, Hb, Wb;
  double w[3], offset;
  float* plane;      // [P][Hb][Wb]
  float* plane_out;  // optional copy for the caller
  NqPlanes p;
};

__global__ __launch_bounds__(NQ_THREADS) void niqe_plane_kernel(NqPlaneArgs a) {
  const int pl = blockIdx.y;
  const int i = blockIdx.x * NQ_THREADS + threadIdx.x;
  if (i >= a.Hb * a.Wb) return;
  const int y = i / a.Wb, xx = i % a.Wb;
  const size_t hw = (size_t)a.H * a.W;
  const size_t pix = (size_t)(y + a.crop) * a.W + (xx + a.crop);
  const float* img = a.x + (size_t)a.p.n[pl] * a.C * hw;
  float v;
  if (a.p.c[pl][1] < 0) {
    // one band: an integer in [0, 255]; the host's / 255 * 255 round trip and round() give it back
    v = (float)quantise(img[(size_t)a.p.c[pl][0] * hw + pix]);
  } else {
    double yv = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float f = (float)quantise(img[(size_t)a.p.c[pl][k] * hw + pix]) / 255.f;
      const double t = (double)f * a.w[k];
      yv = k == 0 ? t : yv + t;
    }
    yv = yv + a.offset;
    const float yf = (float)(yv / 255.0);
    v = rintf(yf * 255.f);
  }
  const size_t o = (size_t)pl * a.Hb * a.Wb + i;
  a.plane[o] = v;
  if (a.plane_out) a.plane_out[o] = v;
}

struct NqMscnArgs {
  const float* src;  // [P][h][w]
  float* dst;        // [P][h][w]
  float* dst_out;    // optional copy
  int h, w, tiles_x, tiles_y;
  double win[49];    // the window convolve() correlates with (flipped by the caller's entry point)
};

__global__ __launch_bounds__(NQ_THREADS) void niqe_mscn_kernel(NqMscnArgs a) {
  __shared__ float t[NQ_TP][NQ_TP + 1];
  const int tid = threadIdx.x;
  const int tiles = a.tiles_x * a.tiles_y;
  const int pl = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int y0 = (tile / a.tiles_x) * NQ_T, x0 = (tile % a.tiles_x) * NQ_T;
  const size_t base = (size_t)pl * a.h * a.w;
  for (int i = tid; i < NQ_TP * NQ_TP; i += NQ_THREADS) {
    const int r = i / NQ_TP, c = i % NQ_TP;
    const int y = min(max(y0 + r - NQ_HALO, 0), a.h - 1), x = min(max(x0 + c - NQ_HALO, 0), a.w - 1);
    t[r][c] = a.src[base + (size_t)y * a.w + x];
  }
  __syncthreads();
  for (int i = tid; i < NQ_T * NQ_T; i += NQ_THREADS) {
    const int r = i / NQ_T, c = i % NQ_T;
    const int y = y0 + r, x = x0 + c;
    if (y >= a.h || x >= a.w) continue;
    double m = 0.0, q = 0.0;
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const float v = t[r + ky][c + kx];
        const double wv = a.win[ky * 7 + kx];
        const float v2 = v * v;  // np.square in fp32
        m = m + (double)v * wv;
        q = q + (double)v2 * wv;
      }
    }
    const float mu = (float)m, sq = (float)q;
    const float mu2 = mu * mu;
    const float sigma = sqrtf(fabsf(sq - mu2));
    const float n = (t[r + NQ_HALO][c + NQ_HALO] - mu) / (sigma + 1.f);
    const size_t o = base + (size_t)y * a.w + x;
    a.dst[o] = n;
    if (a.dst_out) a.dst_out[o] = n;
  }
}

struct NqHalfArgs {
  const float* src;  // [P][h][w]
  float* dst;        // along_w ? [P][h][w/2] : [P][h/2][w]
  int h, w, along_w;
  double tap[8];
};

// one pass of the half-size resample: dst = fp32(sum_k tap[k] * in[reflect(2o - 3 + k)]); the pass along the
// height reads src / 255 (fp32 division), the pass along the width stores * 255
__global__ __launch_bounds__(NQ_THREADS) void niqe_half_kernel(NqHalfArgs a) {
  const int pl = blockIdx.y;
  const int oh = a.along_w ? a.h : a.h / 2, ow = a.along_w ? a.w / 2 : a.w;
  const int i = blockIdx.x * NQ_THREADS + threadIdx.x;
  if (i >= oh * ow) return;
  const int y = i / ow, x = i % ow;
  const float* src = a.src + (size_t)pl * a.h * a.w;
  const int n = a.along_w ? a.w : a.h;
  const int o = a.along_w ? x : y;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int j = 2 * o - 3 + k;
    j = j < 0 ? -j - 1 : j;
    j = j >= n ? 2 * n - 1 - j : j;
    float v = a.along_w ? src[(size_t)y * a.w + j] : src[(size_t)j * a.w + x];
    if (!a.along_w) v = v / 255.f;
    acc = acc + (double)v * a.tap[k];
  }
  float r = (float)acc;
  if (a.along_w) r = r * 255.f;
  a.dst[(size_t)pl * oh * ow + i] = r;
}

struct NqMomArgs {
  const float* n1;  // scale-1 MSCN [P][Hb][Wb]
  const float* n2;  // scale-2 MSCN [P][Hb/2][Wb/2]
  int Hb, Wb, bh, bw;
  double* out;      // [P][2][bh][bw][5][6]
};

SR_DEV double nq_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(NQ_THREADS) void niqe_moments_kernel(NqMomArgs a) {
  __shared__ float blk[NQ_BLOCK * NQ_BLOCK];
  __shared__ double red[NQ_THREADS / 64][6];
  const int tid = threadIdx.x;
  const int nb = a.bh * a.bw;
  const int pl = blockIdx.x / (2 * nb);
  const int s = (blockIdx.x / nb) % 2;
  const int b = blockIdx.x % nb;
  const int by = b / a.bw, bx = b % a.bw;
  const int bs = NQ_BLOCK >> s;
  const int h = a.Hb >> s, w = a.Wb >> s;
  const float* src = (s ? a.n2 : a.n1) + (size_t)pl * h * w + (size_t)by * bs * w + (size_t)bx * bs;
  for (int i = tid; i < bs * bs; i += NQ_THREADS) blk[i] = src[(size_t)(i / bs) * w + (i % bs)];
  __syncthreads();
  double* out = a.out + ((size_t)blockIdx.x) * 30;  // blockIdx.x = ((pl * 2 + s) * bh + by) * bw + bx
  for (int m = 0; m < 5; ++m) {
    // rolled[i][j] = block[(i - s0) mod bs][(j - s1) mod bs], shifts (0,1), (1,0), (1,1), (1,-1)
    const int s0 = m >= 2 ? 1 : 0;
    const int s1 = m == 1 || m == 3 ? 1 : (m == 4 ? -1 : 0);
    int nneg = 0, npos = 0;
    double ssn = 0.0, ssp = 0.0, sab = 0.0, ssq = 0.0;
    for (int i = tid; i < bs * bs; i += NQ_THREADS) {
      const int r = i / bs, c = i % bs;
      float v = blk[i];
      if (m > 0) {
        const int rr = r - s0 < 0 ? r - s0 + bs : r - s0;
        int cc = c - s1;
        cc = cc < 0 ? cc + bs : (cc >= bs ? cc - bs : cc);
        v = v * blk[rr * bs + cc];
      }
      const double d = (double)v;
      const double d2 = d * d;
      if (v < 0.f) {
        ++nneg;
        ssn = ssn + d2;
      } else if (v > 0.f) {
        ++npos;
        ssp = ssp + d2;
      }
      sab = sab + fabs(d);
      ssq = ssq + d2;
    }
    double v6[6] = {(double)nneg, ssn, (double)npos, ssp, sab, ssq};
#pragma unroll
    for (int k = 0; k < 6; ++k) v6[k] = nq_wave_sum(v6[k]);
    if ((tid & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 6; ++k) red[tid >> 6][k] = v6[k];
    }
    __syncthreads();
    if (tid < 6) {
      double t = red[0][tid];
      for (int wv = 1; wv < NQ_THREADS / 64; ++wv) t = t + red[wv][tid];
      out[m * 6 + tid] = t;
    }
    __syncthreads();
  }
}

// block rows / columns after the crop; false when the arguments are outside the envelope
bool nq_geometry(int N, int C, int H, int W, int crop, int P, int* bh, int* bw) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || crop < 0 || P < 1 || P > NQ_MAXP) return false;
  const int64_t hc = (int64_t)H - 2 * (int64_t)crop, wc = (int64_t)W - 2 * (int64_t)crop;
  if (hc < NQ_BLOCK || wc < NQ_BLOCK) return false;
  *bh = (int)(hc / NQ_BLOCK), *bw = (int)(wc / NQ_BLOCK);
  // every index below stays in int: planes * pixels and the grids
  if ((int64_t)P * *bh * *bw * NQ_BLOCK * NQ_BLOCK > 0x7fffffff) return false;
  return true;
}

}  // namespace

extern "C" {

size_t sr_niqe_moments_workspace(int N, int C, int H, int W, int crop, int P) {
  int bh, bw;
  if (!nq_geometry(N, C, H, W, crop, P, &bh, &bw)) return 0;
  // plane, scale-1 MSCN, height-pass image (1/2), half-size plane (1/4), scale-2 MSCN (1/4)
  return (size_t)P * bh * bw * NQ_BLOCK * NQ_BLOCK * 3 * sizeof(float);
}

int sr_niqe_moments(const float* x, int N, int C, int H, int W, int crop, int P, const int* plane_desc,
                    const double* y_coef, const double* window, double* moments, float* planes_out, float* mscn_out,
                    void* ws, size_t ws_bytes, void* stream) {
  if (!x || !plane_desc || !window || !moments || !ws) return sr_fail(SR_EINVAL, "niqe_moments: null pointer");
  if (N < 1 || C < 1 || H < 1 || W < 1) return sr_fail(SR_EINVAL, "niqe_moments: N, C, H, W must be >= 1");
  if (crop < 0) return sr_fail(SR_EINVAL, "niqe_moments: crop must be >= 0");
  if (P < 1 || P > NQ_MAXP) return sr_fail(SR_EINVAL, "niqe_moments: 1 to 64 planes per call");
  if ((int64_t)H - 2 * (int64_t)crop < NQ_BLOCK || (int64_t)W - 2 * (int64_t)crop < NQ_BLOCK)
    return sr_fail(SR_EINVAL, "niqe_moments: H and W after the crop must be at least 96");
  int bh, bw;
  if (!nq_geometry(N, C, H, W, crop, P, &bh, &bw)) return sr_fail(SR_ETOOBIG, "niqe_moments: too many pixels");
  if (ws_bytes < sr_niqe_moments_workspace(N, C, H, W, crop, P))
    return sr_fail(SR_EINVAL, "niqe_moments: workspace too small");
  if ((uintptr_t)ws & 3) return sr_fail(SR_EINVAL, "niqe_moments: workspace must be 4-byte aligned");

  NqPlaneArgs pa;
  bool any_y = false;
  for (int p = 0; p < P; ++p) {
    const int* d = plane_desc + 4 * p;
    if (d[0] < 0 || d[0] >= N) return sr_fail(SR_EINVAL, "niqe_moments: image index out of range");
    const bool single = d[2] < 0 && d[3] < 0;
    for (int k = 0; k < (single ? 1 : 3); ++k)
      if (d[1 + k] < 0 || d[1 + k] >= C) return sr_fail(SR_EINVAL, "niqe_moments: channel index out of range");
    any_y |= !single;
    pa.p.n[p] = d[0];
    pa.p.c[p][0] = d[1], pa.p.c[p][1] = single ? -1 : d[2], pa.p.c[p][2] = single ? -1 : d[3];
  }
  if (any_y && !y_coef) return sr_fail(SR_EINVAL, "niqe_moments: a three-channel plane needs y_coef");

  const int Hb = bh * NQ_BLOCK, Wb = bw * NQ_BLOCK;
  const size_t px = (size_t)Hb * Wb;
  float* plane1 = (float*)ws;
  float* mscn1 = plane1 + (size_t)P * px;
  float* halfh = mscn1 + (size_t)P * px;
  float* plane2 = halfh + (size_t)P * px / 2;
  float* mscn2 = plane2 + (size_t)P * px / 4;
  hipStream_t s = (hipStream_t)stream;

  pa.x = x, pa.C = C, pa.H = H, pa.W = W, pa.crop = crop, pa.Hb = Hb, pa.Wb = Wb;
  for (int k = 0; k < 3; ++k) pa.w[k] = y_coef ? y_coef[k] : 0.0;
  pa.offset = y_coef ? y_coef[3] : 0.0;
  pa.plane = plane1, pa.plane_out = planes_out;
  hipLaunchKernelGGL(niqe_plane_kernel, dim3((unsigned)((px + NQ_THREADS - 1) / NQ_THREADS), (unsigned)P), dim3(NQ_THREADS),
                     0, s, pa);
  if (int rc = sr_check(hipGetLastError(), "niqe plane launch")) return rc;

  NqMscnArgs ma;
  // convolve() correlates with the flipped window
  for (int i = 0; i < 49; ++i) ma.win[i] = window[48 - i];
  ma.src = plane1, ma.dst = mscn1, ma.dst_out = mscn_out;
  ma.h = Hb, ma.w = Wb, ma.tiles_x = (Wb + NQ_T - 1) / NQ_T, ma.tiles_y = (Hb + NQ_T - 1) / NQ_T;
  hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)(P * ma.tiles_x * ma.tiles_y)), dim3(NQ_THREADS), 0, s, ma);
  if (int rc = sr_check(hipGetLastError(), "niqe mscn launch")) return rc;

  NqHalfArgs ha;
  const double taps[8] = {-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625,
                          -0.01171875};
  for (int k = 0; k < 8; ++k) ha.tap[k] = taps[k];
  ha.src = plane1, ha.dst = halfh, ha.h = Hb, ha.w = Wb, ha.along_w = 0;
  hipLaunchKernelGGL(niqe_half_kernel, dim3((unsigned)((px / 2 + NQ_THREADS - 1) / NQ_THREADS), (unsigned)P),
                     dim3(NQ_THREADS), 0, s, ha);
  if (int rc = sr_check(hipGetLastError(), "niqe half (height) launch")) return rc;
  ha.src = halfh, ha.dst = plane2, ha.h = Hb / 2, ha.w = Wb, ha.along_w = 1;
  hipLaunchKernelGGL(niqe_half_kernel, dim3((unsigned)((px / 4 + NQ_THREADS - 1) / NQ_THREADS), (unsigned)P),
                     dim3(NQ_THREADS), 0, s, ha);
  if (int rc = sr_check(hipGetLastError(), "niqe half (width) launch")) return rc;

  ma.src = plane2, ma.dst = mscn2, ma.dst_out = nullptr;
  ma.h = Hb / 2, ma.w = Wb / 2, ma.tiles_x = (ma.w + NQ_T - 1) / NQ_T, ma.tiles_y = (ma.h + NQ_T - 1) / NQ_T;
  hipLaunchKernelGGL(niqe_mscn_kernel, dim3((unsigned)(P * ma.tiles_x * ma.tiles_y)), dim3(NQ_THREADS), 0, s, ma);
  if (int rc = sr_check(hipGetLastError(), "niqe mscn (scale 2) launch")) return rc;

  NqMomArgs mo;
  mo.n1 = mscn1, mo.n2 = mscn2, mo.Hb = Hb, mo.Wb = Wb, mo.bh = bh, mo.bw = bw, mo.out = moments;
  hipLaunchKernelGGL(niqe_moments_kernel, dim3((unsigned)(P * 2 * bh * bw)), dim3(NQ_THREADS), 0, s, mo);
  return sr_check(hipGetLastError(), "niqe moments launch");
}

}  // extern "C"
