// Validation metrics on the device: per (image, channel) the integer sum of squared ubyte differences
// (PSNR) and the mean of the 11 x 11 Gaussian SSIM map, from the [-1, 1] fp32 NCHW network output and
// ground truth.  The device form of metrics/psnr_ssim.py on the images
// utils/img_util.py:minusone_one_tensor_to_ubyte_numpy makes.
//
//   sr_val_metrics  one launch of val_metrics_kernel (a block per (n, c, 32 x 32 tile of the SSIM map))
//                   and one of val_metrics_finish_kernel (a block per (n, c), fixed-order reduction of
//                   the tile partials in the workspace).  No atomics: two runs are bit-identical.
//
// A block quantises its 42 x 42 pixels (tile + the 10-pixel apron of the valid-mode window) of both
// images to ubyte into LDS: clamp to [-1, 1], (t + 1) * 0.5, * 255 with individually rounded fp32
// operations (no contraction), round half to even, clip -- bit for bit the host's values, so the
// squared-difference sum is the host's integer.  The SSIM moments a, b, a^2, b^2, ab are filtered in
// float64 in the host's order (_filter_valid: down the rows first, then along them, every product and
// sum rounded separately, no contraction), which keeps the result within a few 1e-16 of the host's on
// ordinary images and 2e-13 on bright, flat ones (measured; the final mean is summed in another order).
// float64 because sigma^2 = E[x^2] - mu^2 cancels ~5 digits on bright, flat tiles.
// Pixels of the crop are owned by exactly one tile for the squared-difference sum: a tile owns its
// first 32 rows / columns, the last tile of a row / column of tiles also owns its apron.
#include "sr_common.h"
#include "sr_internal.h"

#include <cmath>

namespace {

constexpr int VM_T = 32;             // SSIM map tile edge
constexpr int VM_K = 11;             // window taps
constexpr int VM_P = VM_T + VM_K - 1;  // staged pixel tile edge (42)
constexpr int VM_THREADS = 256;

struct VmArgs {
  const float* sr;
  const float* gt;
  int H, W, crop, Hc, Wc;
  int mh, mw;  // SSIM map size (Hc - 10, Wc - 10; < 1: no map)
  int tiles_x, tiles_y;
  double w[VM_K];
  double c1, c2;
  double* part_ssim;         // [N*C][tiles]
  unsigned long long* part_sse;  // [N*C][tiles]
};

__global__ __launch_bounds__(VM_THREADS) void val_metrics_kernel(VmArgs a) {
  __shared__ unsigned char pa[VM_P * VM_P], pb[VM_P * VM_P];
  __shared__ double V[5][VM_T][VM_P];  // the five moments filtered down the rows
  __shared__ double red[VM_THREADS];
  __shared__ unsigned int redi[VM_THREADS];

  const int tid = threadIdx.x;
  const int tiles = a.tiles_x * a.tiles_y;
  const int nc = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int ty = tile / a.tiles_x, tx = tile % a.tiles_x;
  const int y0 = ty * VM_T, x0 = tx * VM_T;  // tile origin inside the crop
  const bool last_y = ty == a.tiles_y - 1, last_x = tx == a.tiles_x - 1;
  const size_t plane = (size_t)nc * a.H * a.W;

  unsigned int sse = 0;
  for (int i = tid; i < VM_P * VM_P; i += VM_THREADS) {
    const int r = i / VM_P, c = i % VM_P;
    const int y = y0 + r, x = x0 + c;
    unsigned char qa = 0, qb = 0;
    if (y < a.Hc && x < a.Wc) {
      const size_t off = plane + (size_t)(y + a.crop) * a.W + (x + a.crop);
      qa = quantise(a.sr[off]);
      qb = quantise(a.gt[off]);
      if ((r < VM_T || last_y) && (c < VM_T || last_x)) {
        const int d = (int)qa - (int)qb;
        sse += (unsigned int)(d * d);
      }
    }
    pa[i] = qa;
    pb[i] = qb;
  }
  __syncthreads();

  double acc = 0.0;
  if (a.mh >= 1 && a.mw >= 1) {
    for (int i = tid; i < VM_T * VM_P; i += VM_THREADS) {
      const int y = i / VM_P, c = i % VM_P;
      double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
#pragma unroll
      for (int k = 0; k < VM_K; ++k) {
        const double p = (double)pa[(y + k) * VM_P + c], q = (double)pb[(y + k) * VM_P + c];
        const double w = a.w[k];
        m0 = __dadd_rn(m0, __dmul_rn(w, p));
        m1 = __dadd_rn(m1, __dmul_rn(w, q));
        m2 = __dadd_rn(m2, __dmul_rn(w, p * p));  // integer products: exact
        m3 = __dadd_rn(m3, __dmul_rn(w, q * q));
        m4 = __dadd_rn(m4, __dmul_rn(w, p * q));
      }
      V[0][y][c] = m0, V[1][y][c] = m1, V[2][y][c] = m2, V[3][y][c] = m3, V[4][y][c] = m4;
    }
    __syncthreads();
    const int oh = min(VM_T, a.mh - y0), ow = min(VM_T, a.mw - x0);
    for (int i = tid; i < VM_T * VM_T; i += VM_THREADS) {
      const int y = i / VM_T, x = i % VM_T;
      if (y >= oh || x >= ow) continue;
      double m[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < VM_K; ++k) s = __dadd_rn(s, __dmul_rn(a.w[k], V[j][y][x + k]));
        m[j] = s;
      }
      const double mu1_sq = __dmul_rn(m[0], m[0]), mu2_sq = __dmul_rn(m[1], m[1]), mu12 = __dmul_rn(m[0], m[1]);
      const double s1 = __dadd_rn(m[2], -mu1_sq), s2 = __dadd_rn(m[3], -mu2_sq), s12 = __dadd_rn(m[4], -mu12);
      const double num = __dmul_rn(__dadd_rn(__dmul_rn(2.0, mu12), a.c1), __dadd_rn(__dmul_rn(2.0, s12), a.c2));
      const double den = __dmul_rn(__dadd_rn(__dadd_rn(mu1_sq, mu2_sq), a.c1), __dadd_rn(__dadd_rn(s1, s2), a.c2));
      acc = __dadd_rn(acc, __ddiv_rn(num, den));
    }
  }

  red[tid] = acc;
  redi[tid] = sse;
  __syncthreads();
  for (int s = VM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] = __dadd_rn(red[tid], red[tid + s]);
      redi[tid] += redi[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.part_ssim[blockIdx.x] = red[0];
    a.part_sse[blockIdx.x] = redi[0];
  }
}

constexpr int VF_THREADS = 64;

__global__ __launch_bounds__(VF_THREADS) void val_metrics_finish_kernel(const double* __restrict__ part_ssim,
                                                                        const unsigned long long* __restrict__ part_sse,
                                                                        int tiles, int mh, int mw,
                                                                        long long* __restrict__ sse,
                                                                        double* __restrict__ ssim) {
  __shared__ double red[VF_THREADS];
  __shared__ unsigned long long redi[VF_THREADS];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * tiles;
  double acc = 0.0;
  unsigned long long e = 0;
  for (int t = tid; t < tiles; t += VF_THREADS) {
    acc = __dadd_rn(acc, part_ssim[base + t]);
    e += part_sse[base + t];
  }
  red[tid] = acc;
  redi[tid] = e;
  __syncthreads();
  for (int s = VF_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] = __dadd_rn(red[tid], red[tid + s]);
      redi[tid] += redi[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    sse[blockIdx.x] = (long long)redi[0];
    ssim[blockIdx.x] = (mh >= 1 && mw >= 1) ? __ddiv_rn(red[0], (double)mh * (double)mw) : __longlong_as_double(0x7ff8000000000000LL);
  }
}

// tiles of one (n, c) plane; 0 when the arguments are outside the envelope
int64_t vm_tiles(int N, int C, int H, int W, int crop, int* tx, int* ty) {
  if (N < 1 || C < 1 || H < 1 || W < 1 || crop < 0) return 0;
  if (2 * (int64_t)crop >= (H < W ? H : W)) return 0;
  const int mh = H - 2 * crop - (VM_K - 1), mw = W - 2 * crop - (VM_K - 1);
  *ty = mh >= 1 ? (mh + VM_T - 1) / VM_T : 1;
  *tx = mw >= 1 ? (mw + VM_T - 1) / VM_T : 1;
  return (int64_t)*tx * *ty;
}

}  // namespace

extern "C" {

size_t sr_val_metrics_workspace(int N, int C, int H, int W, int crop) {
  int tx, ty;
  const int64_t t = vm_tiles(N, C, H, W, crop, &tx, &ty);
  return (size_t)t * (size_t)(N > 0 ? N : 0) * (size_t)(C > 0 ? C : 0) * (sizeof(double) + sizeof(unsigned long long));
}

int sr_val_metrics(const float* sr, const float* gt, int N, int C, int H, int W, int crop, int64_t* sse, double* ssim,
                   void* ws, size_t ws_bytes, void* stream) {
  if (!sr || !gt || !sse || !ssim || !ws) return sr_fail(SR_EINVAL, "val_metrics: null pointer");
  if (N < 1 || C < 1 || H < 1 || W < 1) return sr_fail(SR_EINVAL, "val_metrics: N, C, H, W must be >= 1");
  if (crop < 0) return sr_fail(SR_EINVAL, "val_metrics: crop must be >= 0");
  if (2 * (int64_t)crop >= (H < W ? H : W)) return sr_fail(SR_EINVAL, "val_metrics: the crop leaves no pixels");
  int tx, ty;
  const int64_t tiles = vm_tiles(N, C, H, W, crop, &tx, &ty);
  const int64_t blocks = tiles * N * C;
  if (tiles > 0x7fffffff || blocks > 0x7fffffff || (int64_t)N * C > 0x7fffffff)
    return sr_fail(SR_ETOOBIG, "val_metrics: too many tiles");
  if (ws_bytes < sr_val_metrics_workspace(N, C, H, W, crop)) return sr_fail(SR_EINVAL, "val_metrics: workspace too small");
  if ((uintptr_t)ws & 7) return sr_fail(SR_EINVAL, "val_metrics: workspace must be 8-byte aligned");
  VmArgs a;
  a.sr = sr, a.gt = gt;
  a.H = H, a.W = W, a.crop = crop, a.Hc = H - 2 * crop, a.Wc = W - 2 * crop;
  a.mh = a.Hc - (VM_K - 1), a.mw = a.Wc - (VM_K - 1);
  a.tiles_x = tx, a.tiles_y = ty;
  // the window of metrics/psnr_ssim.py:_ssim (cv2.getGaussianKernel(11, 1.5)), in float64 on the host
  double sum = 0.0;
  for (int i = 0; i < VM_K; ++i) {
    const double x = (double)i - 5.0;
    a.w[i] = std::exp(-x * x / (2.0 * 1.5 * 1.5));
    sum += a.w[i];
  }
  for (int i = 0; i < VM_K; ++i) a.w[i] /= sum;
  a.c1 = (0.01 * 255) * (0.01 * 255);
  a.c2 = (0.03 * 255) * (0.03 * 255);
  a.part_ssim = (double*)ws;
  a.part_sse = (unsigned long long*)(a.part_ssim + blocks);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(val_metrics_kernel, dim3((unsigned)blocks), dim3(VM_THREADS), 0, s, a);
  if (int rc = sr_check(hipGetLastError(), "val_metrics launch")) return rc;
  hipLaunchKernelGGL(val_metrics_finish_kernel, dim3((unsigned)(N * C)), dim3(VF_THREADS), 0, s, a.part_ssim, a.part_sse,
                     (int)tiles, a.mh, a.mw, (long long*)sse, ssim);
  return sr_check(hipGetLastError(), "val_metrics finish launch");
}

}  // extern "C"
