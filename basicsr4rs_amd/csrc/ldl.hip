// LDL artifact map ("Details or Artifacts", CVPR 2022; basicsr/losses/loss_util.py:99-145) and the ldl_opt
// term of RealESRGANModel (basicsr/models/realesrgan_model.py:211-226), forward and backward.
//
// Per image n and pixel p, with r = sum_c |gt - out|, e = sum_c |gt - ema|, the 7x7 window of the reflect-padded r
// (mean mu, unbiased variance L), the unbiased variance V_n of r over the image and P_n = V_n^(1/5):
//   w[p] = P_n * L[p] * m[p],  m = (r >= e).
//
//   ldl_map_fwd_kernel : a block owns a LT_W x LT_H tile of one image.  r of the tile and a halo of 3 goes to
//       LDS by reflect indexing; a horizontal and a vertical 7-tap pass (separable box sums of r and r^2) give
//       mu and L; the block writes the fp32 planes r, mu, m L and m and leaves one (count, mean, M2, sum m L r)
//       partial: the mean first, then the squared deviations from it, each summed in a fixed order (a shuffle
//       tree per wave, then the four waves).
//   ldl_finalize_kernel : one wave merges the partials of an image with Chan's rule in double (a lane takes
//       every 64th tile, then a shuffle tree) and writes its statistics (mean, V, P, S = sum m L r,
//       Q = dP/dV * 2 / (M - 1), T); the first block also writes the fused L1 loss k * sum_n P_n S_n; with a
//       map wanted, every block scales its rows: w = P_n * (m L).
//   ldl_t_partial_kernel : T_n = sum_p dW m L of the general backward, per image and block.
//   ldl_map_bwd_kernel : a gather, one thread per pixel of the same tiles.  a = m dW (dW = k r for the fused
//       L1 term) and a mu of the tile and a halo of 3 go to LDS, zero outside the image.  A window centred at c
//       reaches the pixel p through every padded position that reflects to p, so the fold of the reflect pad
//       is a multiplicity (1 to 3 per axis) on the taps of the 7x7 window around p:
//         G[p] = 2/48 * (r[p] * sum_c M(p,c) a[c] - sum_c M(p,c) a[c] mu[c]),  M = My(y,cy) * Mx(x,cx),
//       again one horizontal and one vertical pass.  Then g_r = P_n G + T_n Q_n (r - mean_n) and
//       d out[c] = sign(out - gt) * (g_r + k w) * upstream, rounded once to out's dtype, each element written once.
//
// A wave owns one tile row: 64 consecutive pixels per load and store instruction (256 B of fp32, 128 B of
// bf16).  The rows of an odd-width image are not 16-byte aligned and the halo is reflected, so the accesses
// are scalar per lane.  No atomics; every sum has a fixed order, two runs give the same bits; nothing
// allocates or synchronises.
#include <math.h>
#include <stdio.h>
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int LT_W = 64, LT_H = 16, LT_PAD = 3, LT_K = 7;
constexpr int LT_HW = LT_W + 2 * LT_PAD, LT_HH = LT_H + 2 * LT_PAD;  // the halo tile: 70 x 22
constexpr int LT_THREADS = 256, LT_WAVES = LT_THREADS / 64;
constexpr int LT_ROWS = LT_THREADS / LT_W;        // tile rows one pass of the block covers
constexpr int LT_PER_THREAD = LT_H / LT_ROWS;     // pixels per thread
constexpr int LT_TB_MAX = 64;                     // blocks per image of the T_n reduce
constexpr int LT_STATS = 8;                       // floats per image: mean, V, P, S, Q, T, 0, 0
enum { ST_MEAN = 0, ST_V = 1, ST_P = 2, ST_S = 3, ST_Q = 4, ST_T = 5 };

struct LdlGeom {
  int N, C, H, W, tx, ty;  // tiles per row and column
};

SR_DEV int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// taps of the window around x that reach x: itself, its mirror at the low edge, its mirror at the high edge
SR_DEV float fold_mult(int x, int cx, int n) {
  return 1.f + ((x >= 1 && cx <= 3 - x) ? 1.f : 0.f) + ((x <= n - 2 && cx >= 2 * n - 5 - x) ? 1.f : 0.f);
}

// sum over the block in a fixed order (a shuffle tree per wave, then the waves in order); every thread gets
// the result.  red: LT_WAVES floats of LDS.
SR_DEV float block_sum(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < LT_WAVES; ++w) s += red[w];
  return s;
}

template <typename OT, typename GT, typename ET>
__global__ void __launch_bounds__(LT_THREADS)
    ldl_map_fwd_kernel(const OT* __restrict__ out, const GT* __restrict__ gt, const ET* __restrict__ ema, LdlGeom g,
                       float* __restrict__ planes, float* __restrict__ partial) {
  __shared__ float s_r[LT_HH][LT_HW + 1];
  __shared__ float s_h1[LT_HH][LT_W], s_h2[LT_HH][LT_W];
  __shared__ float s_red[LT_WAVES];
  const int tiles = g.tx * g.ty, n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int y0 = (t / g.tx) * LT_H, x0 = (t % g.tx) * LT_W;
  const int64_t HW = (int64_t)g.H * g.W, img = (int64_t)n * g.C * HW;

  // r of the tile and its halo; positions past the padded image (a remainder tile) are never read back
  for (int i = threadIdx.x; i < LT_HH * LT_HW; i += LT_THREADS) {
    const int hy = i / LT_HW, hx = i - hy * LT_HW;
    const int py = y0 + hy - LT_PAD, px = x0 + hx - LT_PAD;
    float r = 0.f;
    if (py < g.H + LT_PAD && px < g.W + LT_PAD) {
      const int64_t p = img + (int64_t)reflect(py, g.H) * g.W + reflect(px, g.W);
      for (int c = 0; c < g.C; ++c) r += fabsf(Elt<GT>::to_f(gt[p + c * HW]) - Elt<OT>::to_f(out[p + c * HW]));
    }
    s_r[hy][hx] = r;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LT_HH * LT_W; i += LT_THREADS) {
    const int hy = i / LT_W, x = i - hy * LT_W;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < LT_K; ++k) {
      const float v = s_r[hy][x + k];
      a += v;
      b = fmaf(v, v, b);
    }
    s_h1[hy][x] = a;
    s_h2[hy][x] = b;
  }
  __syncthreads();

  const int lx = threadIdx.x % LT_W, ly0 = threadIdx.x / LT_W, x = x0 + lx;
  float rv[LT_PER_THREAD], lm[LT_PER_THREAD];
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < LT_PER_THREAD; ++j) {
    const int ly = ly0 + j * LT_ROWS, y = y0 + ly;
    rv[j] = lm[j] = 0.f;
    if (y >= g.H || x >= g.W) continue;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int k = 0; k < LT_K; ++k) {
      a += s_h1[ly + k][lx];
      b += s_h2[ly + k][lx];
    }
    const float mu = a * (1.f / 49.f);
    const float L = fmaxf(fmaf(-a, mu, b), 0.f) * (1.f / 48.f);
    const float r = s_r[ly + LT_PAD][lx + LT_PAD];
    const int64_t p = img + (int64_t)y * g.W + x;
    float e = 0.f;
    for (int c = 0; c < g.C; ++c) e += fabsf(Elt<GT>::to_f(gt[p + c * HW]) - Elt<ET>::to_f(ema[p + c * HW]));
    const float m = r < e ? 0.f : 1.f;
    const int64_t q = (int64_t)n * HW + (int64_t)y * g.W + x, NHW = (int64_t)g.N * HW;
    planes[q] = r;
    planes[NHW + q] = mu;
    planes[2 * NHW + q] = m * L;
    planes[3 * NHW + q] = m;
    rv[j] = r, lm[j] = m * L;
    sum += r;
  }
  // the block's (count, mean, M2, S): the mean first, then the deviations from it
  const float bc = (float)(min(LT_H, g.H - y0) * min(LT_W, g.W - x0));  // the tile's pixels inside the image: >= 1
  const float bmean = block_sum(sum, s_red) / bc;
  float m2 = 0.f, s = 0.f;
#pragma unroll
  for (int j = 0; j < LT_PER_THREAD; ++j) {
    const int y = y0 + ly0 + j * LT_ROWS;
    if (y >= g.H || x >= g.W) continue;
    const float d = rv[j] - bmean;
    m2 = fmaf(d, d, m2);
    s = fmaf(lm[j], rv[j], s);
  }
  const float bm2 = block_sum(m2, s_red), bs = block_sum(s, s_red);
  if (threadIdx.x == 0) {
    float* o = partial + (int64_t)blockIdx.x * 4;
    o[0] = bc, o[1] = bmean, o[2] = bm2, o[3] = bs;
  }
}

// Chan's merge of (cb, mb, Mb, Sb) into (ca, ma, Ma, Sa); an empty side changes nothing
SR_DEV void chan_merge(double& ca, double& ma, double& Ma, double& Sa, double cb, double mb, double Mb, double Sb) {
  if (cb == 0.0) return;
  const double tot = ca + cb, d = mb - ma;
  ma += d * (cb / tot);
  Ma += Mb + d * d * (ca * cb / tot);
  Sa += Sb;
  ca = tot;
}

// The partials of image n merged by one wave in a fixed order (lane l takes tiles l, l + 64, ..., then a shuffle
// tree); every lane returns the same bits.
SR_DEV void fold_image(const float* __restrict__ partial, int n, int tiles, double& mean, double& M2, double& S) {
  const int lane = threadIdx.x & 63;
  double c = 0.0, m = 0.0, M = 0.0, s = 0.0;
  for (int t = lane; t < tiles; t += 64) {
    const float* p = partial + ((int64_t)n * tiles + t) * 4;
    chan_merge(c, m, M, s, (double)p[0], (double)p[1], (double)p[2], (double)p[3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    chan_merge(c, m, M, s, __shfl_down(c, o), __shfl_down(m, o), __shfl_down(M, o), __shfl_down(s, o));
  mean = __shfl(m, 0), M2 = __shfl(M, 0), S = __shfl(s, 0);
}

SR_DEV double ldl_pow5(double V) { return V > 0.0 ? pow(V, 0.2) : 0.0; }

// grid (row chunks, N).  Wave 0 of every block folds its image; the first block also folds every image, wave w
// the images w, w + 4, ..., for the loss.
__global__ void __launch_bounds__(LT_THREADS)
    ldl_finalize_kernel(const float* __restrict__ partial, LdlGeom g, int l1, double k, const float* __restrict__ planes,
                        float* __restrict__ stats, float* __restrict__ loss, float* __restrict__ w) {
  __shared__ double s_acc[LT_WAVES];
  __shared__ float s_P;
  const int tiles = g.tx * g.ty, n = blockIdx.y, wave = threadIdx.x >> 6;
  const int64_t HW = (int64_t)g.H * g.W;
  const bool first = blockIdx.x == 0 && n == 0;
  if (wave == 0) {
    double mean, M2, S;
    fold_image(partial, n, tiles, mean, M2, S);
    const double V = M2 / (double)(HW - 1);
    const double P = ldl_pow5(V);
    if (threadIdx.x == 0) {
      s_P = (float)P;
      if (blockIdx.x == 0) {
        float* st = stats + (int64_t)n * LT_STATS;
        st[ST_MEAN] = (float)mean, st[ST_V] = (float)V, st[ST_P] = (float)P, st[ST_S] = (float)S;
        // V == 0 (a constant residual map): the dP/dV term is defined as 0
        st[ST_Q] = V > 0.0 ? (float)(0.2 * pow(V, -0.8) * 2.0 / (double)(HW - 1)) : 0.f;
        st[ST_T] = l1 ? (float)(k * S) : 0.f;
        st[6] = st[7] = 0.f;
      }
    }
  }
  if (l1 && first) {
    double acc = 0.0;
    for (int i = wave; i < g.N; i += LT_WAVES) {
      double mi, M2i, Si;
      fold_image(partial, i, tiles, mi, M2i, Si);
      acc += ldl_pow5(M2i / (double)(HW - 1)) * Si;
    }
    if ((threadIdx.x & 63) == 0) s_acc[wave] = acc;
  }
  __syncthreads();
  if (l1 && first && threadIdx.x == 0) {
    double acc = s_acc[0];
    for (int i = 1; i < LT_WAVES; ++i) acc += s_acc[i];
    *loss = (float)(k * acc);
  }
  if (w) {
    const float Pf = s_P;
    const float* lm = planes + 2 * (int64_t)g.N * HW + (int64_t)n * HW;
    float* wn = w + (int64_t)n * HW;
    for (int64_t i = (int64_t)blockIdx.x * LT_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * LT_THREADS)
      wn[i] = Pf * lm[i];
  }
}

// grid (nb, N): tpart[n * nb + b] = the block's share of sum_p dW * (m L), a fixed-order tree
__global__ void __launch_bounds__(LT_THREADS)
    ldl_t_partial_kernel(const float* __restrict__ dW, const float* __restrict__ planes, LdlGeom g, float* __restrict__ tpart) {
  __shared__ float s_red[LT_WAVES];
  const int n = blockIdx.y;
  const int64_t HW = (int64_t)g.H * g.W;
  const float* lm = planes + 2 * (int64_t)g.N * HW + (int64_t)n * HW;
  const float* d = dW + (int64_t)n * HW;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LT_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * LT_THREADS)
    s = fmaf(d[i], lm[i], s);
  const float b = block_sum(s, s_red);
  if (threadIdx.x == 0) tpart[(int64_t)n * gridDim.x + blockIdx.x] = b;
}

// dW == null: the fused L1 term (a = k m r, direct = k w, T_n from the statistics); otherwise a = m dW,
// T_n = the fold of tpart[n * nb ...].  up: the upstream scalar on the device (null = 1).
template <typename OT, typename GT>
__global__ void __launch_bounds__(LT_THREADS)
    ldl_map_bwd_kernel(const OT* __restrict__ out, const GT* __restrict__ gt, const float* __restrict__ planes,
                       const float* __restrict__ stats, const float* __restrict__ dW, const float* __restrict__ tpart,
                       int nb, float k, const float* __restrict__ up, LdlGeom g, OT* __restrict__ dout) {
  __shared__ float s_a[LT_HH][LT_HW + 1], s_b[LT_HH][LT_HW + 1];
  __shared__ float s_ha[LT_HH][LT_W], s_hb[LT_HH][LT_W];
  const int tiles = g.tx * g.ty, n = blockIdx.x / tiles, t = blockIdx.x - n * tiles;
  const int y0 = (t / g.tx) * LT_H, x0 = (t % g.tx) * LT_W;
  const int64_t HW = (int64_t)g.H * g.W, NHW = (int64_t)g.N * HW, pl = (int64_t)n * HW;
  const float* p_r = planes + pl;
  const float* p_mu = planes + NHW + pl;
  const float* p_lm = planes + 2 * NHW + pl;
  const float* p_m = planes + 3 * NHW + pl;

  for (int i = threadIdx.x; i < LT_HH * LT_HW; i += LT_THREADS) {
    const int hy = i / LT_HW, hx = i - hy * LT_HW;
    const int py = y0 + hy - LT_PAD, px = x0 + hx - LT_PAD;
    float a = 0.f, b = 0.f;
    if (py >= 0 && py < g.H && px >= 0 && px < g.W) {
      const int64_t q = (int64_t)py * g.W + px;
      a = p_m[q] * (dW ? dW[pl + q] : k * p_r[q]);
      b = a * p_mu[q];
    }
    s_a[hy][hx] = a;
    s_b[hy][hx] = b;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LT_HH * LT_W; i += LT_THREADS) {
    const int hy = i / LT_W, lx = i - hy * LT_W, x = x0 + lx;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < LT_K; ++j) {
      const float m = fold_mult(x, x + j - LT_PAD, g.W);
      a = fmaf(m, s_a[hy][lx + j], a);
      b = fmaf(m, s_b[hy][lx + j], b);
    }
    s_ha[hy][lx] = a;
    s_hb[hy][lx] = b;
  }
  __syncthreads();

  const float* st = stats + (int64_t)n * LT_STATS;
  const float mean = st[ST_MEAN], P = st[ST_P], Q = st[ST_Q];
  float T = st[ST_T];
  if (dW) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc += (double)tpart[(int64_t)n * nb + b];
    T = (float)acc;
  }
  const float us = up ? *up : 1.f;
  const float direct = dW ? 0.f : k * P;
  const int lx = threadIdx.x % LT_W, ly0 = threadIdx.x / LT_W, x = x0 + lx;
  const int64_t img = (int64_t)n * g.C * HW;
#pragma unroll
  for (int j = 0; j < LT_PER_THREAD; ++j) {
    const int ly = ly0 + j * LT_ROWS, y = y0 + ly;
    if (y >= g.H || x >= g.W) continue;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < LT_K; ++i) {
      const float m = fold_mult(y, y + i - LT_PAD, g.H);
      a = fmaf(m, s_ha[ly + i][lx], a);
      b = fmaf(m, s_hb[ly + i][lx], b);
    }
    const int64_t q = (int64_t)y * g.W + x;
    const float r = p_r[q];
    const float G = (2.f / 48.f) * fmaf(r, a, -b);
    const float gr = (fmaf(P, G, T * Q * (r - mean)) + direct * p_lm[q]) * us;
    const int64_t p = img + q;
    for (int c = 0; c < g.C; ++c) {
      const float d = Elt<OT>::to_f(out[p + c * HW]) - Elt<GT>::to_f(gt[p + c * HW]);
      dout[p + c * HW] = Elt<OT>::from_f(d > 0.f ? gr : (d < 0.f ? -gr : 0.f));
    }
  }
}

template <typename OT, typename GT>
void launch_fwd_e(int edt, unsigned grid, hipStream_t s, const void* out, const void* gt, const void* ema, LdlGeom g,
                  float* planes, float* partial) {
  if (edt == SR_F32)
    hipLaunchKernelGGL((ldl_map_fwd_kernel<OT, GT, float>), dim3(grid), dim3(LT_THREADS), 0, s, (const OT*)out, (const GT*)gt,
                       (const float*)ema, g, planes, partial);
  else
    hipLaunchKernelGGL((ldl_map_fwd_kernel<OT, GT, bf16_t>), dim3(grid), dim3(LT_THREADS), 0, s, (const OT*)out,
                       (const GT*)gt, (const bf16_t*)ema, g, planes, partial);
}

// shared refusals of the two entry points; fills the geometry
int ldl_check(const char* who, int out_dtype, int gt_dtype, int N, int C, int H, int W, int ksize, LdlGeom& g) {
  static thread_local char msg[160];
  const char* why = nullptr;
  if (ksize != 7) why = "the kernel covers ksize 7 only";
  else if (N < 1 || C < 1 || N > 65535) why = "N must be 1 to 65535 and C positive";
  else if (H < 4 || W < 4) why = "H and W must be at least 4 (a reflect pad of 3)";
  else if ((int64_t)N * C * H * W >= (1ll << 31)) why = "N*C*H*W must be below 2^31";
  else if ((out_dtype != SR_F32 && out_dtype != SR_BF16) || (gt_dtype != SR_F32 && gt_dtype != out_dtype))
    why = "out must be fp32 or bf16, gt and ema fp32 or out's dtype";
  if (why) {
    snprintf(msg, sizeof(msg), "%s: %s", who, why);
    return sr_fail(SR_EINVAL, msg);
  }
  g.N = N, g.C = C, g.H = H, g.W = W;
  g.tx = (W + LT_W - 1) / LT_W, g.ty = (H + LT_H - 1) / LT_H;
  return SR_OK;
}

int64_t ldl_tiles(int H, int W) { return (int64_t)((W + LT_W - 1) / LT_W) * ((H + LT_H - 1) / LT_H); }

// blocks per image of a row-major pass over H*W fp32 values
int ldl_row_blocks(int64_t HW) {
  const int64_t need = (HW + LT_THREADS * 4 - 1) / (LT_THREADS * 4);
  return (int)(need < 1 ? 1 : (need > LT_TB_MAX ? LT_TB_MAX : need));
}

}  // namespace

extern "C" {

size_t sr_ldl_map_workspace(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  return (size_t)N * (size_t)ldl_tiles(H, W) * 4 * sizeof(float) + (size_t)N * LT_TB_MAX * sizeof(float);
}

int sr_ldl_map_fwd(int out_dtype, int gt_dtype, int ema_dtype, const void* out, const void* gt, const void* ema, int N,
                   int C, int H, int W, int ksize, int l1, int reduction, float loss_weight, float* w, float* planes,
                   float* stats, float* loss, void* workspace, size_t ws_bytes, void* stream) {
  LdlGeom g;
  const int rc = ldl_check("ldl_map_fwd", out_dtype, gt_dtype, N, C, H, W, ksize, g);
  if (rc != SR_OK) return rc;
  if (ema_dtype != SR_F32 && ema_dtype != out_dtype)
    return sr_fail(SR_EINVAL, "ldl_map_fwd: out must be fp32 or bf16, gt and ema fp32 or out's dtype");
  if (!out || !gt || !ema || !planes || !stats || !workspace) return sr_fail(SR_EINVAL, "ldl_map_fwd: null pointer");
  if (l1 ? (!loss || (reduction != SR_REDUCE_MEAN && reduction != SR_REDUCE_SUM)) : !w)
    return sr_fail(SR_EINVAL, "ldl_map_fwd: the L1 term needs loss and reduction 'mean' / 'sum', the bare map needs w");
  if (ws_bytes < sr_ldl_map_workspace(N, H, W)) return sr_fail(SR_EINVAL, "ldl_map_fwd: workspace too small");
  const int osz = out_dtype == SR_BF16 ? 2 : 4, gsz = gt_dtype == SR_BF16 ? 2 : 4, esz = ema_dtype == SR_BF16 ? 2 : 4;
  if (((uintptr_t)out & (osz - 1)) || ((uintptr_t)gt & (gsz - 1)) || ((uintptr_t)ema & (esz - 1)) ||
      (((uintptr_t)w | (uintptr_t)planes | (uintptr_t)stats | (uintptr_t)loss | (uintptr_t)workspace) & 3))
    return sr_fail(SR_EINVAL, "ldl_map_fwd: tensors must be element-aligned");

  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
  const unsigned grid = (unsigned)((int64_t)N * g.tx * g.ty);
  if (out_dtype == SR_F32) launch_fwd_e<float, float>(ema_dtype, grid, s, out, gt, ema, g, planes, partial);
  else if (gt_dtype == SR_F32) launch_fwd_e<bf16_t, float>(ema_dtype, grid, s, out, gt, ema, g, planes, partial);
  else launch_fwd_e<bf16_t, bf16_t>(ema_dtype, grid, s, out, gt, ema, g, planes, partial);
  const int64_t HW = (int64_t)H * W;
  const double k = reduction == SR_REDUCE_MEAN ? (double)loss_weight / ((double)N * C * (double)HW) : (double)loss_weight;
  hipLaunchKernelGGL(ldl_finalize_kernel, dim3(w ? ldl_row_blocks(HW) : 1, N), dim3(LT_THREADS), 0, s, (const float*)partial,
                     g, l1, k, (const float*)planes, stats, loss, w);
  return sr_check(hipGetLastError(), "ldl_map_fwd launch");
}

int sr_ldl_map_bwd(int out_dtype, int gt_dtype, const void* out, const void* gt, const float* planes, const float* stats,
                   const float* dW, const float* upstream, int N, int C, int H, int W, int ksize, int reduction,
                   float loss_weight, void* dout, void* workspace, size_t ws_bytes, void* stream) {
  LdlGeom g;
  const int rc = ldl_check("ldl_map_bwd", out_dtype, gt_dtype, N, C, H, W, ksize, g);
  if (rc != SR_OK) return rc;
  if (!out || !gt || !planes || !stats || !dout || (dW && !workspace)) return sr_fail(SR_EINVAL, "ldl_map_bwd: null pointer");
  if (!dW && reduction != SR_REDUCE_MEAN && reduction != SR_REDUCE_SUM)
    return sr_fail(SR_EINVAL, "ldl_map_bwd: the L1 term (no dW) needs reduction 'mean' / 'sum'");
  if (dW && ws_bytes < sr_ldl_map_workspace(N, H, W)) return sr_fail(SR_EINVAL, "ldl_map_bwd: workspace too small");
  const int osz = out_dtype == SR_BF16 ? 2 : 4, gsz = gt_dtype == SR_BF16 ? 2 : 4;
  if ((((uintptr_t)out | (uintptr_t)dout) & (osz - 1)) || ((uintptr_t)gt & (gsz - 1)) ||
      (((uintptr_t)planes | (uintptr_t)stats | (uintptr_t)dW | (uintptr_t)upstream | (uintptr_t)workspace) & 3))
    return sr_fail(SR_EINVAL, "ldl_map_bwd: tensors must be element-aligned");

  hipStream_t s = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  float* tpart = (float*)workspace;
  const int nb = ldl_row_blocks(HW);
  if (dW) hipLaunchKernelGGL(ldl_t_partial_kernel, dim3(nb, N), dim3(LT_THREADS), 0, s, dW, planes, g, tpart);
  const float k = reduction == SR_REDUCE_MEAN ? (float)((double)loss_weight / ((double)N * C * (double)HW)) : loss_weight;
  const unsigned grid = (unsigned)((int64_t)N * g.tx * g.ty);
  if (out_dtype == SR_F32)
    hipLaunchKernelGGL((ldl_map_bwd_kernel<float, float>), dim3(grid), dim3(LT_THREADS), 0, s, (const float*)out,
                       (const float*)gt, planes, stats, dW, (const float*)tpart, nb, k, upstream, g, (float*)dout);
  else if (gt_dtype == SR_F32)
    hipLaunchKernelGGL((ldl_map_bwd_kernel<bf16_t, float>), dim3(grid), dim3(LT_THREADS), 0, s, (const bf16_t*)out,
                       (const float*)gt, planes, stats, dW, (const float*)tpart, nb, k, upstream, g, (bf16_t*)dout);
  else
    hipLaunchKernelGGL((ldl_map_bwd_kernel<bf16_t, bf16_t>), dim3(grid), dim3(LT_THREADS), 0, s, (const bf16_t*)out,
                       (const bf16_t*)gt, planes, stats, dW, (const float*)tpart, nb, k, upstream, g, (bf16_t*)dout);
  return sr_check(hipGetLastError(), "ldl_map_bwd launch");
}

}  // extern "C"
