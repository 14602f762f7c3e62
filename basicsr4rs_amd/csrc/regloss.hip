// RegisteredLoss (basicsr/losses/align_loss.py:161-256): the minimum over a grid of sub-pixel shifts of the L1 / MSE
// between the shifted prediction and the target, forward and backward, without ever storing a shifted image
// (DESIGN.md §6l).
//
// The shifts are separable: a table T[S][K] of 1-D taps (K = 2r + 1, built on the host; the kernels know nothing of
// Lanczos) serves both axes, shift s = sy * S + sx:
//   shifted[b, s, c, h, w] = sum_j sum_i T[sy, j] T[sx, i] pred[b, c, h + j - r, w + i - r]   (zero outside the image)
//   loss[b, s] = mean over c and the crop [r, H - r) x [r, W - r) of phi(shifted - target),  phi = |d| or d^2.
// No pixel of the crop has a tap outside the image, so the forward never meets the zero padding; the backward does.
//
//   reg_fwd_kernel : a block owns a RT_W x RT_H tile of the crop of one (b, c) plane.  The tile of pred and a halo
//       of r go to LDS; one pass forms the S y-shifted row sets [S][RT_H][RT_W + 2r] in LDS (a thread reads a column
//       of K values once and serves every sy from registers); then a thread owns 4 pixels, reads the K values of a
//       y-shifted row once per sy and runs the S x-filters over them into S^2 accumulators of phi(d), all in
//       registers (the loops over sy, sx and the taps are unrolled, the tap table is read with uniform addresses).
//       The block leaves S^2 partial sums (a tree of DPP rotations and row swaps per wave, then the four waves in
//       order).
//   reg_finalize_kernel : one block per image sums its partials in double (1024 / S^2 strided groups, then the groups
//       in order), divides by n = C (H - 2r)(W - 2r), writes the optional [B, S^2] table, the first minimum (a NaN
//       wins, as torch.argmin) and the image's loss.
//   reg_reduce_kernel : 'mean' / 'sum' over the images, one wave, in double, a fixed order.
//   reg_bwd_kernel : a block owns a RT_W x RT_H tile of d pred of one plane and reads idx[b] from device memory.  pred
//       with a halo of 2r goes to LDS (zero outside the image); the y pass and the x pass of the selected shift alone
//       give d, hence g = k phi'(d) / n, on the tile plus a halo of r (zero outside the crop); the transposed
//       filter is a gather, x then y:  d pred[p, q] = sum_j sum_i T[sy, j] T[sx, i] g[p - j + r, q - i + r].
//       Every element of d pred is written once, rounded once to pred's dtype.
//
// A wave owns tile rows: 64 consecutive pixels per load and store.  No atomics; every sum has a fixed order, two
// runs give the same bits; nothing allocates or synchronises.
#include <math.h>
#include <stdio.h>
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int RT_W = 64, RT_H = 16, RT_THREADS = 256, RT_WAVES = RT_THREADS / 64;
constexpr int RT_ROWS = RT_THREADS / RT_W;      // tile rows one pass of the block covers
constexpr int RT_PER_THREAD = RT_H / RT_ROWS;   // pixels per thread
constexpr int RF_THREADS = 1024;              // the per-image finalise: floor(1024 / S^2) strided groups
constexpr int RL_SMAX = 9, RL_S2MAX = RL_SMAX * RL_SMAX, RL_RMAX = 6, RL_KMAX = 2 * RL_RMAX + 1, RL_KMIN = 7;
// the backward's LDS tiles at r = RL_RMAX (smaller r uses the same row strides)
constexpr int RB_PW = RT_W + 4 * RL_RMAX, RB_PH = RT_H + 4 * RL_RMAX;  // pred with a halo of 2r: 88 x 40
constexpr int RB_GW = RT_W + 2 * RL_RMAX, RB_GH = RT_H + 2 * RL_RMAX;  // g with a halo of r: 76 x 28

struct RegGeom {
  int B, C, H, W, S, K;
  int tx, ty;  // forward: tiles per row / column of the crop
  int bx, by;  // backward: tiles per row / column of the image
};

// v + the value of the lane CTRL selects (a DPP row rotation: the compiler folds it into the add)
template <int CTRL>
SR_DEV float dpp_add(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// sum over the wave in a fixed order, every lane gets the same bits: rotations by 8, 4, 2, 1 inside the rows of 16
// lanes (each step adds the partner lane ^ 8, ^ 4, ...), then the rows (sr_common.h).  All VALU, no LDS round trip.
SR_DEV float wave_sum(float v) {
  v = dpp_add<0x128>(v);  // row_ror:8
  v = dpp_add<0x124>(v);  // row_ror:4
  v = dpp_add<0x122>(v);  // row_ror:2
  v = dpp_add<0x121>(v);  // row_ror:1
  return xsum32(xsum16(v));
}

template <typename PT, typename TT, int K, bool L1>
__global__ void __launch_bounds__(RT_THREADS)
    reg_fwd_kernel(const PT* __restrict__ pred, const TT* __restrict__ target, const float* __restrict__ taps, RegGeom g,
                   float* __restrict__ partial) {
  constexpr int R = K / 2, PW = RT_W + 2 * R, PH = RT_H + 2 * R;
  extern __shared__ float smem[];
  float* s_p = smem;            // [PH][PW]: pred, tile + halo; the wave sums at the end
  float* s_y = smem + PH * PW;  // [S][RT_H][PW]: the y-shifted rows
  const int S = g.S, tiles = g.tx * g.ty, plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  // crop coordinates of the tile's first pixel = image coordinates of the halo's first pixel
  const int y0 = (t / g.tx) * RT_H, x0 = (t % g.tx) * RT_W;
  const int64_t base = (int64_t)plane * g.H * g.W;

  for (int i = threadIdx.x; i < PH * PW; i += RT_THREADS) {
    const int a = i / PW, y = y0 + a, x = x0 + (i - a * PW);
    s_p[i] = (y < g.H && x < g.W) ? Elt<PT>::to_f(pred[base + (int64_t)y * g.W + x]) : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RT_H * PW; i += RT_THREADS) {
    const int ly = i / PW, cc = i - ly * PW;
    float col[K];
#pragma unroll
    for (int j = 0; j < K; ++j) col[j] = s_p[(ly + j) * PW + cc];
#pragma unroll
    for (int sy = 0; sy < RL_SMAX; ++sy) {
      if (sy < S) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j) a = fmaf(taps[sy * K + j], col[j], a);
        s_y[(sy * RT_H + ly) * PW + cc] = a;
      }
    }
  }
  __syncthreads();

  float acc[RL_S2MAX];
#pragma unroll
  for (int s = 0; s < RL_S2MAX; ++s) acc[s] = 0.f;
  const int lx = threadIdx.x % RT_W, ly0 = threadIdx.x / RT_W;
  const int Hc = g.H - 2 * R, Wc = g.W - 2 * R;
#pragma unroll 1
  for (int jj = 0; jj < RT_PER_THREAD; ++jj) {
    const int ly = ly0 + jj * RT_ROWS, cy = y0 + ly, cx = x0 + lx;
    // a pixel past the crop (a remainder tile) adds nothing: its lane sits the body out
    if (cy >= Hc || cx >= Wc) continue;
    const float tv = Elt<TT>::to_f(target[base + (int64_t)(cy + R) * g.W + cx + R]);
#pragma unroll
    for (int sy = 0; sy < RL_SMAX; ++sy) {
      if (sy < S) {
        float row[K];
#pragma unroll
        for (int i = 0; i < K; ++i) row[i] = s_y[(sy * RT_H + ly) * PW + lx + i];
#pragma unroll
        for (int sx = 0; sx < RL_SMAX; ++sx) {
          if (sx < S) {
            float v = 0.f;
#pragma unroll
            for (int i = 0; i < K; ++i) v = fmaf(taps[sx * K + i], row[i], v);
            const float d = v - tv;
            acc[sy * RL_SMAX + sx] += L1 ? fabsf(d) : d * d;
          }
        }
      }
    }
  }

  // the block's S^2 sums: a tree per wave, then the waves in order
  __syncthreads();
  float* s_red = smem;  // [RT_WAVES][RL_S2MAX] <= PH * PW
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < RL_S2MAX; ++s) {
    if (s / RL_SMAX < S && s % RL_SMAX < S) {
      const float v = wave_sum(acc[s]);
      if (lane == 0) s_red[wave * RL_S2MAX + s] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < RL_S2MAX) {
    const int sy = threadIdx.x / RL_SMAX, sx = threadIdx.x % RL_SMAX;
    if (sy < S && sx < S) {
      float v = s_red[threadIdx.x];
#pragma unroll
      for (int w = 1; w < RT_WAVES; ++w) v += s_red[w * RL_S2MAX + threadIdx.x];
      partial[(int64_t)blockIdx.x * (S * S) + sy * S + sx] = v;
    }
  }
}

// grid B, RF_THREADS threads.  partial: [B][nblk][S2].  minloss: the selected mean of every image, in double.
__global__ void __launch_bounds__(RF_THREADS)
    reg_finalize_kernel(const float* __restrict__ partial, int nblk, int S2, double n, float loss_weight, int none,
                        int* __restrict__ idx, float* __restrict__ table, double* __restrict__ minloss,
                        float* __restrict__ out) {
  __shared__ double s_part[RF_THREADS];
  __shared__ double s_mean[RL_S2MAX];
  const int b = blockIdx.x, G = RF_THREADS / S2, gi = threadIdx.x / S2, s = threadIdx.x - gi * S2;
  double a = 0.0;
  if (gi < G) {
    const float* p = partial + (int64_t)b * nblk * S2 + s;
#pragma unroll 4
    for (int k = gi; k < nblk; k += G) a += (double)p[(int64_t)k * S2];
  }
  s_part[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x < S2) {
    double t = s_part[threadIdx.x];
    for (int q = 1; q < G; ++q) t += s_part[q * S2 + threadIdx.x];
    t /= n;
    s_mean[threadIdx.x] = t;
    if (table) table[(int64_t)b * S2 + threadIdx.x] = (float)t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // the first minimum of the fp32 values; the first NaN wins over every number (torch.argmin)
    int best = 0;
    float bv = (float)s_mean[0];
    for (int q = 1; q < S2 && bv == bv; ++q) {
      const float v = (float)s_mean[q];
      if (v < bv || v != v) best = q, bv = v;
    }
    idx[b] = best;
    minloss[b] = s_mean[best];
    if (none) out[b] = (float)((double)loss_weight * s_mean[best]);
  }
}

// one wave: out = k * sum_b minloss[b]; lane l takes the images l, l + 64, ..., then a shuffle tree
__global__ void __launch_bounds__(64) reg_reduce_kernel(const double* __restrict__ minloss, int B, double k, float* __restrict__ out) {
  double a = 0.0;
  for (int b = threadIdx.x; b < B; b += 64) a += minloss[b];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
  if (threadIdx.x == 0) *out = (float)(k * a);
}

// kf = k_b / n.  d pred = the transposed filter of g = kf phi'(d) on the crop, 0 elsewhere.
template <typename PT, typename TT>
__global__ void __launch_bounds__(RT_THREADS)
    reg_bwd_kernel(const PT* __restrict__ pred, const TT* __restrict__ target, const float* __restrict__ taps,
                   const int* __restrict__ idx, RegGeom g, int l1, float kf, PT* __restrict__ dpred) {
  __shared__ float s_p[RB_PH * RB_PW];  // pred, tile + 2r; then the x-filtered g [gh][RT_W]
  __shared__ float s_y[RB_GH * RB_PW];  // y-shifted rows of the tile + r
  __shared__ float s_g[RB_GH * RB_GW];
  __shared__ float s_t[2 * RL_KMAX];    // T[sy], T[sx]
  const int K = g.K, r = K / 2, S = g.S;
  const int tiles = g.bx * g.by, plane = blockIdx.x / tiles, t = blockIdx.x - plane * tiles;
  const int y0 = (t / g.bx) * RT_H, x0 = (t % g.bx) * RT_W;
  const int64_t base = (int64_t)plane * g.H * g.W;
  const int sel = min(max(idx[plane / g.C], 0), S * S - 1);
  const int sy = sel / S, sx = sel - sy * S;
  if (threadIdx.x < K) {
    s_t[threadIdx.x] = taps[sy * K + threadIdx.x];
    s_t[RL_KMAX + threadIdx.x] = taps[sx * K + threadIdx.x];
  }
  const int pw = RT_W + 4 * r, ph = RT_H + 4 * r, gw = RT_W + 2 * r, gh = RT_H + 2 * r;
  for (int i = threadIdx.x; i < ph * pw; i += RT_THREADS) {
    const int a = i / pw, c = i - a * pw, y = y0 - 2 * r + a, x = x0 - 2 * r + c;
    s_p[a * RB_PW + c] =
        (y >= 0 && y < g.H && x >= 0 && x < g.W) ? Elt<PT>::to_f(pred[base + (int64_t)y * g.W + x]) : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < gh * pw; i += RT_THREADS) {
    const int a = i / pw, c = i - a * pw;
    float v = 0.f;
    for (int j = 0; j < K; ++j) v = fmaf(s_t[j], s_p[(a + j) * RB_PW + c], v);
    s_y[a * RB_PW + c] = v;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < gh * gw; i += RT_THREADS) {
    const int a = i / gw, c = i - a * gw, h = y0 - r + a, w = x0 - r + c;
    float gv = 0.f;
    if (h >= r && h < g.H - r && w >= r && w < g.W - r) {
      float v = 0.f;
      for (int k = 0; k < K; ++k) v = fmaf(s_t[RL_KMAX + k], s_y[a * RB_PW + c + k], v);
      const float d = v - Elt<TT>::to_f(target[base + (int64_t)h * g.W + w]);
      // sign(0) = 0; a NaN stays a NaN
      gv = l1 ? (d > 0.f ? kf : (d < 0.f ? -kf : (d == 0.f ? 0.f : d))) : (2.f * kf) * d;
    }
    s_g[a * RB_GW + c] = gv;
  }
  __syncthreads();
  float* s_gx = s_p;  // [gh][RT_W]
  for (int i = threadIdx.x; i < gh * RT_W; i += RT_THREADS) {
    const int a = i / RT_W, lq = i - a * RT_W;
    float v = 0.f;
    for (int k = 0; k < K; ++k) v = fmaf(s_t[RL_KMAX + k], s_g[a * RB_GW + lq - k + 2 * r], v);
    s_gx[i] = v;
  }
  __syncthreads();
  const int lq = threadIdx.x % RT_W, lp0 = threadIdx.x / RT_W, q = x0 + lq;
#pragma unroll
  for (int jj = 0; jj < RT_PER_THREAD; ++jj) {
    const int lp = lp0 + jj * RT_ROWS, p = y0 + lp;
    if (p >= g.H || q >= g.W) continue;
    float v = 0.f;
    for (int j = 0; j < K; ++j) v = fmaf(s_t[j], s_gx[(lp - j + 2 * r) * RT_W + lq], v);
    dpred[base + (int64_t)p * g.W + q] = Elt<PT>::from_f(v);
  }
}

int ceil_div(int a, int b) { return (a + b - 1) / b; }

template <typename PT, typename TT, bool L1>
void launch_fwd_k(int K, unsigned grid, size_t lds, hipStream_t s, const void* pred, const void* target, const float* taps,
                  RegGeom g, float* partial) {
#define REG_FWD(KK)                                                                                                   \
  hipLaunchKernelGGL((reg_fwd_kernel<PT, TT, KK, L1>), dim3(grid), dim3(RT_THREADS), lds, s, (const PT*)pred,         \
                     (const TT*)target, taps, g, partial)
  if (K == 7) REG_FWD(7);
  else if (K == 9) REG_FWD(9);
  else if (K == 11) REG_FWD(11);
  else REG_FWD(13);
#undef REG_FWD
}

template <typename PT, typename TT>
void launch_fwd(int K, unsigned grid, size_t lds, hipStream_t s, const void* pred, const void* target, const float* taps,
                RegGeom g, int l1, float* partial) {
  if (l1) launch_fwd_k<PT, TT, true>(K, grid, lds, s, pred, target, taps, g, partial);
  else launch_fwd_k<PT, TT, false>(K, grid, lds, s, pred, target, taps, g, partial);
}

}  // namespace

extern "C" {

size_t sr_registered_loss_workspace(int B, int C, int H, int W, int S) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || S < 1 || S > RL_SMAX) return 0;
  // B doubles (the selected means), then one row of S^2 partial sums per tile; the tiles of the crop are no more
  // than those of the image
  return (size_t)B * sizeof(double) +
         (size_t)B * C * ceil_div(H, RT_H) * ceil_div(W, RT_W) * (size_t)(S * S) * sizeof(float);
}

int sr_registered_loss(int kind, int reduction, int pred_dtype, int target_dtype, const void* pred, const void* target,
                       const float* taps, int S, int K, int B, int C, int H, int W, float loss_weight, float* loss,
                       int* idx, float* table, void* grad, void* workspace, size_t ws_bytes, void* stream) {
  static thread_local char msg[160];
  const char* why = nullptr;
  if (kind != SR_LOSS_L1 && kind != SR_LOSS_MSE) why = "kind must be SR_LOSS_L1 or SR_LOSS_MSE";
  else if (reduction != SR_REDUCE_NONE && reduction != SR_REDUCE_MEAN && reduction != SR_REDUCE_SUM) why = "unknown reduction";
  else if (S < 1 || S > RL_SMAX) why = "S must be 1 to 9";
  else if (K < RL_KMIN || K > RL_KMAX || K % 2 == 0) why = "K must be odd, 7 to 13";
  else if (B < 1 || C < 1) why = "B and C must be positive";
  else if (H < K || W < K) why = "H and W must be at least K = 2r + 1";
  else if ((int64_t)B * C * H * W >= (1ll << 31)) why = "B*C*H*W must be below 2^31";
  else if ((pred_dtype != SR_F32 && pred_dtype != SR_BF16) || (target_dtype != SR_F32 && target_dtype != pred_dtype))
    why = "pred must be fp32 or bf16, target fp32 or pred's dtype";
  else if (!pred || !target || !taps || !loss || !idx || !workspace) why = "null pointer";
  else if (ws_bytes < sr_registered_loss_workspace(B, C, H, W, S)) why = "workspace too small";
  else {
    const int psz = pred_dtype == SR_BF16 ? 2 : 4, tsz = target_dtype == SR_BF16 ? 2 : 4;
    if ((((uintptr_t)pred | (uintptr_t)grad) & (psz - 1)) || ((uintptr_t)target & (tsz - 1)) ||
        (((uintptr_t)taps | (uintptr_t)loss | (uintptr_t)idx | (uintptr_t)table) & 3) || ((uintptr_t)workspace & 7))
      why = "tensors must be element-aligned, the workspace 8-byte aligned";
  }
  if (why) {
    snprintf(msg, sizeof(msg), "registered_loss: %s", why);
    return sr_fail(SR_EINVAL, msg);
  }

  const int r = K / 2, Hc = H - 2 * r, Wc = W - 2 * r, S2 = S * S;
  RegGeom g;
  g.B = B, g.C = C, g.H = H, g.W = W, g.S = S, g.K = K;
  g.tx = ceil_div(Wc, RT_W), g.ty = ceil_div(Hc, RT_H);
  g.bx = ceil_div(W, RT_W), g.by = ceil_div(H, RT_H);
  hipStream_t s = (hipStream_t)stream;
  double* minloss = (double*)workspace;
  float* partial = (float*)(minloss + B);
  const int l1 = kind == SR_LOSS_L1;
  const int pw = RT_W + 2 * r;
  const size_t lds = (size_t)((RT_H + 2 * r) * pw + S * RT_H * pw) * sizeof(float);
  const unsigned fgrid = (unsigned)((int64_t)B * C * g.tx * g.ty);
  if (pred_dtype == SR_F32) launch_fwd<float, float>(K, fgrid, lds, s, pred, target, taps, g, l1, partial);
  else if (target_dtype == SR_F32) launch_fwd<bf16_t, float>(K, fgrid, lds, s, pred, target, taps, g, l1, partial);
  else launch_fwd<bf16_t, bf16_t>(K, fgrid, lds, s, pred, target, taps, g, l1, partial);

  const double n = (double)C * Hc * Wc;
  const int none = reduction == SR_REDUCE_NONE;
  hipLaunchKernelGGL(reg_finalize_kernel, dim3(B), dim3(RF_THREADS), 0, s, (const float*)partial, C * g.tx * g.ty, S2, n,
                     loss_weight, none, idx, table, minloss, loss);
  const double kb = reduction == SR_REDUCE_MEAN ? (double)loss_weight / B : (double)loss_weight;
  if (!none) hipLaunchKernelGGL(reg_reduce_kernel, dim3(1), dim3(64), 0, s, (const double*)minloss, B, kb, loss);

  if (grad) {
    const float kf = (float)(kb / n);
    const unsigned bgrid = (unsigned)((int64_t)B * C * g.bx * g.by);
    if (pred_dtype == SR_F32)
      hipLaunchKernelGGL((reg_bwd_kernel<float, float>), dim3(bgrid), dim3(RT_THREADS), 0, s, (const float*)pred,
                         (const float*)target, taps, (const int*)idx, g, l1, kf, (float*)grad);
    else if (target_dtype == SR_F32)
      hipLaunchKernelGGL((reg_bwd_kernel<bf16_t, float>), dim3(bgrid), dim3(RT_THREADS), 0, s, (const bf16_t*)pred,
                         (const float*)target, taps, (const int*)idx, g, l1, kf, (bf16_t*)grad);
    else
      hipLaunchKernelGGL((reg_bwd_kernel<bf16_t, bf16_t>), dim3(bgrid), dim3(RT_THREADS), 0, s, (const bf16_t*)pred,
                         (const bf16_t*)target, taps, (const int*)idx, g, l1, kf, (bf16_t*)grad);
  }
  return sr_check(hipGetLastError(), "registered_loss launch");
}

}  // extern "C"
