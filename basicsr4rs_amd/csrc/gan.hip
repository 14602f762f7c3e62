// Kernels of the VGG-style discriminator (basicsr/archs/discriminator_arch.py) that the conv engine does not
// cover: the 4x4 stride-2 pad-1 convolution, BatchNorm2d with a fused LeakyReLU, and the two head linears.
//
//   conv4s2_prep_kernel : the GEMM images of an nn.Conv2d(cin, cout, 4, 2, 1) weight.
//       wf [Cout][16 * Cin], wf[co][t * Cin + ci] = w[co][ci][kh][kw], t = kh * 4 + kw (forward);
//       wd [4][Cin][4 * Cout], wd[cls][ci][t * Cout + co] = w[co][ci][kh][kw] with cls = ph * 2 + pw the
//       (row, column) parity of the input pixel, t = th * 2 + tw, kh = 1 - ph + 2 th, kw = 1 - pw + 2 tw
//       (dgrad); padded channels are zeros.
//   conv4s2_gemm_kernel : forward and dgrad, one implicit GEMM.  A block owns 64 pixels x 64 output channels
//       and walks K in steps of 64: the pixel operand is GATHERED tap by tap (16 bytes = 8 bf16 / 4 fp32
//       channels of one tap, zeros outside the map), the weight operand is a row of the image.  MFMA:
//       v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x4_f32, fp32 accumulation, 4 waves = 2 x 2 of 32 x 32.
//       Forward: pixel (n, oh, ow) reads x[2 oh - 1 + kh][2 ow - 1 + kw], K = 16 Cin; an optional LeakyReLU on
//       the fp32 sums before the store (sr_conv4s2_fwd_act: the U-Net discriminator, where no BatchNorm follows).
//       Dgrad: ih = 2 oh - 1 + kh means an input row of parity ph meets only the two kh = 1 - ph + 2 th, from
//       output rows oh = a + ph - th (ih = 2 a + ph); the same per column: each of the four parity classes
//       (grid z) is a GEMM with K = 4 Cout over dy, written to its own pixels of dx.  Every dx element is
//       written exactly once: a gather, no scatter, 16 tap products per pixel instead of the 36 of a
//       pixel-unshuffled 3x3.
//   conv4s2_wgrad_kernel + conv4s2_wgrad_reduce_kernel : dW[co][t][ci] = sum over the N Ho Wo output pixels of
//       dy[pix][co] * x[tap t of pix][ci].  Both operands are staged TRANSPOSED in LDS ([channel][pixel]), the
//       x operand gathered.  Split K (c4_plan): S blocks of kb pixels write fp32 partials [S][Cout][16 Cin];
//       the reduce sums them in split order, scales, and writes (or accumulates into) the parameter layout
//       [cout][cin][4][4].
//   bn_stats_kernel + bn_stats_final_kernel : per-channel mean and biased variance over the N H W rows of an
//       NHWC map.  A thread runs Welford's update over its rows for one 16-byte channel vector; the threads
//       of a block and then the blocks are merged with Chan's (count, mean, M2) rule in a fixed order (the blocks
//       in 16 runs of consecutive blocks, then the 16 results): no E[x^2] - E[x]^2, so a mean far from zero
//       does not cancel.  The final kernel leaves save_mean,
//       save_rstd and updates the running statistics (unbiased variance; momentum < 0: the cumulative
//       average 1 / num_batches_tracked, read from the device).
//   bn_apply_kernel : y = act(gamma * (x - mean) * rstd + beta), act none / LeakyReLU.
//   bn_bwd_reduce_kernel + bn_bwd_final_kernel : dbeta = sum g, dgamma = sum g * xhat, g = dy times the
//       activation gate recomputed from x; block partials, folded in the same two-level fixed order.
//   bn_bwd_dx_kernel : dx = rstd * gamma * (g - dbeta / M - xhat * dgamma / M) (training),
//       dx = g * gamma * rstd (eval).
//   fc_fwd_kernel / fc_dgrad_kernel / fc_wgrad_kernel : y = act(x W^T + b) on the fp32 nn.Linear weight as
//       it is.  With P > 1 the feature index of x is NHWC ((h w) * C + c) and the weight's is the
//       reference's NCHW flatten (c * P + (h w)): the kernels walk the weight's order and permute on the x
//       side, so the gradient comes back in the parameter's own order.
//
// No atomics, fixed summation orders: two runs give identical bits.  Nothing allocates or synchronises.
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int G_THREADS = 256;
constexpr int G_MAX_BLOCKS = 8192;
constexpr int C4_TILE = 64;
constexpr int C4_KT = 64;
constexpr int C4_KBLOCK = 256;      // output pixels per split-K block of the wgrad (times m, c4_plan)
constexpr int C4_MAX_SPLITS = 64;
constexpr int C4_BLOCK_TARGET = 2048;
constexpr int BN_MAX_BLOCKS = 256;
constexpr int BN_MIN_ROWS = 64;
constexpr int BN_FG = 16;                  // thread groups of a final merge, each over a run of block partials
constexpr int BN_FC = G_THREADS / BN_FG;  // channels per block of a final merge

template <typename T, int V>
SR_DEV void ld16(const T* __restrict__ p, float (&v)[V]) {
  if constexpr (sizeof(T) == 4) {
    const f32x4 x = *(const f32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x[k];
  } else {
    const u32x4 x = *(const u32x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = bf16_to_f32((unsigned short)(x[k] & 0xffff));
      v[2 * k + 1] = bf16_to_f32((unsigned short)(x[k] >> 16));
    }
  }
}

template <typename T, int V>
SR_DEV void st16(T* __restrict__ p, const float (&v)[V]) {
  if constexpr (sizeof(T) == 4) {
    f32x4 x;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = v[k];
    *(f32x4*)p = x;
  } else {
    u32x4 x;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
    *(u32x4*)p = x;
  }
}

template <typename T>
SR_DEV void mfma_k(const u32x4& a, const u32x4& b, f32x4& acc) {
  if constexpr (sizeof(T) == 2) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), acc, 0, 0,
                                                  0);
  } else {
    // a 16-byte fragment = 4 consecutive k per lane: four K = 4 MFMAs, A and B with the same lane -> k map
#pragma unroll
    for (int s = 0; s < 4; ++s)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[s]), __uint_as_float(b[s]), acc, 0, 0, 0);
  }
}

unsigned g_grid(int64_t n) {
  int64_t g = (n + G_THREADS - 1) / G_THREADS;
  if (g > G_MAX_BLOCKS) g = G_MAX_BLOCKS;
  return (unsigned)(g < 1 ? 1 : g);
}

bool dtype_ok(int dtype) { return dtype == SR_F32 || dtype == SR_BF16; }

// ---------------------------------------------------------------------------------------- conv 4x4 stride 2

template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    conv4s2_prep_kernel(const float* __restrict__ w, int cout_real, int cin_real, int Cout, int Cin, T* __restrict__ wf,
                        T* __restrict__ wd) {
  const uint32_t nf = (uint32_t)Cout * 16u * Cin;
  for (uint32_t i = blockIdx.x * G_THREADS + threadIdx.x; i < 2u * nf; i += gridDim.x * G_THREADS) {
    int co, ci, kh, kw;
    if (i < nf) {
      co = i / (16u * Cin);
      const uint32_t r = i - (uint32_t)co * 16u * Cin;
      const int t = r / Cin;
      ci = r - t * Cin, kh = t >> 2, kw = t & 3;
    } else {
      const uint32_t e = i - nf;
      const int cls = e / ((uint32_t)Cin * 4u * Cout);
      uint32_t r = e - (uint32_t)cls * Cin * 4u * Cout;
      ci = r / (4u * Cout);
      r -= (uint32_t)ci * 4u * Cout;
      const int t = r / Cout;
      co = r - t * Cout;
      kh = 1 - (cls >> 1) + 2 * (t >> 1), kw = 1 - (cls & 1) + 2 * (t & 1);
    }
    float v = 0.f;
    if (co < cout_real && ci < cin_real) v = w[(((size_t)co * cin_real + ci) * 4 + kh) * 4 + kw];
    if (i < nf) wf[i] = Elt<T>::from_f(v);
    else wd[i - nf] = Elt<T>::from_f(v);
  }
}

struct C4Args {
  int Hs, Ws, Cs;  // the gathered map (x forward, dy dgrad): size and channels
  int Hr, Wr;      // pixel grid of a GEMM's rows per image
  int M;           // N * Hr * Wr
  int K, Nout;     // reduction length (taps * Cs) and output channels
  int Hd, Wd;      // the written map
  int act;         // forward epilogue: 0 none, 2 LeakyReLU(slope)
  float slope;
  FastDiv fd_w, fd_hw, fd_cs;
};

// MODE 0 forward (source pixel 2 r - 1 + kh, written pixel r), MODE 1 dgrad (source pixel r + ph - th, written
// pixel 2 r + ph; grid z = parity class)
template <typename T, int MODE>
__global__ void __launch_bounds__(G_THREADS)
    conv4s2_gemm_kernel(const T* __restrict__ src, const T* __restrict__ wimg, T* __restrict__ dst, C4Args a) {
  constexpr int V = Elt<T>::PER16;
  constexpr int LDT = C4_KT + V;
  constexpr int CG = C4_KT / V;
  constexpr int SL = C4_TILE * CG / G_THREADS;  // vectors a thread stages per operand and step
  __shared__ __attribute__((aligned(16))) T sP[C4_TILE * LDT];
  __shared__ __attribute__((aligned(16))) T sW[C4_TILE * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * C4_TILE, n0 = blockIdx.y * C4_TILE;
  const int cls = MODE ? (int)blockIdx.z : 0, ph = cls >> 1, pw = cls & 1;
  const T* W = wimg + (size_t)cls * a.Nout * a.K;
  const int HrWr = a.Hr * a.Wr;

  // the rows this thread stages: their image and grid position (fixed over the K loop)
  int p_img[SL], p_r[SL], p_c[SL];
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    const int rl = (tid + s * G_THREADS) / CG, m = m0 + rl;
    if (m < a.M) {
      const uint32_t img = fdiv((uint32_t)m, a.fd_hw), rem = (uint32_t)m - img * HrWr;
      const uint32_t r = fdiv(rem, a.fd_w);
      p_img[s] = (int)img, p_r[s] = (int)r, p_c[s] = (int)(rem - r * a.Wr);
    } else {
      p_img[s] = -1, p_r[s] = 0, p_c[s] = 0;
    }
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < a.K; k0 += C4_KT) {
#pragma unroll
    for (int s = 0; s < SL; ++s) {
      const int v = tid + s * G_THREADS, rl = v / CG, cg = v - rl * CG;
      const int k = k0 + cg * V;
      u32x4 q = u32x4{0u, 0u, 0u, 0u}, qw = u32x4{0u, 0u, 0u, 0u};
      if (k < a.K) {
        if (p_img[s] >= 0) {
          const int t = (int)fdiv((uint32_t)k, a.fd_cs), ch = k - t * a.Cs;
          int sh, sw;
          if constexpr (MODE == 0) {
            sh = 2 * p_r[s] - 1 + (t >> 2), sw = 2 * p_c[s] - 1 + (t & 3);
          } else {
            sh = p_r[s] + ph - (t >> 1), sw = p_c[s] + pw - (t & 1);
          }
          if (sh >= 0 && sh < a.Hs && sw >= 0 && sw < a.Ws)
            q = *(const u32x4*)(src + (((size_t)p_img[s] * a.Hs + sh) * a.Ws + sw) * a.Cs + ch);
        }
        const int j = n0 + rl;
        if (j < a.Nout) qw = *(const u32x4*)(W + (size_t)j * a.K + k);
      }
      *(u32x4*)(sP + rl * LDT + cg * V) = q;
      *(u32x4*)(sW + rl * LDT + cg * V) = qw;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < C4_KT; kk += 4 * V) {
      u32x4 wv[2], pv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        wv[i] = *(const u32x4*)(sW + (wr * 32 + i * 16 + fr) * LDT + kk + fq * V);
        pv[i] = *(const u32x4*)(sP + (wc * 32 + i * 16 + fr) * LDT + kk + fq * V);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mfma_k<T>(wv[i], pv[j], acc[i][j]);
    }
    __syncthreads();
  }

  // acc[i][j][r]: output channel n0 + wr * 32 + i * 16 + fq * 4 + r of pixel m0 + wc * 32 + j * 16 + fr
  if (MODE == 0 && a.act == 2) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = acc[i][j][r] > 0.f ? acc[i][j][r] : acc[i][j][r] * a.slope;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wc * 32 + j * 16 + fr;
    if (m >= a.M) continue;
    const uint32_t img = fdiv((uint32_t)m, a.fd_hw), rem = (uint32_t)m - img * HrWr;
    const uint32_t r = fdiv(rem, a.fd_w), c = rem - r * a.Wr;
    const int dh = MODE ? 2 * (int)r + ph : (int)r, dw = MODE ? 2 * (int)c + pw : (int)c;
    T* o = dst + (((size_t)img * a.Hd + dh) * a.Wd + dw) * a.Nout;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int co = n0 + wr * 32 + i * 16 + fq * 4;
      if (co >= a.Nout) continue;  // Nout % 8 == 0: the four channels are inside together
      if constexpr (sizeof(T) == 4) {
        *(f32x4*)(o + co) = acc[i][j];
      } else {
        *(u32x2*)(o + co) = u32x2{pack_bf16x2(acc[i][j][0], acc[i][j][1]), pack_bf16x2(acc[i][j][2], acc[i][j][3])};
      }
    }
  }
}

struct C4WArgs {
  int N, H, W, Cin, Ho, Wo, Cout;
  int Mr;  // N * Ho * Wo
  int KW;  // 16 * Cin
  int tiles_col, S, kb;
  FastDiv fd_wo, fd_howo, fd_cin;
};

// grid (tiles_co * tiles_col, S): part[sp][co][t * Cin + ci]
template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    conv4s2_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part, C4WArgs a) {
  constexpr int V = Elt<T>::PER16;
  constexpr int LDT = C4_KT + V;
  constexpr int CG = C4_TILE / V;
  constexpr int SL = C4_KT * CG / G_THREADS;
  __shared__ __attribute__((aligned(16))) T sA[C4_TILE * LDT];
  __shared__ __attribute__((aligned(16))) T sB[C4_TILE * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int tc = blockIdx.x / a.tiles_col, tl = blockIdx.x - tc * a.tiles_col, sp = blockIdx.y;
  const int co0 = tc * C4_TILE, col0 = tl * C4_TILE;
  const int k_begin = sp * a.kb, k_end = min(a.Mr, k_begin + a.kb);
  const int HoWo = a.Ho * a.Wo;
  // cg = (tid + s * 256) % CG is the same for every s (256 % CG == 0): one column vector per thread
  const int cg = tid % CG;
  const int col = col0 + cg * V, cdy = co0 + cg * V;
  const int tap = col < a.KW ? (int)fdiv((uint32_t)col, a.fd_cin) : 0, ci = col - tap * a.Cin;
  const int kh = tap >> 2, kw = tap & 3;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto put = [&](T* dstp, int kl, const u32x4& q) {
    T* d = dstp + (cg * V) * LDT + kl;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        d[(2 * j) * LDT] = (T)(q[j] & 0xffff);
        d[(2 * j + 1) * LDT] = (T)(q[j] >> 16);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j * LDT] = __uint_as_float(q[j]);
    }
  };

  for (int k0 = k_begin; k0 < k_end; k0 += C4_KT) {
#pragma unroll
    for (int s = 0; s < SL; ++s) {
      const int kl = (tid + s * G_THREADS) / CG, k = k0 + kl;
      u32x4 qa = u32x4{0u, 0u, 0u, 0u}, qb = u32x4{0u, 0u, 0u, 0u};
      if (k < k_end) {
        if (cdy < a.Cout) qa = *(const u32x4*)(dy + (size_t)k * a.Cout + cdy);
        if (col < a.KW) {
          const uint32_t img = fdiv((uint32_t)k, a.fd_howo), rem = (uint32_t)k - img * HoWo;
          const uint32_t oh = fdiv(rem, a.fd_wo), ow = rem - oh * a.Wo;
          const int ih = 2 * (int)oh - 1 + kh, iw = 2 * (int)ow - 1 + kw;
          if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
            qb = *(const u32x4*)(x + (((size_t)img * a.H + ih) * a.W + iw) * a.Cin + ci);
        }
      }
      put(sA, kl, qa);
      put(sB, kl, qb);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < C4_KT; kk += 4 * V) {
      u32x4 av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        av[i] = *(const u32x4*)(sA + (wr * 32 + i * 16 + fr) * LDT + kk + fq * V);
        bv[i] = *(const u32x4*)(sB + (wc * 32 + i * 16 + fr) * LDT + kk + fq * V);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mfma_k<T>(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }

  float* out = part + (size_t)sp * a.Cout * a.KW;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gco = co0 + wr * 32 + i * 16 + fq * 4 + r, gcol = col0 + wc * 32 + j * 16 + fr;
        if (gco < a.Cout && gcol < a.KW) out[(size_t)gco * a.KW + gcol] = acc[i][j][r];
      }
}

// dw[co][ci][kh][kw] (=, or += with accumulate) scale * sum over s of part[s][co][(kh * 4 + kw) * Cin + ci]
__global__ void __launch_bounds__(G_THREADS)
    conv4s2_wgrad_reduce_kernel(const float* __restrict__ part, int S, int Cout, int Cin, int cout_real, int cin_real,
                                float scale, int accumulate, float* __restrict__ dw) {
  const uint32_t total = (uint32_t)cout_real * cin_real * 16u;
  const size_t KW = (size_t)16 * Cin, stride = (size_t)Cout * KW;
  for (uint32_t i = blockIdx.x * G_THREADS + threadIdx.x; i < total; i += gridDim.x * G_THREADS) {
    const uint32_t t = i & 15u, cc = i >> 4;
    const uint32_t co = cc / (uint32_t)cin_real, ci = cc - co * cin_real;
    const float* p = part + (size_t)co * KW + (size_t)t * Cin + ci;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += p[(size_t)k * stride];
    s *= scale;
    dw[i] = accumulate ? dw[i] + s : s;
  }
}

void c4_plan(int Mr, int Cout, int Cin, int& S, int& kb, int& tiles_co, int& tiles_col) {
  tiles_co = (Cout + C4_TILE - 1) / C4_TILE;
  tiles_col = (16 * Cin + C4_TILE - 1) / C4_TILE;
  int smax = C4_BLOCK_TARGET / (tiles_co * tiles_col);
  smax = smax < 1 ? 1 : (smax > C4_MAX_SPLITS ? C4_MAX_SPLITS : smax);
  const int64_t blocks = ((int64_t)Mr + C4_KBLOCK - 1) / C4_KBLOCK;
  const int64_t m = (blocks + smax - 1) / smax;
  kb = (int)(C4_KBLOCK * (m < 1 ? 1 : m));
  S = (int)(((int64_t)Mr + kb - 1) / kb);
}

int c4_check(const char* what, int dtype, int N, int H, int W, int Cin, int Cout) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    return sr_fail(code, msg);
  };
  if (!dtype_ok(dtype)) return fail(SR_EINVAL, "dtype must be fp32 or bf16");
  if (N <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1)) return fail(SR_EINVAL, "H and W must be even and at least 2");
  if (Cin < 8 || Cout < 8 || Cin > 512 || Cout > 512 || Cin % 8 || Cout % 8)
    return fail(SR_EINVAL, "channels must be multiples of 8 from 8 to 512");
  const int64_t esz = dtype == SR_BF16 ? 2 : 4;
  if ((int64_t)N * H * W * Cin * esz >= 0x80000000ll || (int64_t)N * (H / 2) * (W / 2) * Cout * esz >= 0x80000000ll)
    return fail(SR_ETOOBIG, "tensor too large");
  return SR_OK;
}

template <typename T, int MODE>
void c4_launch(const void* src, const void* wimg, void* dst, const C4Args& a, int classes, hipStream_t s) {
  const dim3 grid((unsigned)((a.M + C4_TILE - 1) / C4_TILE), (unsigned)((a.Nout + C4_TILE - 1) / C4_TILE), (unsigned)classes);
  hipLaunchKernelGGL((conv4s2_gemm_kernel<T, MODE>), grid, dim3(G_THREADS), 0, s, (const T*)src, (const T*)wimg, (T*)dst, a);
}

// ---------------------------------------------------------------------------------------------- batch norm

// Chan's merge of (na, ma, Ma) with (nb, mb, Mb)
SR_DEV void chan_merge(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
  if (nb == 0.f) return;
  const float n = na + nb, d = mb - ma, f = nb / n;
  ma += d * f;
  Ma += Mb + d * d * na * f;
  na = n;
}

// (x - mean) * rstd of V channels starting at c0; rstd from the variance when use_var
template <int V>
SR_DEV void bn_coeffs(const float* __restrict__ mean, const float* __restrict__ rv, int use_var, float eps, int c0,
                      float (&mu)[V], float (&rs)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) {
    mu[k] = mean[c0 + k];
    rs[k] = use_var ? 1.f / sqrtf(rv[c0 + k] + eps) : rv[c0 + k];
  }
}

SR_DEV float bn_gate(float z, int act, float slope) { return act == 2 ? (z > 0.f ? 1.f : slope) : 1.f; }

// grid B blocks of rpb rows; partial [B][3][C] = (count, mean, M2)
template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    bn_stats_kernel(const T* __restrict__ x, int M, int C, int rpb, float* __restrict__ partial) {
  constexpr int V = Elt<T>::PER16;
  __shared__ float s_mean[G_THREADS * V], s_m2[G_THREADS * V], s_n[G_THREADS];
  const int CV = C / V, RL = G_THREADS / CV;
  const int tid = threadIdx.x, rl = tid / CV, cv = tid - rl * CV;
  const int r0 = blockIdx.x * rpb, r1 = min(M, r0 + rpb);
  float mean[V], m2[V], n = 0.f;
#pragma unroll
  for (int k = 0; k < V; ++k) mean[k] = 0.f, m2[k] = 0.f;
  if (rl < RL)
    for (int r = r0 + rl; r < r1; r += RL) {
      float v[V];
      ld16<T, V>(x + (size_t)r * C + cv * V, v);
      n += 1.f;
      const float inv = 1.f / n;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float d = v[k] - mean[k];
        mean[k] += d * inv;
        m2[k] += d * (v[k] - mean[k]);
      }
    }
  s_n[tid] = n;
#pragma unroll
  for (int k = 0; k < V; ++k) s_mean[tid * V + k] = mean[k], s_m2[tid * V + k] = m2[k];
  __syncthreads();
  for (int c = tid; c < C; c += G_THREADS) {
    const int cvv = c / V, k = c - cvv * V;
    float na = 0.f, ma = 0.f, Ma = 0.f;
    for (int j = 0; j < RL; ++j) {
      const int t = j * CV + cvv;
      chan_merge(na, ma, Ma, s_n[t], s_mean[t * V + k], s_m2[t * V + k]);
    }
    float* p = partial + (size_t)blockIdx.x * 3 * C + c;
    p[0] = na, p[C] = ma, p[2 * C] = Ma;
  }
}

// A block owns BN_FC channels; group g of its BN_FG thread groups merges the g-th run of consecutive block
// partials in block order, then the first group merges the BN_FG results in group order: a fixed order with a
// dependent chain of B / BN_FG + BN_FG merges instead of B.
__global__ void __launch_bounds__(G_THREADS)
    bn_stats_final_kernel(const float* __restrict__ partial, int B, int C, int M, float eps, float momentum,
                          const int64_t* __restrict__ nbt, float* __restrict__ save_mean, float* __restrict__ save_rstd,
                          float* __restrict__ running_mean, float* __restrict__ running_var) {
  __shared__ float s_n[G_THREADS], s_m[G_THREADS], s_M[G_THREADS];
  const int tid = threadIdx.x, cl = tid % BN_FC, grp = tid / BN_FC;
  const int c = blockIdx.x * BN_FC + cl;
  const int per = (B + BN_FG - 1) / BN_FG, b0 = grp * per, b1 = min(B, b0 + per);
  float na = 0.f, ma = 0.f, Ma = 0.f;
  if (c < C)
    for (int b = b0; b < b1; ++b) {
      const float* p = partial + (size_t)b * 3 * C + c;
      chan_merge(na, ma, Ma, p[0], p[C], p[2 * C]);
    }
  s_n[tid] = na, s_m[tid] = ma, s_M[tid] = Ma;
  __syncthreads();
  if (grp != 0 || c >= C) return;
  na = 0.f, ma = 0.f, Ma = 0.f;
  for (int g = 0; g < BN_FG; ++g) chan_merge(na, ma, Ma, s_n[g * BN_FC + cl], s_m[g * BN_FC + cl], s_M[g * BN_FC + cl]);
  const float var = Ma / (float)M;
  save_mean[c] = ma;
  save_rstd[c] = 1.f / sqrtf(var + eps);
  if (running_mean) {
    const float f = momentum < 0.f ? 1.f / (float)(*nbt) : momentum;
    running_mean[c] = (1.f - f) * running_mean[c] + f * ma;
    running_var[c] = (1.f - f) * running_var[c] + f * (Ma / (float)(M - 1));
  }
}

template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    bn_apply_kernel(const T* __restrict__ x, T* __restrict__ y, uint32_t total, int CV, FastDiv fd_cv,
                    const float* __restrict__ mean, const float* __restrict__ rv, int use_var, float eps,
                    const float* __restrict__ gamma, const float* __restrict__ beta, int act, float slope) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * G_THREADS + threadIdx.x; i < total; i += gridDim.x * G_THREADS) {
    const int c0 = (int)(i - fdiv(i, fd_cv) * CV) * V;
    float v[V], mu[V], rs[V];
    ld16<T, V>(x + (size_t)i * V, v);
    bn_coeffs<V>(mean, rv, use_var, eps, c0, mu, rs);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float z = gamma[c0 + k] * ((v[k] - mu[k]) * rs[k]) + beta[c0 + k];
      v[k] = act == 2 ? (z > 0.f ? z : z * slope) : z;
    }
    st16<T, V>(y + (size_t)i * V, v);
  }
}

// partial [B][2][C] = (sum g, sum g * xhat)
template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    bn_bwd_reduce_kernel(const T* __restrict__ x, const T* __restrict__ dy, int M, int C, int rpb,
                         const float* __restrict__ mean, const float* __restrict__ rv, int use_var, float eps,
                         const float* __restrict__ gamma, const float* __restrict__ beta, int act, float slope,
                         float* __restrict__ partial) {
  constexpr int V = Elt<T>::PER16;
  __shared__ float s_b[G_THREADS * V], s_g[G_THREADS * V];
  const int CV = C / V, RL = G_THREADS / CV;
  const int tid = threadIdx.x, rl = tid / CV, cv = tid - rl * CV;
  const int r0 = blockIdx.x * rpb, r1 = min(M, r0 + rpb);
  float sb[V], sg[V];
#pragma unroll
  for (int k = 0; k < V; ++k) sb[k] = 0.f, sg[k] = 0.f;
  if (rl < RL) {
    float mu[V], rs[V], ga[V], be[V];
    bn_coeffs<V>(mean, rv, use_var, eps, cv * V, mu, rs);
#pragma unroll
    for (int k = 0; k < V; ++k) ga[k] = gamma[cv * V + k], be[k] = beta[cv * V + k];
    for (int r = r0 + rl; r < r1; r += RL) {
      float v[V], g[V];
      ld16<T, V>(x + (size_t)r * C + cv * V, v);
      ld16<T, V>(dy + (size_t)r * C + cv * V, g);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float xh = (v[k] - mu[k]) * rs[k];
        const float gg = g[k] * bn_gate(ga[k] * xh + be[k], act, slope);
        sb[k] += gg;
        sg[k] += gg * xh;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < V; ++k) s_b[tid * V + k] = sb[k], s_g[tid * V + k] = sg[k];
  __syncthreads();
  for (int c = tid; c < C; c += G_THREADS) {
    const int cvv = c / V, k = c - cvv * V;
    float b = 0.f, g = 0.f;
    for (int j = 0; j < RL; ++j) {
      const int t = j * CV + cvv;
      b += s_b[t * V + k], g += s_g[t * V + k];
    }
    float* p = partial + (size_t)blockIdx.x * 2 * C + c;
    p[0] = b, p[C] = g;
  }
}

// the same two-level fixed order as bn_stats_final_kernel, with plain sums
__global__ void __launch_bounds__(G_THREADS)
    bn_bwd_final_kernel(const float* __restrict__ partial, int B, int C, float* __restrict__ dgamma,
                        float* __restrict__ dbeta) {
  __shared__ float s_b[G_THREADS], s_g[G_THREADS];
  const int tid = threadIdx.x, cl = tid % BN_FC, grp = tid / BN_FC;
  const int c = blockIdx.x * BN_FC + cl;
  const int per = (B + BN_FG - 1) / BN_FG, b0 = grp * per, b1 = min(B, b0 + per);
  float b = 0.f, g = 0.f;
  if (c < C)
    for (int k = b0; k < b1; ++k) {
      const float* p = partial + (size_t)k * 2 * C + c;
      b += p[0], g += p[C];
    }
  s_b[tid] = b, s_g[tid] = g;
  __syncthreads();
  if (grp != 0 || c >= C) return;
  b = 0.f, g = 0.f;
  for (int k = 0; k < BN_FG; ++k) b += s_b[k * BN_FC + cl], g += s_g[k * BN_FC + cl];
  dbeta[c] = b, dgamma[c] = g;
}

template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    bn_bwd_dx_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, uint32_t total, int CV,
                     FastDiv fd_cv, const float* __restrict__ mean, const float* __restrict__ rv, int use_var, float eps,
                     const float* __restrict__ gamma, const float* __restrict__ beta, int act, float slope,
                     const float* __restrict__ dgamma, const float* __restrict__ dbeta, int training, float inv_m) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * G_THREADS + threadIdx.x; i < total; i += gridDim.x * G_THREADS) {
    const int c0 = (int)(i - fdiv(i, fd_cv) * CV) * V;
    float v[V], g[V], mu[V], rs[V];
    ld16<T, V>(x + (size_t)i * V, v);
    ld16<T, V>(dy + (size_t)i * V, g);
    bn_coeffs<V>(mean, rv, use_var, eps, c0, mu, rs);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float ga = gamma[c0 + k], xh = (v[k] - mu[k]) * rs[k];
      const float gg = g[k] * bn_gate(ga * xh + beta[c0 + k], act, slope);
      v[k] = training ? rs[k] * ga * (gg - dbeta[c0 + k] * inv_m - xh * (dgamma[c0 + k] * inv_m)) : gg * ga * rs[k];
    }
    st16<T, V>(dx + (size_t)i * V, v);
  }
}

void bn_plan(int64_t M, int& B, int& rpb) {
  int64_t r = (M + BN_MAX_BLOCKS - 1) / BN_MAX_BLOCKS;
  if (r < BN_MIN_ROWS) r = BN_MIN_ROWS;
  rpb = (int)r;
  B = (int)((M + r - 1) / r);
}

int bn_check(const char* what, int dtype, int64_t M, int C, int act) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    return sr_fail(code, msg);
  };
  if (!dtype_ok(dtype)) return fail(SR_EINVAL, "dtype must be fp32 or bf16");
  if (M <= 0 || C < 8 || C % 8 || C > 1024) return fail(SR_EINVAL, "bad arguments (C a multiple of 8 up to 1024)");
  if (act != 0 && act != 2) return fail(SR_EINVAL, "act must be none (0) or LeakyReLU (2)");
  // the Welford / Chan counts are fp32: exact up to 2^24 rows per channel
  if (M > (1ll << 24)) return fail(SR_ETOOBIG, "more than 2^24 rows per channel");
  if (M * C * (dtype == SR_BF16 ? 2 : 4) >= 0x80000000ll) return fail(SR_ETOOBIG, "tensor too large");
  return SR_OK;
}

// ------------------------------------------------------------------------------------------- head linears

// weight index j = c * P + p  <->  x index p * C + c (C = K / P); P == 1: the same index
SR_DEV int fc_xidx(int j, int P, int C, FastDiv fd_p) {
  if (P == 1) return j;
  const int c = (int)fdiv((uint32_t)j, fd_p), p = j - c * P;
  return p * C + c;
}

SR_DEV float fc_block_sum(float s) {
  __shared__ float red[G_THREADS];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = G_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// grid (O, M): y[m][o] = act(sum_j x[m][xidx(j)] w[o][j] + b[o])
template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    fc_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, int K, int O, int P,
                  FastDiv fd_p, int act, float slope, float* __restrict__ y) {
  const int o = blockIdx.x, m = blockIdx.y, C = K / P;
  const T* xr = x + (size_t)m * K;
  const float* wr = w + (size_t)o * K;
  float s = 0.f;
  for (int j = threadIdx.x; j < K; j += G_THREADS) s += Elt<T>::to_f(xr[fc_xidx(j, P, C, fd_p)]) * wr[j];
  s = fc_block_sum(s);
  if (threadIdx.x == 0) {
    const float z = s + (b ? b[o] : 0.f);
    y[(size_t)m * O + o] = act == 2 ? (z > 0.f ? z : z * slope) : z;
  }
}

// g[m][o] = dy[m][o] * gate(y[m][o])
SR_DEV float fc_g(const float* __restrict__ dy, const float* __restrict__ y, size_t i, float slope) {
  const float g = dy[i];
  return y ? (y[i] > 0.f ? g : g * slope) : g;
}

// one thread per (m, j): dx[m][xidx(j)] = sum_o g[m][o] w[o][j]
template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    fc_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ w, int M, int K,
                    int O, int P, FastDiv fd_p, FastDiv fd_k, float slope, T* __restrict__ dx) {
  const uint32_t total = (uint32_t)M * K;
  const int C = K / P;
  for (uint32_t i = blockIdx.x * G_THREADS + threadIdx.x; i < total; i += gridDim.x * G_THREADS) {
    const int m = (int)fdiv(i, fd_k), j = (int)(i - (uint32_t)m * K);
    float s = 0.f;
    for (int o = 0; o < O; ++o) s += fc_g(dy, y, (size_t)m * O + o, slope) * w[(size_t)o * K + j];
    dx[(size_t)m * K + fc_xidx(j, P, C, fd_p)] = Elt<T>::from_f(s);
  }
}

// one thread per (o, j): dw[o][j] (=, +=) sum_m g[m][o] x[m][xidx(j)]; the threads with j == 0 also db[o]
template <typename T>
__global__ void __launch_bounds__(G_THREADS)
    fc_wgrad_kernel(const float* __restrict__ dy, const float* __restrict__ y, const T* __restrict__ x, int M, int K, int O,
                    int P, FastDiv fd_p, FastDiv fd_k, float slope, int accumulate, float* __restrict__ dw,
                    float* __restrict__ db) {
  const uint32_t total = (uint32_t)O * K;
  const int C = K / P;
  for (uint32_t i = blockIdx.x * G_THREADS + threadIdx.x; i < total; i += gridDim.x * G_THREADS) {
    const int o = (int)fdiv(i, fd_k), j = (int)(i - (uint32_t)o * K);
    const int xi = fc_xidx(j, P, C, fd_p);
    float s = 0.f, sb = 0.f;
    for (int m = 0; m < M; ++m) {
      const float g = fc_g(dy, y, (size_t)m * O + o, slope);
      s += g * Elt<T>::to_f(x[(size_t)m * K + xi]);
      sb += g;
    }
    dw[i] = accumulate ? dw[i] + s : s;
    if (j == 0 && db) db[o] = accumulate ? db[o] + sb : sb;
  }
}

int fc_check(const char* what, int dtype, int M, int K, int O, int P) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    return sr_fail(code, msg);
  };
  if (!dtype_ok(dtype)) return fail(SR_EINVAL, "dtype must be fp32 or bf16");
  if (M <= 0 || K <= 0 || O <= 0 || P <= 0 || K % P) return fail(SR_EINVAL, "bad arguments (K a multiple of P)");
  if (M > 65535) return fail(SR_EINVAL, "at most 65535 rows");
  if ((int64_t)M * K >= 0x40000000ll || (int64_t)O * K >= 0x40000000ll) return fail(SR_ETOOBIG, "tensor too large");
  return SR_OK;
}

}  // namespace

extern "C" {

int sr_conv4s2_prep(int dtype, const float* w, int cout_real, int cin_real, int Cout, int Cin, void* wf, void* wd,
                    void* stream) {
  if (!w || !wf || !wd || cout_real <= 0 || cin_real <= 0 || cout_real > Cout || cin_real > Cin)
    return sr_fail(SR_EINVAL, "conv4s2_prep: bad arguments");
  if (int rc = c4_check("conv4s2_prep", dtype, 1, 2, 2, Cin, Cout)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = g_grid((int64_t)2 * Cout * 16 * Cin);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(conv4s2_prep_kernel<bf16_t>, dim3(grid), dim3(G_THREADS), 0, s, w, cout_real, cin_real, Cout, Cin,
                       (bf16_t*)wf, (bf16_t*)wd);
  else
    hipLaunchKernelGGL(conv4s2_prep_kernel<float>, dim3(grid), dim3(G_THREADS), 0, s, w, cout_real, cin_real, Cout, Cin,
                       (float*)wf, (float*)wd);
  return sr_check(hipGetLastError(), "conv4s2_prep launch");
}

int sr_conv4s2_fwd_act(int dtype, const void* x, const void* wf, int N, int H, int W, int Cin, int Cout, int act,
                       float slope, void* y, void* stream) {
  if (!x || !wf || !y) return sr_fail(SR_EINVAL, "conv4s2_fwd: null pointer");
  if (int rc = c4_check("conv4s2_fwd", dtype, N, H, W, Cin, Cout)) return rc;
  if (act != 0 && act != 2) return sr_fail(SR_EINVAL, "conv4s2_fwd: act must be none (0) or LeakyReLU (2)");
  if (((uintptr_t)x | (uintptr_t)wf | (uintptr_t)y) & 15) return sr_fail(SR_EINVAL, "conv4s2_fwd: tensors must be 16-byte aligned");
  C4Args a;
  a.Hs = H, a.Ws = W, a.Cs = Cin, a.Hr = H / 2, a.Wr = W / 2, a.M = N * a.Hr * a.Wr;
  a.K = 16 * Cin, a.Nout = Cout, a.Hd = a.Hr, a.Wd = a.Wr;
  a.act = act, a.slope = slope;
  a.fd_w = make_fastdiv((uint32_t)a.Wr), a.fd_hw = make_fastdiv((uint32_t)(a.Hr * a.Wr)), a.fd_cs = make_fastdiv((uint32_t)Cin);
  if (dtype == SR_BF16) c4_launch<bf16_t, 0>(x, wf, y, a, 1, (hipStream_t)stream);
  else c4_launch<float, 0>(x, wf, y, a, 1, (hipStream_t)stream);
  return sr_check(hipGetLastError(), "conv4s2_fwd launch");
}

int sr_conv4s2_fwd(int dtype, const void* x, const void* wf, int N, int H, int W, int Cin, int Cout, void* y,
                   void* stream) {
  return sr_conv4s2_fwd_act(dtype, x, wf, N, H, W, Cin, Cout, 0, 0.f, y, stream);
}

int sr_conv4s2_dgrad(int dtype, const void* dy, const void* wd, int N, int H, int W, int Cin, int Cout, void* dx,
                     void* stream) {
  if (!dy || !wd || !dx) return sr_fail(SR_EINVAL, "conv4s2_dgrad: null pointer");
  if (int rc = c4_check("conv4s2_dgrad", dtype, N, H, W, Cin, Cout)) return rc;
  if (((uintptr_t)dy | (uintptr_t)wd | (uintptr_t)dx) & 15) return sr_fail(SR_EINVAL, "conv4s2_dgrad: tensors must be 16-byte aligned");
  C4Args a;
  a.Hs = H / 2, a.Ws = W / 2, a.Cs = Cout, a.Hr = H / 2, a.Wr = W / 2, a.M = N * a.Hr * a.Wr;
  a.K = 4 * Cout, a.Nout = Cin, a.Hd = H, a.Wd = W;
  a.act = 0, a.slope = 0.f;
  a.fd_w = make_fastdiv((uint32_t)a.Wr), a.fd_hw = make_fastdiv((uint32_t)(a.Hr * a.Wr)), a.fd_cs = make_fastdiv((uint32_t)Cout);
  if (dtype == SR_BF16) c4_launch<bf16_t, 1>(dy, wd, dx, a, 4, (hipStream_t)stream);
  else c4_launch<float, 1>(dy, wd, dx, a, 4, (hipStream_t)stream);
  return sr_check(hipGetLastError(), "conv4s2_dgrad launch");
}

size_t sr_conv4s2_wgrad_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H < 2 || W < 2 || Cin <= 0 || Cout <= 0) return 0;
  int S, kb, tco, tcol;
  c4_plan(N * (H / 2) * (W / 2), Cout, Cin, S, kb, tco, tcol);
  return (size_t)S * Cout * 16 * Cin * sizeof(float);
}

int sr_conv4s2_wgrad_splits(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H < 2 || W < 2 || Cin <= 0 || Cout <= 0) return 0;
  int S, kb, tco, tcol;
  c4_plan(N * (H / 2) * (W / 2), Cout, Cin, S, kb, tco, tcol);
  return S;
}

int sr_conv4s2_wgrad(int dtype, const void* dy, const void* x, int N, int H, int W, int Cin, int cin_real, int Cout,
                     int cout_real, float scale, int accumulate, float* dw, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !x || !dw || !ws) return sr_fail(SR_EINVAL, "conv4s2_wgrad: null pointer");
  if (int rc = c4_check("conv4s2_wgrad", dtype, N, H, W, Cin, Cout)) return rc;
  if (cin_real <= 0 || cin_real > Cin || cout_real <= 0 || cout_real > Cout)
    return sr_fail(SR_EINVAL, "conv4s2_wgrad: real channel counts out of range");
  if ((((uintptr_t)dy | (uintptr_t)x) & 15) || (((uintptr_t)dw | (uintptr_t)ws) & 3))
    return sr_fail(SR_EINVAL, "conv4s2_wgrad: dy and x must be 16-byte, dw and the workspace 4-byte aligned");
  if (ws_bytes < sr_conv4s2_wgrad_workspace(N, H, W, Cin, Cout))
    return sr_fail(SR_EINVAL, "conv4s2_wgrad: workspace smaller than sr_conv4s2_wgrad_workspace()");
  C4WArgs a;
  a.N = N, a.H = H, a.W = W, a.Cin = Cin, a.Ho = H / 2, a.Wo = W / 2, a.Cout = Cout;
  a.Mr = N * a.Ho * a.Wo, a.KW = 16 * Cin;
  int tco;
  c4_plan(a.Mr, Cout, Cin, a.S, a.kb, tco, a.tiles_col);
  a.fd_wo = make_fastdiv((uint32_t)a.Wo), a.fd_howo = make_fastdiv((uint32_t)(a.Ho * a.Wo)), a.fd_cin = make_fastdiv((uint32_t)Cin);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(tco * a.tiles_col), (unsigned)a.S);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(conv4s2_wgrad_kernel<bf16_t>, grid, dim3(G_THREADS), 0, s, (const bf16_t*)dy, (const bf16_t*)x,
                       (float*)ws, a);
  else
    hipLaunchKernelGGL(conv4s2_wgrad_kernel<float>, grid, dim3(G_THREADS), 0, s, (const float*)dy, (const float*)x,
                       (float*)ws, a);
  hipLaunchKernelGGL(conv4s2_wgrad_reduce_kernel, dim3(g_grid((int64_t)cout_real * cin_real * 16)), dim3(G_THREADS), 0, s,
                     (const float*)ws, a.S, Cout, Cin, cout_real, cin_real, scale, accumulate, dw);
  return sr_check(hipGetLastError(), "conv4s2_wgrad launch");
}

size_t sr_bn_workspace(int64_t M, int C) {
  if (M <= 0 || C <= 0) return 0;
  int B, rpb;
  bn_plan(M, B, rpb);
  return (size_t)B * 3 * C * sizeof(float);
}

int sr_bn_blocks(int64_t M) {
  if (M <= 0) return 0;
  int B, rpb;
  bn_plan(M, B, rpb);
  return B;
}

int sr_bn_stats(int dtype, const void* x, int64_t M, int C, float eps, float momentum, const int64_t* nbt, float* save_mean,
                float* save_rstd, float* running_mean, float* running_var, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !save_mean || !save_rstd || !ws) return sr_fail(SR_EINVAL, "bn_stats: null pointer");
  if (int rc = bn_check("bn_stats", dtype, M, C, 0)) return rc;
  if (M < 2) return sr_fail(SR_EINVAL, "bn_stats: more than one value per channel is needed");
  if (!running_mean != !running_var) return sr_fail(SR_EINVAL, "bn_stats: running_mean and running_var come together");
  if (running_mean && momentum < 0.f && !nbt)
    return sr_fail(SR_EINVAL, "bn_stats: the cumulative average (momentum < 0) needs num_batches_tracked");
  if (((uintptr_t)x & 15) || ((uintptr_t)ws & 3) || ((uintptr_t)nbt & 7))
    return sr_fail(SR_EINVAL, "bn_stats: x must be 16-byte aligned");
  if (ws_bytes < sr_bn_workspace(M, C)) return sr_fail(SR_EINVAL, "bn_stats: workspace smaller than sr_bn_workspace()");
  int B, rpb;
  bn_plan(M, B, rpb);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(bn_stats_kernel<bf16_t>, dim3(B), dim3(G_THREADS), 0, s, (const bf16_t*)x, (int)M, C, rpb, (float*)ws);
  else
    hipLaunchKernelGGL(bn_stats_kernel<float>, dim3(B), dim3(G_THREADS), 0, s, (const float*)x, (int)M, C, rpb, (float*)ws);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + BN_FC - 1) / BN_FC), dim3(G_THREADS), 0, s, (const float*)ws, B,
                     C, (int)M, eps, momentum, nbt, save_mean, save_rstd, running_mean, running_var);
  return sr_check(hipGetLastError(), "bn_stats launch");
}

int sr_bn_apply(int dtype, const void* x, int64_t M, int C, const float* mean, const float* rstd_or_var, int use_var,
                float eps, const float* gamma, const float* beta, int act, float slope, void* y, void* stream) {
  if (!x || !y || !mean || !rstd_or_var || !gamma || !beta) return sr_fail(SR_EINVAL, "bn_apply: null pointer");
  if (int rc = bn_check("bn_apply", dtype, M, C, act)) return rc;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return sr_fail(SR_EINVAL, "bn_apply: tensors must be 16-byte aligned");
  const int V = dtype == SR_BF16 ? 8 : 4, CV = C / V;
  const uint32_t total = (uint32_t)(M * CV);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(bn_apply_kernel<bf16_t>, dim3(g_grid(total)), dim3(G_THREADS), 0, s, (const bf16_t*)x, (bf16_t*)y,
                       total, CV, make_fastdiv((uint32_t)CV), mean, rstd_or_var, use_var, eps, gamma, beta, act, slope);
  else
    hipLaunchKernelGGL(bn_apply_kernel<float>, dim3(g_grid(total)), dim3(G_THREADS), 0, s, (const float*)x, (float*)y, total,
                       CV, make_fastdiv((uint32_t)CV), mean, rstd_or_var, use_var, eps, gamma, beta, act, slope);
  return sr_check(hipGetLastError(), "bn_apply launch");
}

int sr_bn_bwd_reduce(int dtype, const void* x, const void* dy, int64_t M, int C, const float* mean,
                     const float* rstd_or_var, int use_var, float eps, const float* gamma, const float* beta, int act,
                     float slope, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (!x || !dy || !mean || !rstd_or_var || !gamma || !beta || !dgamma || !dbeta || !ws)
    return sr_fail(SR_EINVAL, "bn_bwd_reduce: null pointer");
  if (int rc = bn_check("bn_bwd_reduce", dtype, M, C, act)) return rc;
  if ((((uintptr_t)x | (uintptr_t)dy) & 15) || ((uintptr_t)ws & 3))
    return sr_fail(SR_EINVAL, "bn_bwd_reduce: tensors must be 16-byte aligned");
  if (ws_bytes < sr_bn_workspace(M, C)) return sr_fail(SR_EINVAL, "bn_bwd_reduce: workspace smaller than sr_bn_workspace()");
  int B, rpb;
  bn_plan(M, B, rpb);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<bf16_t>, dim3(B), dim3(G_THREADS), 0, s, (const bf16_t*)x, (const bf16_t*)dy,
                       (int)M, C, rpb, mean, rstd_or_var, use_var, eps, gamma, beta, act, slope, (float*)ws);
  else
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<float>, dim3(B), dim3(G_THREADS), 0, s, (const float*)x, (const float*)dy, (int)M,
                       C, rpb, mean, rstd_or_var, use_var, eps, gamma, beta, act, slope, (float*)ws);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + BN_FC - 1) / BN_FC), dim3(G_THREADS), 0, s, (const float*)ws, B,
                     C, dgamma, dbeta);
  return sr_check(hipGetLastError(), "bn_bwd_reduce launch");
}

int sr_bn_bwd_dx(int dtype, const void* x, const void* dy, int64_t M, int C, const float* mean, const float* rstd_or_var,
                 int use_var, float eps, const float* gamma, const float* beta, int act, float slope,
                 const float* dgamma, const float* dbeta, int training, void* dx, void* stream) {
  if (!x || !dy || !dx || !mean || !rstd_or_var || !gamma || !beta || (training && (!dgamma || !dbeta)))
    return sr_fail(SR_EINVAL, "bn_bwd_dx: null pointer");
  if (int rc = bn_check("bn_bwd_dx", dtype, M, C, act)) return rc;
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 15)
    return sr_fail(SR_EINVAL, "bn_bwd_dx: tensors must be 16-byte aligned");
  const int V = dtype == SR_BF16 ? 8 : 4, CV = C / V;
  const uint32_t total = (uint32_t)(M * CV);
  const float inv_m = 1.f / (float)M;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(bn_bwd_dx_kernel<bf16_t>, dim3(g_grid(total)), dim3(G_THREADS), 0, s, (const bf16_t*)x,
                       (const bf16_t*)dy, (bf16_t*)dx, total, CV, make_fastdiv((uint32_t)CV), mean, rstd_or_var, use_var, eps,
                       gamma, beta, act, slope, dgamma, dbeta, training, inv_m);
  else
    hipLaunchKernelGGL(bn_bwd_dx_kernel<float>, dim3(g_grid(total)), dim3(G_THREADS), 0, s, (const float*)x, (const float*)dy,
                       (float*)dx, total, CV, make_fastdiv((uint32_t)CV), mean, rstd_or_var, use_var, eps, gamma, beta, act,
                       slope, dgamma, dbeta, training, inv_m);
  return sr_check(hipGetLastError(), "bn_bwd_dx launch");
}

int sr_fc_fwd(int dtype, const void* x, const float* w, const float* bias, int M, int K, int O, int P, int act, float slope,
              float* y, void* stream) {
  if (!x || !w || !y) return sr_fail(SR_EINVAL, "fc_fwd: null pointer");
  if (int rc = fc_check("fc_fwd", dtype, M, K, O, P)) return rc;
  if (act != 0 && act != 2) return sr_fail(SR_EINVAL, "fc_fwd: act must be none (0) or LeakyReLU (2)");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)O, (unsigned)M);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(fc_fwd_kernel<bf16_t>, grid, dim3(G_THREADS), 0, s, (const bf16_t*)x, w, bias, K, O, P,
                       make_fastdiv((uint32_t)P), act, slope, y);
  else
    hipLaunchKernelGGL(fc_fwd_kernel<float>, grid, dim3(G_THREADS), 0, s, (const float*)x, w, bias, K, O, P,
                       make_fastdiv((uint32_t)P), act, slope, y);
  return sr_check(hipGetLastError(), "fc_fwd launch");
}

int sr_fc_dgrad(int dtype, const float* dy, const float* y, const float* w, int M, int K, int O, int P, float slope,
                void* dx, void* stream) {
  if (!dy || !w || !dx) return sr_fail(SR_EINVAL, "fc_dgrad: null pointer");
  if (int rc = fc_check("fc_dgrad", dtype, M, K, O, P)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = g_grid((int64_t)M * K);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(fc_dgrad_kernel<bf16_t>, dim3(grid), dim3(G_THREADS), 0, s, dy, y, w, M, K, O, P,
                       make_fastdiv((uint32_t)P), make_fastdiv((uint32_t)K), slope, (bf16_t*)dx);
  else
    hipLaunchKernelGGL(fc_dgrad_kernel<float>, dim3(grid), dim3(G_THREADS), 0, s, dy, y, w, M, K, O, P,
                       make_fastdiv((uint32_t)P), make_fastdiv((uint32_t)K), slope, (float*)dx);
  return sr_check(hipGetLastError(), "fc_dgrad launch");
}

int sr_fc_wgrad(int dtype, const float* dy, const float* y, const void* x, int M, int K, int O, int P, float slope,
                int accumulate, float* dw, float* db, void* stream) {
  if (!dy || !x || !dw) return sr_fail(SR_EINVAL, "fc_wgrad: null pointer");
  if (int rc = fc_check("fc_wgrad", dtype, M, K, O, P)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = g_grid((int64_t)O * K);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(fc_wgrad_kernel<bf16_t>, dim3(grid), dim3(G_THREADS), 0, s, dy, y, (const bf16_t*)x, M, K, O, P,
                       make_fastdiv((uint32_t)P), make_fastdiv((uint32_t)K), slope, accumulate, dw, db);
  else
    hipLaunchKernelGGL(fc_wgrad_kernel<float>, dim3(grid), dim3(G_THREADS), 0, s, dy, y, (const float*)x, M, K, O, P,
                       make_fastdiv((uint32_t)P), make_fastdiv((uint32_t)K), slope, accumulate, dw, db);
  return sr_check(hipGetLastError(), "fc_wgrad launch");
}

}  // extern "C"
