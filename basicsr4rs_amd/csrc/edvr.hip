// Kernels of EDVR (basicsr/archs/edvr_arch.py) that the conv engine and the deformable convolution do not cover:
// the 3x3 stride-2 pad-1 convolution of the feature pyramids, the max + average pooling pair and the temporal
// attention of TSAFusion, and its final sigmoid modulation.
//
//   conv3s2_prep_kernel : the GEMM images of an nn.Conv2d(cin, cout, 3, 2, 1) weight.
//       wf [Cout][9 * Cin], wf[co][t * Cin + ci] = w[co][ci][kh][kw], t = kh * 3 + kw (forward);
//       wd: one image per (row, column) parity class cls = ph * 2 + pw of the input pixel, class cls with
//       nt = (1 + ph)(1 + pw) taps is [Cin][nt * Cout] at offset {0, 1, 3, 5}[cls] * Cin * Cout,
//       wd[ci][t * Cout + co] = w[co][ci][kh][kw] with t = th * (1 + pw) + tw, kh = ph ? 2 th : 1,
//       kw = pw ? 2 tw : 1 (dgrad); padded channels are zeros.
//   conv3s2_gemm_kernel : forward and dgrad, one implicit GEMM, the sibling of conv4s2_gemm_kernel (gan.hip).  A
//       block owns 64 pixels x 64 output channels and walks K in steps of 64: the pixel operand is GATHERED tap by
//       tap (16 bytes = 8 bf16 / 4 fp32 channels of one tap, zeros outside the map), the weight operand is a row
//       of the image.  MFMA: v_mfma_f32_16x16x32_bf16 / v_mfma_f32_16x16x4_f32, fp32 accumulation, 4 waves =
//       2 x 2 of 32 x 32.
//       Forward: pixel (n, oh, ow) reads x[2 oh - 1 + kh][2 ow - 1 + kw], K = 9 Cin, Ho = (H - 1) / 2 + 1; the
//       bias and an optional LeakyReLU are applied to the fp32 sums before the store.
//       Dgrad: ih = 2 oh - 1 + kh: an even input row meets only kh = 1 (from oh = ih / 2), an odd row
//       ih = 2 a + 1 meets kh = 0 (oh = a + 1) and kh = 2 (oh = a), i.e. oh = a + ph - th; the same per column.
//       Each parity class (grid z) is a GEMM with K = nt * Cout over dy, written to its own pixels of dx: 1, 2,
//       2 and 4 taps, the 9 tap products of the forward per 4 pixels, every dx element written exactly once.
//   conv3s2_wgrad_kernel + conv3s2_wgrad_reduce_kernel : dW[co][t][ci] = sum over the N Ho Wo output pixels of
//       dy[pix][co] * x[tap t of pix][ci], both operands staged transposed in LDS; split K (c3_plan) into fp32
//       partials [S][Cout][9 Cin], summed in split order into the parameter layout [cout][cin][3][3].
//   pool3s2_fwd_kernel / pool3s2_bwd_kernel : MaxPool2d(3, 2, 1) and AvgPool2d(3, 2, 1) of one map in one pass,
//       stored as the channel concat [max | avg] of a [N, Ho, Wo, 2C] map.  Max: padding never wins, the first
//       maximum in row-major window order wins, a NaN replaces whatever was there (torch).  Avg: the fp32 sum in
//       window order divided by 9 (count_include_pad).  Backward: a gather, one thread per dx vector; the choice
//       of each of the at most four windows that hold the pixel is recomputed from x.
//   tsa_corr_fwd_kernel / tsa_corr_bwd_kernel : prob = sigmoid(sum_c emb * emb_ref) per pixel and frame,
//       out[b][h][w][t * C + c] = aligned[b * T + t][h][w][c] * prob.  The G lanes of a pixel (a power of two
//       covering the C / V vectors) hold its channels; the channel sum is an xor butterfly inside them.
//   tsa_mod_fwd_kernel / tsa_mod_bwd_kernel : y = feat * sigmoid(attn) * 2 + attn_add and its gradients.
//
// No atomics, fixed summation orders: two runs give identical bits.  Nothing allocates or synchronises.
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int E_THREADS = 256;
constexpr int E_MAX_BLOCKS = 8192;
constexpr int C3_TILE = 64;
constexpr int C3_KT = 64;
constexpr int C3_KBLOCK = 256;  // output pixels per split-K block of the wgrad (times m, c3_plan)
constexpr int C3_MAX_SPLITS = 64;
constexpr int C3_BLOCK_TARGET = 2048;

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

unsigned e_grid(int64_t n) {
  int64_t g = (n + E_THREADS - 1) / E_THREADS;
  if (g > E_MAX_BLOCKS) g = E_MAX_BLOCKS;
  return (unsigned)(g < 1 ? 1 : g);
}

bool dtype_ok(int dtype) { return dtype == SR_F32 || dtype == SR_BF16; }

SR_DEV float sigmoid_f(float v) { return 1.f / (1.f + expf(-v)); }

// ---------------------------------------------------------------------------------------- conv 3x3 stride 2

// offset of a dgrad class image in units of Cin * Cout, and its tap count
__host__ __device__ inline int c3_cls_off(int cls) { return cls == 0 ? 0 : (cls == 1 ? 1 : (cls == 2 ? 3 : 5)); }
__host__ __device__ inline int c3_cls_taps(int cls) { return (1 + (cls >> 1)) * (1 + (cls & 1)); }

template <typename T>
__global__ void __launch_bounds__(E_THREADS)
    conv3s2_prep_kernel(const float* __restrict__ w, int cout_real, int cin_real, int Cout, int Cin, T* __restrict__ wf,
                        T* __restrict__ wd) {
  const uint32_t nf = (uint32_t)Cout * 9u * Cin, cc = (uint32_t)Cin * Cout;
  for (uint32_t i = blockIdx.x * E_THREADS + threadIdx.x; i < 2u * nf; i += gridDim.x * E_THREADS) {
    int co, ci, kh, kw;
    if (i < nf) {
      co = i / (9u * Cin);
      const uint32_t r = i - (uint32_t)co * 9u * Cin;
      const int t = r / Cin;
      ci = r - t * Cin, kh = t / 3, kw = t - 3 * kh;
    } else {
      const uint32_t e = i - nf;
      const int cls = e < cc ? 0 : (e < 3u * cc ? 1 : (e < 5u * cc ? 2 : 3));
      const int ph = cls >> 1, pw = cls & 1, nt = c3_cls_taps(cls);
      uint32_t r = e - (uint32_t)c3_cls_off(cls) * cc;
      ci = r / ((uint32_t)nt * Cout);
      r -= (uint32_t)ci * nt * Cout;
      const int t = r / Cout;
      co = r - t * Cout;
      const int th = t / (1 + pw), tw = t - th * (1 + pw);
      kh = ph ? 2 * th : 1, kw = pw ? 2 * tw : 1;
    }
    float v = 0.f;
    if (co < cout_real && ci < cin_real) v = w[(((size_t)co * cin_real + ci) * 3 + kh) * 3 + kw];
    if (i < nf) wf[i] = Elt<T>::from_f(v);
    else wd[i - nf] = Elt<T>::from_f(v);
  }
}

struct C3Args {
  int Hs, Ws, Cs;  // the gathered map (x forward, dy dgrad): size and channels
  int Hd, Wd;      // the written map
  int N, Nout;     // images and output channels
  int cout_real;   // forward: length of the bias
  int act;         // forward epilogue: 0 none, 2 LeakyReLU(slope)
  float slope;
  FastDiv fd_cs;
  // pixel grid of a GEMM's rows per image, per parity (forward: index 0)
  FastDiv fd_w[2], fd_hw[4];
};

// MODE 0 forward (source pixel 2 r - 1 + kh, written pixel r), MODE 1 dgrad (source pixel r + ph - th, written
// pixel 2 r + ph; grid z = parity class)
template <typename T, int MODE>
__global__ void __launch_bounds__(E_THREADS)
    conv3s2_gemm_kernel(const T* __restrict__ src, const T* __restrict__ wimg, const float* __restrict__ bias,
                        T* __restrict__ dst, C3Args a) {
  constexpr int V = Elt<T>::PER16;
  constexpr int LDT = C3_KT + V;
  constexpr int CG = C3_KT / V;
  constexpr int SL = C3_TILE * CG / E_THREADS;  // vectors a thread stages per operand and step
  __shared__ __attribute__((aligned(16))) T sP[C3_TILE * LDT];
  __shared__ __attribute__((aligned(16))) T sW[C3_TILE * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int m0 = blockIdx.x * C3_TILE, n0 = blockIdx.y * C3_TILE;
  const int cls = MODE ? (int)blockIdx.z : 0, ph = cls >> 1, pw = cls & 1;
  const int tw_n = 1 + pw;
  const int K = MODE ? c3_cls_taps(cls) * a.Cs : 9 * a.Cs;
  const T* W = wimg + (MODE ? (size_t)c3_cls_off(cls) * a.Nout * a.Cs : 0);
  // rows and columns of this GEMM's pixel grid: the forward's output map, the dgrad's pixels of parity (ph, pw)
  const int Hr = MODE ? (a.Hd - ph + 1) / 2 : a.Hd, Wr = MODE ? (a.Wd - pw + 1) / 2 : a.Wd;
  const int HrWr = Hr * Wr, M = a.N * HrWr;
  if (m0 >= M) return;
  const FastDiv fd_w = a.fd_w[pw], fd_hw = a.fd_hw[cls];

  // the rows this thread stages: their image and grid position (fixed over the K loop)
  int p_img[SL], p_r[SL], p_c[SL];
#pragma unroll
  for (int s = 0; s < SL; ++s) {
    const int rl = (tid + s * E_THREADS) / CG, m = m0 + rl;
    if (m < M) {
      const uint32_t img = fdiv((uint32_t)m, fd_hw), rem = (uint32_t)m - img * HrWr;
      const uint32_t r = fdiv(rem, fd_w);
      p_img[s] = (int)img, p_r[s] = (int)r, p_c[s] = (int)(rem - r * Wr);
    } else {
      p_img[s] = -1, p_r[s] = 0, p_c[s] = 0;
    }
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += C3_KT) {
#pragma unroll
    for (int s = 0; s < SL; ++s) {
      const int v = tid + s * E_THREADS, rl = v / CG, cg = v - rl * CG;
      const int k = k0 + cg * V;
      u32x4 q = u32x4{0u, 0u, 0u, 0u}, qw = u32x4{0u, 0u, 0u, 0u};
      if (k < K) {
        if (p_img[s] >= 0) {
          const int t = (int)fdiv((uint32_t)k, a.fd_cs), ch = k - t * a.Cs;
          int sh, sw;
          if constexpr (MODE == 0) {
            const int kh = t / 3;
            sh = 2 * p_r[s] - 1 + kh, sw = 2 * p_c[s] - 1 + (t - 3 * kh);
          } else {
            const int th = tw_n == 2 ? t >> 1 : t, tw = tw_n == 2 ? t & 1 : 0;
            sh = p_r[s] + ph - th, sw = p_c[s] + pw - tw;
          }
          if (sh >= 0 && sh < a.Hs && sw >= 0 && sw < a.Ws)
            q = *(const u32x4*)(src + (((size_t)p_img[s] * a.Hs + sh) * a.Ws + sw) * a.Cs + ch);
        }
        const int j = n0 + rl;
        if (j < a.Nout) qw = *(const u32x4*)(W + (size_t)j * K + k);
      }
      *(u32x4*)(sP + rl * LDT + cg * V) = q;
      *(u32x4*)(sW + rl * LDT + cg * V) = qw;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < C3_KT; kk += 4 * V) {
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
  if constexpr (MODE == 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int co = n0 + wr * 32 + i * 16 + fq * 4;
      float b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) b[r] = (bias && co + r < a.cout_real) ? bias[co + r] : 0.f;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float z = acc[i][j][r] + b[r];
          acc[i][j][r] = a.act == 2 ? (z > 0.f ? z : z * a.slope) : z;
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + wc * 32 + j * 16 + fr;
    if (m >= M) continue;
    const uint32_t img = fdiv((uint32_t)m, fd_hw), rem = (uint32_t)m - img * HrWr;
    const uint32_t r = fdiv(rem, fd_w), c = rem - r * Wr;
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

struct C3WArgs {
  int N, H, W, Cin, Ho, Wo, Cout;
  int Mr;  // N * Ho * Wo
  int KW;  // 9 * Cin
  int tiles_col, S, kb;
  FastDiv fd_wo, fd_howo, fd_cin;
};

// grid (tiles_co * tiles_col, S): part[sp][co][t * Cin + ci]
template <typename T>
__global__ void __launch_bounds__(E_THREADS)
    conv3s2_wgrad_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part, C3WArgs a) {
  constexpr int V = Elt<T>::PER16;
  constexpr int LDT = C3_KT + V;
  constexpr int CG = C3_TILE / V;
  constexpr int SL = C3_KT * CG / E_THREADS;
  __shared__ __attribute__((aligned(16))) T sA[C3_TILE * LDT];
  __shared__ __attribute__((aligned(16))) T sB[C3_TILE * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int tc = blockIdx.x / a.tiles_col, tl = blockIdx.x - tc * a.tiles_col, sp = blockIdx.y;
  const int co0 = tc * C3_TILE, col0 = tl * C3_TILE;
  const int k_begin = sp * a.kb, k_end = min(a.Mr, k_begin + a.kb);
  const int HoWo = a.Ho * a.Wo;
  // cg = (tid + s * 256) % CG is the same for every s (256 % CG == 0): one column vector per thread
  const int cg = tid % CG;
  const int col = col0 + cg * V, cdy = co0 + cg * V;
  const int tap = col < a.KW ? (int)fdiv((uint32_t)col, a.fd_cin) : 0, ci = col - tap * a.Cin;
  const int kh = tap / 3, kw = tap - 3 * kh;
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

  for (int k0 = k_begin; k0 < k_end; k0 += C3_KT) {
#pragma unroll
    for (int s = 0; s < SL; ++s) {
      const int kl = (tid + s * E_THREADS) / CG, k = k0 + kl;
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
    for (int kk = 0; kk < C3_KT; kk += 4 * V) {
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

// dw[co][ci][kh][kw] (=, or += with accumulate) scale * sum over s of part[s][co][(kh * 3 + kw) * Cin + ci]
__global__ void __launch_bounds__(E_THREADS)
    conv3s2_wgrad_reduce_kernel(const float* __restrict__ part, int S, int Cout, int Cin, int cout_real, int cin_real,
                                float scale, int accumulate, float* __restrict__ dw) {
  const uint32_t total = (uint32_t)cout_real * cin_real * 9u;
  const size_t KW = (size_t)9 * Cin, stride = (size_t)Cout * KW;
  for (uint32_t i = blockIdx.x * E_THREADS + threadIdx.x; i < total; i += gridDim.x * E_THREADS) {
    const uint32_t cc = i / 9u, t = i - cc * 9u;
    const uint32_t co = cc / (uint32_t)cin_real, ci = cc - co * cin_real;
    const float* p = part + (size_t)co * KW + (size_t)t * Cin + ci;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += p[(size_t)k * stride];
    s *= scale;
    dw[i] = accumulate ? dw[i] + s : s;
  }
}

void c3_plan(int Mr, int Cout, int Cin, int& S, int& kb, int& tiles_co, int& tiles_col) {
  tiles_co = (Cout + C3_TILE - 1) / C3_TILE;
  tiles_col = (9 * Cin + C3_TILE - 1) / C3_TILE;
  int smax = C3_BLOCK_TARGET / (tiles_co * tiles_col);
  smax = smax < 1 ? 1 : (smax > C3_MAX_SPLITS ? C3_MAX_SPLITS : smax);
  const int64_t blocks = ((int64_t)Mr + C3_KBLOCK - 1) / C3_KBLOCK;
  const int64_t m = (blocks + smax - 1) / smax;
  kb = (int)(C3_KBLOCK * (m < 1 ? 1 : m));
  S = (int)(((int64_t)Mr + kb - 1) / kb);
}

int c3_out(int n) { return (n - 1) / 2 + 1; }

int e_fail(const char* what, int code, const char* why) {
  static thread_local char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", what, why);
  return sr_fail(code, msg);
}

int c3_check(const char* what, int dtype, int N, int H, int W, int Cin, int Cout) {
  if (!dtype_ok(dtype)) return e_fail(what, SR_EINVAL, "dtype must be fp32 or bf16");
  if (N <= 0 || H < 2 || W < 2) return e_fail(what, SR_EINVAL, "N must be positive, H and W at least 2");
  if (Cin < 8 || Cout < 8 || Cin > 512 || Cout > 512 || Cin % 8 || Cout % 8)
    return e_fail(what, SR_EINVAL, "channels must be multiples of 8 from 8 to 512");
  const int64_t esz = dtype == SR_BF16 ? 2 : 4;
  if ((int64_t)N * H * W * Cin * esz >= 0x80000000ll || (int64_t)N * c3_out(H) * c3_out(W) * Cout * esz >= 0x80000000ll)
    return e_fail(what, SR_ETOOBIG, "tensor too large");
  return SR_OK;
}

template <typename T, int MODE>
void c3_launch(const void* src, const void* wimg, const float* bias, void* dst, const C3Args& a, int M, int classes,
               hipStream_t s) {
  const dim3 grid((unsigned)((M + C3_TILE - 1) / C3_TILE), (unsigned)((a.Nout + C3_TILE - 1) / C3_TILE), (unsigned)classes);
  hipLaunchKernelGGL((conv3s2_gemm_kernel<T, MODE>), grid, dim3(E_THREADS), 0, s, (const T*)src, (const T*)wimg, bias,
                     (T*)dst, a);
}

// ------------------------------------------------------------------------------------- pooling 3x3 stride 2

// torch's max-pool update: the first maximum wins, a NaN replaces whatever was there
SR_DEV bool mp_takes(float v, float m) { return v > m || v != v; }

struct P3Args {
  int H, W, C, Ho, Wo, CV;
  uint32_t total;  // vectors of the kernel's index space
  FastDiv fd_cv, fd_w, fd_h;
};

// one thread per (n, oh, ow, cv): the max to y[..., cv], the average to y[..., C + cv]
template <typename T>
__global__ void __launch_bounds__(E_THREADS) pool3s2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, P3Args a) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * E_THREADS + threadIdx.x; i < a.total; i += gridDim.x * E_THREADS) {
    const uint32_t pix = fdiv(i, a.fd_cv), cv = i - pix * a.CV;
    const uint32_t row = fdiv(pix, a.fd_w), ow = pix - row * a.Wo;
    const uint32_t n = fdiv(row, a.fd_h), oh = row - n * a.Ho;
    const T* base = x + (size_t)n * a.H * a.W * a.C + cv * V;
    float m[V], s[V];
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = -INFINITY, s[k] = 0.f;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const int ih = 2 * (int)oh - 1 + q / 3, iw = 2 * (int)ow - 1 + q % 3;
      if (ih < 0 || ih >= a.H || iw < 0 || iw >= a.W) continue;
      float v[V];
      ld16<T, V>(base + ((size_t)ih * a.W + iw) * a.C, v);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if (mp_takes(v[k], m[k])) m[k] = v[k];
        s[k] += v[k];
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) s[k] = __fdiv_rn(s[k], 9.f);
    T* o = y + (size_t)pix * 2 * a.C + cv * V;
    st16<T, V>(o, m);
    st16<T, V>(o + a.C, s);
  }
}

// one thread per dx vector (n, h, w, cv): the windows oh in {h / 2, (h + 1) / 2} x ow in {w / 2, (w + 1) / 2} inside
// the output map, in ascending (oh, ow) order
template <typename T>
__global__ void __launch_bounds__(E_THREADS)
    pool3s2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, P3Args a) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * E_THREADS + threadIdx.x; i < a.total; i += gridDim.x * E_THREADS) {
    const uint32_t pix = fdiv(i, a.fd_cv), cv = i - pix * a.CV;
    const uint32_t row = fdiv(pix, a.fd_w), w = pix - row * a.W;
    const uint32_t n = fdiv(row, a.fd_h), h = row - n * a.H;
    const int oh0 = (int)h / 2, oh1 = min(((int)h + 1) / 2, a.Ho - 1);
    const int ow0 = (int)w / 2, ow1 = min(((int)w + 1) / 2, a.Wo - 1);
    const T* base = x + (size_t)n * a.H * a.W * a.C + cv * V;
    float gm[V], ga[V];
#pragma unroll
    for (int k = 0; k < V; ++k) gm[k] = 0.f, ga[k] = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh)
      for (int ow = ow0; ow <= ow1; ++ow) {
        const int mine = ((int)h - (2 * oh - 1)) * 3 + ((int)w - (2 * ow - 1));
        float m[V];
        int idx[V];
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = -INFINITY, idx[k] = -1;
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          const int ih = 2 * oh - 1 + q / 3, iw = 2 * ow - 1 + q % 3;
          if (ih < 0 || ih >= a.H || iw < 0 || iw >= a.W) continue;
          float v[V];
          ld16<T, V>(base + ((size_t)ih * a.W + iw) * a.C, v);
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (mp_takes(v[k], m[k])) m[k] = v[k], idx[k] = q;
        }
        const T* g = dy + (((size_t)n * a.Ho + oh) * a.Wo + ow) * 2 * a.C + cv * V;
        float g_max[V], g_avg[V];
        ld16<T, V>(g, g_max);
        ld16<T, V>(g + a.C, g_avg);
#pragma unroll
        for (int k = 0; k < V; ++k) {
          if (idx[k] == mine) gm[k] += g_max[k];
          ga[k] += g_avg[k];
        }
      }
#pragma unroll
    for (int k = 0; k < V; ++k) gm[k] += __fdiv_rn(ga[k], 9.f);
    st16<T, V>(dx + (size_t)i * V, gm);
  }
}

int p3_check(const char* what, int dtype, const void* p0, const void* p1, const void* p2, int N, int H, int W, int C,
             P3Args& a, bool bwd) {
  if (!p0 || !p1 || !p2) return e_fail(what, SR_EINVAL, "null pointer");
  if (!dtype_ok(dtype)) return e_fail(what, SR_EINVAL, "dtype must be fp32 or bf16");
  if (N <= 0 || H <= 0 || W <= 0 || C < 8 || C % 8) return e_fail(what, SR_EINVAL, "bad arguments (C a multiple of 8)");
  if (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) return e_fail(what, SR_EINVAL, "tensors must be 16-byte aligned");
  const int64_t esz = dtype == SR_BF16 ? 2 : 4;
  if ((int64_t)N * H * W * C * esz >= 0x80000000ll) return e_fail(what, SR_ETOOBIG, "tensor too large");
  const int V = dtype == SR_BF16 ? 8 : 4;
  a.H = H, a.W = W, a.C = C, a.Ho = c3_out(H), a.Wo = c3_out(W), a.CV = C / V;
  a.fd_cv = make_fastdiv((uint32_t)a.CV);
  if (bwd) {
    a.total = (uint32_t)((int64_t)N * H * W * a.CV);
    a.fd_w = make_fastdiv((uint32_t)W), a.fd_h = make_fastdiv((uint32_t)H);
  } else {
    a.total = (uint32_t)((int64_t)N * a.Ho * a.Wo * a.CV);
    a.fd_w = make_fastdiv((uint32_t)a.Wo), a.fd_h = make_fastdiv((uint32_t)a.Ho);
  }
  return SR_OK;
}

// ----------------------------------------------------------------------------------------- temporal attention

constexpr int TSA_NV = 2;  // vectors of a pixel a lane holds at most (C / V <= 128)

struct TsaArgs {
  int B, T, HW, C, CV;
  int G, gshift;   // lanes per pixel (a power of two <= 64) and its log2
  uint32_t npix;   // B * HW
  FastDiv fd_hw;
};

// butterfly sum over the G lanes of a pixel: every lane ends with the same bits
SR_DEV float group_sum(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T>
__global__ void __launch_bounds__(E_THREADS)
    tsa_corr_fwd_kernel(const T* __restrict__ emb, const T* __restrict__ ref, const T* __restrict__ aligned,
                        T* __restrict__ out, float* __restrict__ prob, TsaArgs a) {
  constexpr int V = Elt<T>::PER16;
  const uint32_t gid = (blockIdx.x * E_THREADS + threadIdx.x) >> a.gshift, j0 = threadIdx.x & (a.G - 1);
  const uint32_t ngroups = (gridDim.x * E_THREADS) >> a.gshift;
  // whole groups iterate together: the shuffles of a group see all of its lanes
  for (uint32_t p = gid; p < a.npix; p += ngroups) {
    const uint32_t b = fdiv(p, a.fd_hw), hw = p - b * a.HW;
    const T* rp = ref + (size_t)p * a.C;
    for (int t = 0; t < a.T; ++t) {
      const size_t fp = ((size_t)(b * a.T + t) * a.HW + hw) * a.C;
      float s = 0.f;
#pragma unroll
      for (int n = 0; n < TSA_NV; ++n) {
        const int j = (int)j0 + n * a.G;
        if (j < a.CV) {
          float e[V], r[V];
          ld16<T, V>(emb + fp + j * V, e);
          ld16<T, V>(rp + j * V, r);
#pragma unroll
          for (int k = 0; k < V; ++k) s = fmaf(e[k], r[k], s);
        }
      }
      s = group_sum(s, a.G);
      const float pr = sigmoid_f(s);
      if (j0 == 0) prob[((size_t)b * a.T + t) * a.HW + hw] = pr;
      T* op = out + ((size_t)p * a.T + t) * a.C;
#pragma unroll
      for (int n = 0; n < TSA_NV; ++n) {
        const int j = (int)j0 + n * a.G;
        if (j < a.CV) {
          float v[V];
          ld16<T, V>(aligned + fp + j * V, v);
#pragma unroll
          for (int k = 0; k < V; ++k) v[k] *= pr;
          st16<T, V>(op + j * V, v);
        }
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(E_THREADS)
    tsa_corr_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ emb, const T* __restrict__ ref,
                        const T* __restrict__ aligned, const float* __restrict__ prob, T* __restrict__ d_aligned,
                        T* __restrict__ d_emb, T* __restrict__ d_ref, TsaArgs a) {
  constexpr int V = Elt<T>::PER16;
  const uint32_t gid = (blockIdx.x * E_THREADS + threadIdx.x) >> a.gshift, j0 = threadIdx.x & (a.G - 1);
  const uint32_t ngroups = (gridDim.x * E_THREADS) >> a.gshift;
  for (uint32_t p = gid; p < a.npix; p += ngroups) {
    const uint32_t b = fdiv(p, a.fd_hw), hw = p - b * a.HW;
    const T* rp = ref + (size_t)p * a.C;
    float r[TSA_NV][V], dr[TSA_NV][V];
#pragma unroll
    for (int n = 0; n < TSA_NV; ++n) {
      const int j = (int)j0 + n * a.G;
#pragma unroll
      for (int k = 0; k < V; ++k) r[n][k] = 0.f, dr[n][k] = 0.f;
      if (j < a.CV) ld16<T, V>(rp + j * V, r[n]);
    }
    for (int t = 0; t < a.T; ++t) {
      const size_t fp = ((size_t)(b * a.T + t) * a.HW + hw) * a.C;
      const T* gp = dout + ((size_t)p * a.T + t) * a.C;
      const float pr = prob[((size_t)b * a.T + t) * a.HW + hw];
      float g[TSA_NV][V], s = 0.f;
#pragma unroll
      for (int n = 0; n < TSA_NV; ++n) {
        const int j = (int)j0 + n * a.G;
        if (j < a.CV) {
          float al[V];
          ld16<T, V>(gp + j * V, g[n]);
          ld16<T, V>(aligned + fp + j * V, al);
#pragma unroll
          for (int k = 0; k < V; ++k) s = fmaf(g[n][k], al[k], s);
        }
      }
      s = group_sum(s, a.G);
      const float dc = s * pr * (1.f - pr);
#pragma unroll
      for (int n = 0; n < TSA_NV; ++n) {
        const int j = (int)j0 + n * a.G;
        if (j < a.CV) {
          float e[V], da[V], de[V];
          ld16<T, V>(emb + fp + j * V, e);
#pragma unroll
          for (int k = 0; k < V; ++k) {
            da[k] = g[n][k] * pr;
            de[k] = dc * r[n][k];
            dr[n][k] = fmaf(dc, e[k], dr[n][k]);
          }
          st16<T, V>(d_aligned + fp + j * V, da);
          st16<T, V>(d_emb + fp + j * V, de);
        }
      }
    }
#pragma unroll
    for (int n = 0; n < TSA_NV; ++n) {
      const int j = (int)j0 + n * a.G;
      if (j < a.CV) st16<T, V>(d_ref + (size_t)p * a.C + j * V, dr[n]);
    }
  }
}

int tsa_check(const char* what, int dtype, int B, int T, int H, int W, int C, TsaArgs& a) {
  if (!dtype_ok(dtype)) return e_fail(what, SR_EINVAL, "dtype must be fp32 or bf16");
  if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || C < 8 || C % 8 || C > 512)
    return e_fail(what, SR_EINVAL, "bad arguments (C a multiple of 8 up to 512)");
  const int64_t esz = dtype == SR_BF16 ? 2 : 4;
  if ((int64_t)B * T * H * W * C * esz >= 0x80000000ll) return e_fail(what, SR_ETOOBIG, "tensor too large");
  const int V = dtype == SR_BF16 ? 8 : 4;
  a.B = B, a.T = T, a.HW = H * W, a.C = C, a.CV = C / V;
  a.G = 1, a.gshift = 0;
  while (a.G < a.CV && a.G < 64) a.G <<= 1, ++a.gshift;
  a.npix = (uint32_t)((int64_t)B * H * W);
  a.fd_hw = make_fastdiv((uint32_t)a.HW);
  return SR_OK;
}

// ------------------------------------------------------------------------------------------ sigmoid modulation

template <typename T>
__global__ void __launch_bounds__(E_THREADS)
    tsa_mod_fwd_kernel(const T* __restrict__ feat, const T* __restrict__ attn, const T* __restrict__ add,
                       T* __restrict__ y, uint32_t total) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * E_THREADS + threadIdx.x; i < total; i += gridDim.x * E_THREADS) {
    float f[V], s[V], d[V];
    ld16<T, V>(feat + (size_t)i * V, f);
    ld16<T, V>(attn + (size_t)i * V, s);
    ld16<T, V>(add + (size_t)i * V, d);
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] = fmaf(f[k] * sigmoid_f(s[k]), 2.f, d[k]);
    st16<T, V>(y + (size_t)i * V, f);
  }
}

template <typename T>
__global__ void __launch_bounds__(E_THREADS)
    tsa_mod_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ feat, const T* __restrict__ attn,
                       T* __restrict__ d_feat, T* __restrict__ d_attn, uint32_t total) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * E_THREADS + threadIdx.x; i < total; i += gridDim.x * E_THREADS) {
    float g[V], f[V], s[V];
    ld16<T, V>(dy + (size_t)i * V, g);
    ld16<T, V>(feat + (size_t)i * V, f);
    ld16<T, V>(attn + (size_t)i * V, s);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float sg = sigmoid_f(s[k]), g2 = g[k] * 2.f;
      s[k] = g2 * f[k] * (sg * (1.f - sg));
      f[k] = g2 * sg;
    }
    st16<T, V>(d_feat + (size_t)i * V, f);
    st16<T, V>(d_attn + (size_t)i * V, s);
  }
}

int mod_check(const char* what, int dtype, int64_t n, uintptr_t ptrs) {
  if (!dtype_ok(dtype)) return e_fail(what, SR_EINVAL, "dtype must be fp32 or bf16");
  if (n <= 0 || n % 8) return e_fail(what, SR_EINVAL, "bad arguments (n a positive multiple of 8)");
  if (ptrs & 15) return e_fail(what, SR_EINVAL, "tensors must be 16-byte aligned");
  if (n * (dtype == SR_BF16 ? 2 : 4) >= 0x80000000ll) return e_fail(what, SR_ETOOBIG, "tensor too large");
  return SR_OK;
}

}  // namespace

extern "C" {

int sr_conv3s2_prep(int dtype, const float* w, int cout_real, int cin_real, int Cout, int Cin, void* wf, void* wd,
                    void* stream) {
  if (!w || !wf || !wd || cout_real <= 0 || cin_real <= 0 || cout_real > Cout || cin_real > Cin)
    return sr_fail(SR_EINVAL, "conv3s2_prep: bad arguments");
  if (int rc = c3_check("conv3s2_prep", dtype, 1, 2, 2, Cin, Cout)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = e_grid((int64_t)2 * Cout * 9 * Cin);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(conv3s2_prep_kernel<bf16_t>, dim3(grid), dim3(E_THREADS), 0, s, w, cout_real, cin_real, Cout, Cin,
                       (bf16_t*)wf, (bf16_t*)wd);
  else
    hipLaunchKernelGGL(conv3s2_prep_kernel<float>, dim3(grid), dim3(E_THREADS), 0, s, w, cout_real, cin_real, Cout, Cin,
                       (float*)wf, (float*)wd);
  return sr_check(hipGetLastError(), "conv3s2_prep launch");
}

int sr_conv3s2_fwd(int dtype, const void* x, const void* wf, const float* bias, int N, int H, int W, int Cin, int Cout,
                   int cout_real, int act, float slope, void* y, void* stream) {
  if (!x || !wf || !y) return sr_fail(SR_EINVAL, "conv3s2_fwd: null pointer");
  if (int rc = c3_check("conv3s2_fwd", dtype, N, H, W, Cin, Cout)) return rc;
  if (act != 0 && act != 2) return sr_fail(SR_EINVAL, "conv3s2_fwd: act must be none (0) or LeakyReLU (2)");
  if (cout_real <= 0 || cout_real > Cout) return sr_fail(SR_EINVAL, "conv3s2_fwd: real channel count out of range");
  if ((((uintptr_t)x | (uintptr_t)wf | (uintptr_t)y) & 15) || ((uintptr_t)bias & 3))
    return sr_fail(SR_EINVAL, "conv3s2_fwd: tensors must be 16-byte aligned");
  C3Args a = {};
  a.Hs = H, a.Ws = W, a.Cs = Cin, a.Hd = c3_out(H), a.Wd = c3_out(W), a.N = N, a.Nout = Cout;
  a.cout_real = cout_real, a.act = act, a.slope = slope;
  a.fd_cs = make_fastdiv((uint32_t)Cin);
  a.fd_w[0] = make_fastdiv((uint32_t)a.Wd), a.fd_hw[0] = make_fastdiv((uint32_t)(a.Hd * a.Wd));
  const int M = N * a.Hd * a.Wd;
  if (dtype == SR_BF16) c3_launch<bf16_t, 0>(x, wf, bias, y, a, M, 1, (hipStream_t)stream);
  else c3_launch<float, 0>(x, wf, bias, y, a, M, 1, (hipStream_t)stream);
  return sr_check(hipGetLastError(), "conv3s2_fwd launch");
}

int sr_conv3s2_dgrad(int dtype, const void* dy, const void* wd, int N, int H, int W, int Cin, int Cout, void* dx,
                     void* stream) {
  if (!dy || !wd || !dx) return sr_fail(SR_EINVAL, "conv3s2_dgrad: null pointer");
  if (int rc = c3_check("conv3s2_dgrad", dtype, N, H, W, Cin, Cout)) return rc;
  if (((uintptr_t)dy | (uintptr_t)wd | (uintptr_t)dx) & 15) return sr_fail(SR_EINVAL, "conv3s2_dgrad: tensors must be 16-byte aligned");
  C3Args a = {};
  a.Hs = c3_out(H), a.Ws = c3_out(W), a.Cs = Cout, a.Hd = H, a.Wd = W, a.N = N, a.Nout = Cin;
  a.cout_real = 0, a.act = 0, a.slope = 0.f;
  a.fd_cs = make_fastdiv((uint32_t)Cout);
  for (int pw = 0; pw < 2; ++pw) a.fd_w[pw] = make_fastdiv((uint32_t)((W - pw + 1) / 2));
  for (int cls = 0; cls < 4; ++cls)
    a.fd_hw[cls] = make_fastdiv((uint32_t)(((H - (cls >> 1) + 1) / 2) * ((W - (cls & 1) + 1) / 2)));
  // the grid covers the largest class (even rows, even columns); blocks past a smaller class's pixels return
  const int M = N * ((H + 1) / 2) * ((W + 1) / 2);
  if (dtype == SR_BF16) c3_launch<bf16_t, 1>(dy, wd, nullptr, dx, a, M, 4, (hipStream_t)stream);
  else c3_launch<float, 1>(dy, wd, nullptr, dx, a, M, 4, (hipStream_t)stream);
  return sr_check(hipGetLastError(), "conv3s2_dgrad launch");
}

size_t sr_conv3s2_wgrad_workspace(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H < 2 || W < 2 || Cin <= 0 || Cout <= 0) return 0;
  int S, kb, tco, tcol;
  c3_plan(N * c3_out(H) * c3_out(W), Cout, Cin, S, kb, tco, tcol);
  return (size_t)S * Cout * 9 * Cin * sizeof(float);
}

int sr_conv3s2_wgrad_splits(int N, int H, int W, int Cin, int Cout) {
  if (N <= 0 || H < 2 || W < 2 || Cin <= 0 || Cout <= 0) return 0;
  int S, kb, tco, tcol;
  c3_plan(N * c3_out(H) * c3_out(W), Cout, Cin, S, kb, tco, tcol);
  return S;
}

int sr_conv3s2_wgrad(int dtype, const void* dy, const void* x, int N, int H, int W, int Cin, int cin_real, int Cout,
                     int cout_real, float scale, int accumulate, float* dw, void* ws, size_t ws_bytes, void* stream) {
  if (!dy || !x || !dw || !ws) return sr_fail(SR_EINVAL, "conv3s2_wgrad: null pointer");
  if (int rc = c3_check("conv3s2_wgrad", dtype, N, H, W, Cin, Cout)) return rc;
  if (cin_real <= 0 || cin_real > Cin || cout_real <= 0 || cout_real > Cout)
    return sr_fail(SR_EINVAL, "conv3s2_wgrad: real channel counts out of range");
  if ((((uintptr_t)dy | (uintptr_t)x) & 15) || (((uintptr_t)dw | (uintptr_t)ws) & 3))
    return sr_fail(SR_EINVAL, "conv3s2_wgrad: dy and x must be 16-byte, dw and the workspace 4-byte aligned");
  if (ws_bytes < sr_conv3s2_wgrad_workspace(N, H, W, Cin, Cout))
    return sr_fail(SR_EINVAL, "conv3s2_wgrad: workspace smaller than sr_conv3s2_wgrad_workspace()");
  C3WArgs a;
  a.N = N, a.H = H, a.W = W, a.Cin = Cin, a.Ho = c3_out(H), a.Wo = c3_out(W), a.Cout = Cout;
  a.Mr = N * a.Ho * a.Wo, a.KW = 9 * Cin;
  int tco;
  c3_plan(a.Mr, Cout, Cin, a.S, a.kb, tco, a.tiles_col);
  a.fd_wo = make_fastdiv((uint32_t)a.Wo), a.fd_howo = make_fastdiv((uint32_t)(a.Ho * a.Wo)), a.fd_cin = make_fastdiv((uint32_t)Cin);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(tco * a.tiles_col), (unsigned)a.S);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(conv3s2_wgrad_kernel<bf16_t>, grid, dim3(E_THREADS), 0, s, (const bf16_t*)dy, (const bf16_t*)x,
                       (float*)ws, a);
  else
    hipLaunchKernelGGL(conv3s2_wgrad_kernel<float>, grid, dim3(E_THREADS), 0, s, (const float*)dy, (const float*)x,
                       (float*)ws, a);
  hipLaunchKernelGGL(conv3s2_wgrad_reduce_kernel, dim3(e_grid((int64_t)cout_real * cin_real * 9)), dim3(E_THREADS), 0, s,
                     (const float*)ws, a.S, Cout, Cin, cout_real, cin_real, scale, accumulate, dw);
  return sr_check(hipGetLastError(), "conv3s2_wgrad launch");
}

int sr_pool3s2_fwd(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream) {
  P3Args a;
  if (int rc = p3_check("pool3s2_fwd", dtype, x, y, y, N, H, W, C, a, false)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(pool3s2_fwd_kernel<bf16_t>, dim3(e_grid(a.total)), dim3(E_THREADS), 0, s, (const bf16_t*)x,
                       (bf16_t*)y, a);
  else
    hipLaunchKernelGGL(pool3s2_fwd_kernel<float>, dim3(e_grid(a.total)), dim3(E_THREADS), 0, s, (const float*)x, (float*)y,
                       a);
  return sr_check(hipGetLastError(), "pool3s2_fwd launch");
}

int sr_pool3s2_bwd(int dtype, const void* x, const void* dy, int N, int H, int W, int C, void* dx, void* stream) {
  P3Args a;
  if (int rc = p3_check("pool3s2_bwd", dtype, x, dy, dx, N, H, W, C, a, true)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(pool3s2_bwd_kernel<bf16_t>, dim3(e_grid(a.total)), dim3(E_THREADS), 0, s, (const bf16_t*)x,
                       (const bf16_t*)dy, (bf16_t*)dx, a);
  else
    hipLaunchKernelGGL(pool3s2_bwd_kernel<float>, dim3(e_grid(a.total)), dim3(E_THREADS), 0, s, (const float*)x,
                       (const float*)dy, (float*)dx, a);
  return sr_check(hipGetLastError(), "pool3s2_bwd launch");
}

int sr_tsa_corr_fwd(int dtype, const void* emb, const void* emb_ref, const void* aligned, int B, int T, int H, int W,
                    int C, void* out, float* prob, void* stream) {
  if (!emb || !emb_ref || !aligned || !out || !prob) return sr_fail(SR_EINVAL, "tsa_corr_fwd: null pointer");
  TsaArgs a;
  if (int rc = tsa_check("tsa_corr_fwd", dtype, B, T, H, W, C, a)) return rc;
  if ((((uintptr_t)emb | (uintptr_t)emb_ref | (uintptr_t)aligned | (uintptr_t)out) & 15) || ((uintptr_t)prob & 3))
    return sr_fail(SR_EINVAL, "tsa_corr_fwd: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = e_grid((int64_t)a.npix * a.G);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(tsa_corr_fwd_kernel<bf16_t>, dim3(grid), dim3(E_THREADS), 0, s, (const bf16_t*)emb,
                       (const bf16_t*)emb_ref, (const bf16_t*)aligned, (bf16_t*)out, prob, a);
  else
    hipLaunchKernelGGL(tsa_corr_fwd_kernel<float>, dim3(grid), dim3(E_THREADS), 0, s, (const float*)emb,
                       (const float*)emb_ref, (const float*)aligned, (float*)out, prob, a);
  return sr_check(hipGetLastError(), "tsa_corr_fwd launch");
}

int sr_tsa_corr_bwd(int dtype, const void* d_out, const void* emb, const void* emb_ref, const void* aligned,
                    const float* prob, int B, int T, int H, int W, int C, void* d_aligned, void* d_emb, void* d_emb_ref,
                    void* stream) {
  if (!d_out || !emb || !emb_ref || !aligned || !prob || !d_aligned || !d_emb || !d_emb_ref)
    return sr_fail(SR_EINVAL, "tsa_corr_bwd: null pointer");
  TsaArgs a;
  if (int rc = tsa_check("tsa_corr_bwd", dtype, B, T, H, W, C, a)) return rc;
  if ((((uintptr_t)d_out | (uintptr_t)emb | (uintptr_t)emb_ref | (uintptr_t)aligned | (uintptr_t)d_aligned |
        (uintptr_t)d_emb | (uintptr_t)d_emb_ref) & 15) || ((uintptr_t)prob & 3))
    return sr_fail(SR_EINVAL, "tsa_corr_bwd: tensors must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = e_grid((int64_t)a.npix * a.G);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(tsa_corr_bwd_kernel<bf16_t>, dim3(grid), dim3(E_THREADS), 0, s, (const bf16_t*)d_out,
                       (const bf16_t*)emb, (const bf16_t*)emb_ref, (const bf16_t*)aligned, prob, (bf16_t*)d_aligned,
                       (bf16_t*)d_emb, (bf16_t*)d_emb_ref, a);
  else
    hipLaunchKernelGGL(tsa_corr_bwd_kernel<float>, dim3(grid), dim3(E_THREADS), 0, s, (const float*)d_out,
                       (const float*)emb, (const float*)emb_ref, (const float*)aligned, prob, (float*)d_aligned,
                       (float*)d_emb, (float*)d_emb_ref, a);
  return sr_check(hipGetLastError(), "tsa_corr_bwd launch");
}

int sr_tsa_modulate_fwd(int dtype, const void* feat, const void* attn, const void* attn_add, int64_t n, void* y,
                        void* stream) {
  if (!feat || !attn || !attn_add || !y) return sr_fail(SR_EINVAL, "tsa_modulate_fwd: null pointer");
  if (int rc = mod_check("tsa_modulate_fwd", dtype, n, (uintptr_t)feat | (uintptr_t)attn | (uintptr_t)attn_add | (uintptr_t)y))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(tsa_mod_fwd_kernel<bf16_t>, dim3(e_grid(n / 8)), dim3(E_THREADS), 0, s, (const bf16_t*)feat,
                       (const bf16_t*)attn, (const bf16_t*)attn_add, (bf16_t*)y, (uint32_t)(n / 8));
  else
    hipLaunchKernelGGL(tsa_mod_fwd_kernel<float>, dim3(e_grid(n / 4)), dim3(E_THREADS), 0, s, (const float*)feat,
                       (const float*)attn, (const float*)attn_add, (float*)y, (uint32_t)(n / 4));
  return sr_check(hipGetLastError(), "tsa_modulate_fwd launch");
}

int sr_tsa_modulate_bwd(int dtype, const void* dy, const void* feat, const void* attn, int64_t n, void* d_feat,
                        void* d_attn, void* stream) {
  if (!dy || !feat || !attn || !d_feat || !d_attn) return sr_fail(SR_EINVAL, "tsa_modulate_bwd: null pointer");
  if (int rc = mod_check("tsa_modulate_bwd", dtype, n,
                         (uintptr_t)dy | (uintptr_t)feat | (uintptr_t)attn | (uintptr_t)d_feat | (uintptr_t)d_attn))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(tsa_mod_bwd_kernel<bf16_t>, dim3(e_grid(n / 8)), dim3(E_THREADS), 0, s, (const bf16_t*)dy,
                       (const bf16_t*)feat, (const bf16_t*)attn, (bf16_t*)d_feat, (bf16_t*)d_attn, (uint32_t)(n / 8));
  else
    hipLaunchKernelGGL(tsa_mod_bwd_kernel<float>, dim3(e_grid(n / 4)), dim3(E_THREADS), 0, s, (const float*)dy,
                       (const float*)feat, (const float*)attn, (float*)d_feat, (float*)d_attn, (uint32_t)(n / 4));
  return sr_check(hipGetLastError(), "tsa_modulate_bwd launch");
}

}  // extern "C"
