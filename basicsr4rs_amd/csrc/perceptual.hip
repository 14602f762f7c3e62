// Kernels of the perceptual / style loss (basicsr/losses/basic_loss.py:147-253 over the VGG feature
// extractor of basicsr/archs/vgg_arch.py) that the conv engine does not already cover:
//
//   maxpool2_fwd_kernel / maxpool2_bwd_kernel : nn.MaxPool2d(2, stride 1 or 2), NHWC, 16-byte vectors over the
//       channels.  Forward: the first maximum in row-major window order wins and a NaN propagates (torch's
//       `val > max || isnan(val)` update).  Backward: one thread per dx vector GATHERS from the (one, or with
//       stride 1 up to four) windows that contain its pixel, recomputing each window's choice from x with the
//       forward's rule -- every dx element is written exactly once (zeros for a row / column the floor
//       drops), overlapping windows are summed in fp32 in a fixed order, nothing is stored by the forward.
//   gram_fwd_kernel (+ gram_reduce_kernel) : G[n] = F[n]^T F[n] * scale, F NHWC [N, HW, C], G fp32 [N, C, C].
//       A block owns a 64 x 64 tile of G over a range of K = HW rows: it stages 64 rows x 64 channels of F
//       TRANSPOSED in LDS ([channel][k], so an MFMA operand fragment is 16 contiguous bytes), once for the
//       tile's row channels and once for its column channels, and multiplies them with
//       v_mfma_f32_16x16x32_bf16 (bf16) / v_mfma_f32_16x16x4_f32 (fp32); 4 waves = 2 x 2 of 32 x 32.
//       Split-K rule (gram_plan): a block covers kb = GRAM_KBLOCK * m rows, m the smallest integer with
//       ceil(HW / kb) <= GRAM_MAX_SPLITS.  One K block: G is written directly; more: fp32 partials
//       [N][S][C][C] in the caller's workspace, summed in a fixed order by gram_reduce_kernel.
//   gram_bwd_kernel : dF[n] = alpha * F[n] (dG[n] + dG[n]^T) + beta * res, an [HW x C] . [C x C] GEMM per image.
//       dG is fp32 and the result is held to an fp32 bound, so both dtypes multiply on the f32 MFMA (bf16
//       features are widened exactly while staging); the symmetrised dG tile is built while staging
//       (Sym[c][j] = dG[c][j] + dG[j][c], read as the B operand through Sym[j][c] = Sym[c][j]).
//
// No atomics, fixed summation orders: two runs give identical bits.  Nothing allocates or synchronises.
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_MAX_BLOCKS = 8192;

constexpr int GR_TILE = 64;            // channels per side of an output tile
constexpr int GR_KT = 64;              // k rows staged per step
constexpr int GRAM_KBLOCK = 1024;      // k rows per block of the split-K plan (times m, gram_plan)
constexpr int GRAM_MAX_SPLITS = 64;    // K blocks per image at most
constexpr int GB_LD = GR_TILE + 4;     // fp32 row stride of the backward's LDS tiles (16-byte multiple)
constexpr int GB_MIN_BLOCKS = 512;     // the backward at C <= 64 gives a block 2 .. 8 row tiles above this many tiles

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

// torch's max-pool update: the first maximum wins, a NaN replaces whatever was there
SR_DEV bool mp_takes(float v, float m) { return v > m || v != v; }

struct PoolArgs {
  int H, W, C, Ho, Wo, s, CV;
  uint32_t total;  // vectors of the kernel's index space
  FastDiv fd_cv, fd_w, fd_h;
};

// one thread per output vector (n, oh, ow, cv)
template <typename T>
__global__ void __launch_bounds__(PC_THREADS) maxpool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, PoolArgs a) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * PC_THREADS + threadIdx.x; i < a.total; i += gridDim.x * PC_THREADS) {
    const uint32_t pix = fdiv(i, a.fd_cv), cv = i - pix * a.CV;
    const uint32_t row = fdiv(pix, a.fd_w), ow = pix - row * a.Wo;
    const uint32_t n = fdiv(row, a.fd_h), oh = row - n * a.Ho;
    const T* p = x + (((size_t)n * a.H + oh * a.s) * a.W + ow * a.s) * a.C + cv * V;
    float m[V];
#pragma unroll
    for (int k = 0; k < V; ++k) m[k] = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v[V];
      ld16<T, V>(p + ((size_t)(q >> 1) * a.W + (q & 1)) * a.C, v);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if (mp_takes(v[k], m[k])) m[k] = v[k];
    }
    st16<T, V>(y + (size_t)i * V, m);
  }
}

// one thread per dx vector (n, h, w, cv): gather from the windows that contain (h, w)
template <typename T>
__global__ void __launch_bounds__(PC_THREADS)
    maxpool2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx, PoolArgs a) {
  constexpr int V = Elt<T>::PER16;
  for (uint32_t i = blockIdx.x * PC_THREADS + threadIdx.x; i < a.total; i += gridDim.x * PC_THREADS) {
    const uint32_t pix = fdiv(i, a.fd_cv), cv = i - pix * a.CV;
    const uint32_t row = fdiv(pix, a.fd_w), w = pix - row * a.W;
    const uint32_t n = fdiv(row, a.fd_h), h = row - n * a.H;
    const int s = a.s;
    // windows oh with oh * s <= h <= oh * s + 1 inside [0, Ho)
    const int oh0 = h >= 1 ? ((int)h - 1 + s - 1) / s : 0, oh1 = min((int)h / s, a.Ho - 1);
    const int ow0 = w >= 1 ? ((int)w - 1 + s - 1) / s : 0, ow1 = min((int)w / s, a.Wo - 1);
    float acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k] = 0.f;
    for (int oh = oh0; oh <= oh1; ++oh)
      for (int ow = ow0; ow <= ow1; ++ow) {
        const T* p = x + (((size_t)n * a.H + oh * s) * a.W + ow * s) * a.C + cv * V;
        const int mine = ((int)h - oh * s) * 2 + ((int)w - ow * s);
        float m[V];
        int idx[V];
#pragma unroll
        for (int k = 0; k < V; ++k) m[k] = -INFINITY, idx[k] = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float v[V];
          ld16<T, V>(p + ((size_t)(q >> 1) * a.W + (q & 1)) * a.C, v);
#pragma unroll
          for (int k = 0; k < V; ++k)
            if (mp_takes(v[k], m[k])) m[k] = v[k], idx[k] = q;
        }
        float g[V];
        ld16<T, V>(dy + ((((size_t)n * a.Ho + oh) * a.Wo + ow) * a.C + cv * V), g);
#pragma unroll
        for (int k = 0; k < V; ++k)
          if (idx[k] == mine) acc[k] += g[k];
      }
    st16<T, V>(dx + (size_t)i * V, acc);
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

// grid (tiles * tiles, S, N); out = G (S == 1, values times scale) or the partials [N][S][C][C]
template <typename T>
__global__ void __launch_bounds__(PC_THREADS)
    gram_fwd_kernel(const T* __restrict__ F, float* __restrict__ out, int HW, int C, int tiles, int S, int kb, float scale) {
  constexpr int V = Elt<T>::PER16;
  constexpr int LDT = GR_KT + V;   // row stride in elements: 144 B (bf16) / 272 B (fp32), 16-byte multiples
  constexpr int CG = GR_TILE / V;  // 16-byte vectors per staged row of F
  __shared__ __attribute__((aligned(16))) T sA[GR_TILE * LDT];
  __shared__ __attribute__((aligned(16))) T sB[GR_TILE * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int ti = blockIdx.x / tiles, tj = blockIdx.x - ti * tiles, sp = blockIdx.y, n = blockIdx.z;
  const T* Fn = F + (size_t)n * HW * C;
  const int k_begin = sp * kb, k_end = min(HW, k_begin + kb);
  const bool diag = ti == tj;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // dst[channel c0 + c][k] = F[k0 + k][c0 + c]; rows past k_end and channels past C are zeros (a vector
  // of V channels is inside or outside as a whole: C % 8 == 0)
  auto stage = [&](T* dst, int c0, int k0) {
    for (int v = tid; v < GR_KT * CG; v += PC_THREADS) {
      const int kl = v / CG, cg = v - kl * CG;
      const int k = k0 + kl, c = c0 + cg * V;
      u32x4 q = u32x4{0u, 0u, 0u, 0u};
      if (k < k_end && c < C) q = *(const u32x4*)(Fn + (size_t)k * C + c);
      T* d = dst + (cg * V) * LDT + kl;
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
    }
  };

  for (int k0 = k_begin; k0 < k_end; k0 += GR_KT) {
    stage(sA, ti * GR_TILE, k0);
    if (!diag) stage(sB, tj * GR_TILE, k0);
    __syncthreads();
    const T* pB = diag ? sA : sB;
#pragma unroll
    for (int kk = 0; kk < GR_KT; kk += 4 * V) {
      u32x4 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *(const u32x4*)(sA + (wr * 32 + i * 16 + fr) * LDT + kk + fq * V);
        b[i] = *(const u32x4*)(pB + (wc * 32 + i * 16 + fr) * LDT + kk + fq * V);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mfma_k<T>(a[i], b[j], acc[i][j]);
    }
    __syncthreads();
  }

  float* dst = out + ((size_t)n * S + sp) * C * C;
  const float scl = S == 1 ? scale : 1.f;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti * GR_TILE + wr * 32 + i * 16 + fq * 4 + r, gj = tj * GR_TILE + wc * 32 + j * 16 + fr;
        if (gi < C && gj < C) dst[(size_t)gi * C + gj] = acc[i][j][r] * scl;
      }
}

// G[n][e] = scale * sum over s of part[n][s][e], e over the C * C elements.  A block owns 64 consecutive
// elements; wave g of its four sums the g-th quarter of the splits in split order (a wave reads 256
// contiguous bytes per split), and the four quarter sums are added in quarter order: a fixed order.
__global__ void __launch_bounds__(PC_THREADS)
    gram_reduce_kernel(const float* __restrict__ part, float* __restrict__ G, uint32_t total, uint32_t CC, FastDiv fd_cc,
                       int S, float scale) {
  __shared__ float red[PC_THREADS];
  const int el = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * 64u + el;
  const int per = (S + 3) / 4, s0 = grp * per, s1 = min(S, s0 + per);
  float s = 0.f;
  if (i < total) {
    const uint32_t n = fdiv(i, fd_cc), e = i - n * CC;
    const float* p = part + (size_t)n * S * CC + e;
    for (int k = s0; k < s1; ++k) s += p[(size_t)k * CC];
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (grp == 0 && i < total) G[i] = (((red[el] + red[64 + el]) + red[128 + el]) + red[192 + el]) * scale;
}

// grid (ceil(row tiles / rpb), ceil(C / 64), N): a block computes rpb consecutive 64-row tiles of one
// 64-column slice of dF[n]
template <typename T>
__global__ void __launch_bounds__(PC_THREADS)
    gram_bwd_kernel(const T* __restrict__ F, const float* __restrict__ dG, const T* __restrict__ res, T* __restrict__ dF,
                    int HW, int C, int rpb, float alpha, float beta) {
  constexpr int V = Elt<T>::PER16;
  constexpr int CG = GR_TILE / V;
  __shared__ __attribute__((aligned(16))) float sF[GR_TILE * GB_LD];
  __shared__ __attribute__((aligned(16))) float sS[GR_TILE * GB_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, fr = lane & 15, fq = lane >> 4;
  const int n = blockIdx.z, c0 = blockIdx.y * GR_TILE;
  const T* Fn = F + (size_t)n * HW * C;
  const T* Rn = res ? res + (size_t)n * HW * C : nullptr;
  T* On = dF + (size_t)n * HW * C;
  const float* Gn = dG + (size_t)n * C * C;
  const int row_tiles = (HW + GR_TILE - 1) / GR_TILE;
  const int rt0 = blockIdx.x * rpb, rt1 = min(row_tiles, rt0 + rpb);
  const bool one_k = C <= GR_TILE;  // a single K step: the Sym tile is staged once per block

  for (int rt = rt0; rt < rt1; ++rt) {
    const int r0 = rt * GR_TILE;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < C; j0 += GR_TILE) {
      if (!one_k || rt == rt0) {
        // sS[c][j] = dG[c0 + c][j0 + j] + dG[j0 + j][c0 + c] (zeros past C), both terms read along dG's
        // rows: the first lands as it is read, the second is added transposed in LDS (every element of sS
        // by exactly one thread)
        for (int e = tid; e < GR_TILE * (GR_TILE / 4); e += PC_THREADS) {
          const int cl = e / (GR_TILE / 4), jq = e - cl * (GR_TILE / 4);
          const int c = c0 + cl, j = j0 + jq * 4;
          f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
          if (c < C && j < C) v = *(const f32x4*)(Gn + (size_t)c * C + j);
          *(f32x4*)(sS + cl * GB_LD + jq * 4) = v;
        }
        __syncthreads();
        for (int e = tid; e < GR_TILE * (GR_TILE / 4); e += PC_THREADS) {
          const int jl = e / (GR_TILE / 4), cq = e - jl * (GR_TILE / 4);
          const int j = j0 + jl, c = c0 + cq * 4;
          if (j < C && c < C) {
            const f32x4 v = *(const f32x4*)(Gn + (size_t)j * C + c);
#pragma unroll
            for (int q = 0; q < 4; ++q) sS[(cq * 4 + q) * GB_LD + jl] += v[q];
          }
        }
      }
      // sF[row][j] = F[r0 + row][j0 + j] as fp32 (zeros past HW / C)
      for (int v = tid; v < GR_TILE * CG; v += PC_THREADS) {
        const int rl = v / CG, cg = v - rl * CG;
        const int r = r0 + rl, j = j0 + cg * V;
        float f[V];
#pragma unroll
        for (int k = 0; k < V; ++k) f[k] = 0.f;
        if (r < HW && j < C) ld16<T, V>(Fn + (size_t)r * C + j, f);
#pragma unroll
        for (int k = 0; k < V; k += 4) *(f32x4*)(sF + rl * GB_LD + cg * V + k) = f32x4{f[k], f[k + 1], f[k + 2], f[k + 3]};
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < GR_TILE; kk += 16) {
        u32x4 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *(const u32x4*)(sF + (wr * 32 + i * 16 + fr) * GB_LD + kk + fq * 4);
          b[i] = *(const u32x4*)(sS + (wc * 32 + i * 16 + fr) * GB_LD + kk + fq * 4);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) mfma_k<float>(a[i], b[j], acc[i][j]);
      }
      __syncthreads();
    }
    // the tile through LDS, so that the store (and the residual load) is 16 bytes over the channels
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sF[(wr * 32 + i * 16 + fq * 4 + r) * GB_LD + wc * 32 + j * 16 + fr] = acc[i][j][r];
    __syncthreads();
    for (int v = tid; v < GR_TILE * CG; v += PC_THREADS) {
      const int rl = v / CG, cg = v - rl * CG;
      const int r = r0 + rl, c = c0 + cg * V;
      if (r < HW && c < C) {
        float o[V];
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = alpha * sF[rl * GB_LD + cg * V + k];
        if (Rn) {
          float rv[V];
          ld16<T, V>(Rn + (size_t)r * C + c, rv);
#pragma unroll
          for (int k = 0; k < V; ++k) o[k] = fmaf(beta, rv[k], o[k]);
        }
        st16<T, V>(On + (size_t)r * C + c, o);
      }
    }
    __syncthreads();
  }
}

unsigned pc_grid(int64_t n) {
  int64_t g = (n + PC_THREADS - 1) / PC_THREADS;
  if (g > PC_MAX_BLOCKS) g = PC_MAX_BLOCKS;
  return (unsigned)(g < 1 ? 1 : g);
}

// split-K plan of the Gram forward: S blocks of kb rows (the last one shorter)
void gram_plan(int HW, int& S, int& kb) {
  const int64_t blocks = ((int64_t)HW + GRAM_KBLOCK - 1) / GRAM_KBLOCK;
  const int64_t m = (blocks + GRAM_MAX_SPLITS - 1) / GRAM_MAX_SPLITS;
  kb = (int)(GRAM_KBLOCK * (m < 1 ? 1 : m));
  S = (int)(((int64_t)HW + kb - 1) / kb);
}

bool dtype_ok(int dtype) { return dtype == SR_F32 || dtype == SR_BF16; }

// shared argument checks of the two pooling entries; fills a (without total / fd_*)
int pool_check(const char* what, int dtype, const void* p0, const void* p1, const void* p2, int N, int H, int W, int C,
               int stride, PoolArgs& a) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    return sr_fail(code, msg);
  };
  if (!p0 || !p1 || !p2 || N <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(SR_EINVAL, "bad arguments");
  if (!dtype_ok(dtype)) return fail(SR_EINVAL, "dtype must be fp32 or bf16");
  if (stride != 1 && stride != 2) return fail(SR_EINVAL, "stride must be 1 or 2");
  if (H < 2 || W < 2) return fail(SR_EINVAL, "the map is smaller than the 2 x 2 window");
  if (C % 8) return fail(SR_EINVAL, "C must be a multiple of 8");
  if (((uintptr_t)p0 | (uintptr_t)p1 | (uintptr_t)p2) & 15) return fail(SR_EINVAL, "tensors must be 16-byte aligned");
  if ((int64_t)N * H * W * C * (dtype == SR_BF16 ? 2 : 4) >= 0x80000000ll) return fail(SR_ETOOBIG, "tensor too large");
  a.H = H, a.W = W, a.C = C, a.s = stride;
  a.Ho = (H - 2) / stride + 1, a.Wo = (W - 2) / stride + 1;
  a.CV = C / (dtype == SR_BF16 ? 8 : 4);
  a.fd_cv = make_fastdiv((uint32_t)a.CV);
  return SR_OK;
}

}  // namespace

extern "C" {

int sr_maxpool2_fwd(int dtype, const void* x, int N, int H, int W, int C, int stride, void* y, void* stream) {
  PoolArgs a;
  if (int rc = pool_check("maxpool2_fwd", dtype, x, y, y, N, H, W, C, stride, a)) return rc;
  a.total = (uint32_t)((int64_t)N * a.Ho * a.Wo * a.CV);
  a.fd_w = make_fastdiv((uint32_t)a.Wo), a.fd_h = make_fastdiv((uint32_t)a.Ho);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(maxpool2_fwd_kernel<bf16_t>, dim3(pc_grid(a.total)), dim3(PC_THREADS), 0, s, (const bf16_t*)x,
                       (bf16_t*)y, a);
  else
    hipLaunchKernelGGL(maxpool2_fwd_kernel<float>, dim3(pc_grid(a.total)), dim3(PC_THREADS), 0, s, (const float*)x,
                       (float*)y, a);
  return sr_check(hipGetLastError(), "maxpool2_fwd launch");
}

int sr_maxpool2_bwd(int dtype, const void* x, const void* dy, int N, int H, int W, int C, int stride, void* dx,
                    void* stream) {
  PoolArgs a;
  if (int rc = pool_check("maxpool2_bwd", dtype, x, dy, dx, N, H, W, C, stride, a)) return rc;
  a.total = (uint32_t)((int64_t)N * H * W * a.CV);
  a.fd_w = make_fastdiv((uint32_t)W), a.fd_h = make_fastdiv((uint32_t)H);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(maxpool2_bwd_kernel<bf16_t>, dim3(pc_grid(a.total)), dim3(PC_THREADS), 0, s, (const bf16_t*)x,
                       (const bf16_t*)dy, (bf16_t*)dx, a);
  else
    hipLaunchKernelGGL(maxpool2_bwd_kernel<float>, dim3(pc_grid(a.total)), dim3(PC_THREADS), 0, s, (const float*)x,
                       (const float*)dy, (float*)dx, a);
  return sr_check(hipGetLastError(), "maxpool2_bwd launch");
}

int sr_gram_kblock(void) { return GRAM_KBLOCK; }

int sr_gram_splits(int HW) {
  if (HW <= 0) return 0;
  int S, kb;
  gram_plan(HW, S, kb);
  return S;
}

size_t sr_gram_workspace(int N, int HW, int C) {
  if (N <= 0 || HW <= 0 || C <= 0) return 0;
  int S, kb;
  gram_plan(HW, S, kb);
  return S > 1 ? (size_t)N * S * C * C * sizeof(float) : 0;
}

int sr_gram_fwd(int dtype, const void* F, int N, int HW, int C, float scale, float* G, void* ws, size_t ws_bytes,
                void* stream) {
  if (!F || !G || N <= 0 || HW <= 0 || C <= 0) return sr_fail(SR_EINVAL, "gram_fwd: bad arguments");
  if (!dtype_ok(dtype)) return sr_fail(SR_EINVAL, "gram_fwd: dtype must be fp32 or bf16");
  if (C % 8 || C > 512) return sr_fail(SR_EINVAL, "gram_fwd: C must be a multiple of 8, at most 512");
  if (N > 65535) return sr_fail(SR_EINVAL, "gram_fwd: at most 65535 images");
  if (((uintptr_t)F & 15) || ((uintptr_t)G & 3)) return sr_fail(SR_EINVAL, "gram_fwd: F must be 16-byte, G 4-byte aligned");
  if ((int64_t)N * HW * C * (dtype == SR_BF16 ? 2 : 4) >= 0x80000000ll || (int64_t)N * C * C >= 0x80000000ll)
    return sr_fail(SR_ETOOBIG, "gram_fwd: tensor too large");
  int S, kb;
  gram_plan(HW, S, kb);
  const size_t need = sr_gram_workspace(N, HW, C);
  if (S > 1 && (!ws || ((uintptr_t)ws & 3) || ws_bytes < need))
    return sr_fail(SR_EINVAL, "gram_fwd: workspace missing, misaligned or smaller than sr_gram_workspace()");
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (C + GR_TILE - 1) / GR_TILE;
  float* out = S > 1 ? (float*)ws : G;
  const dim3 grid((unsigned)(tiles * tiles), (unsigned)S, (unsigned)N);
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(gram_fwd_kernel<bf16_t>, grid, dim3(PC_THREADS), 0, s, (const bf16_t*)F, out, HW, C, tiles, S, kb,
                       scale);
  else
    hipLaunchKernelGGL(gram_fwd_kernel<float>, grid, dim3(PC_THREADS), 0, s, (const float*)F, out, HW, C, tiles, S, kb,
                       scale);
  if (S > 1) {
    const uint32_t CC = (uint32_t)C * C, total = (uint32_t)N * CC;
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((total + 63) / 64), dim3(PC_THREADS), 0, s, (const float*)ws, G, total, CC,
                       make_fastdiv(CC), S, scale);
  }
  return sr_check(hipGetLastError(), "gram_fwd launch");
}

int sr_gram_bwd(int dtype, const void* F, const float* dG, const void* res, int N, int HW, int C, float alpha, float beta,
                void* dF, void* stream) {
  if (!F || !dG || !dF || N <= 0 || HW <= 0 || C <= 0) return sr_fail(SR_EINVAL, "gram_bwd: bad arguments");
  if (!dtype_ok(dtype)) return sr_fail(SR_EINVAL, "gram_bwd: dtype must be fp32 or bf16");
  if (C % 8 || C > 512) return sr_fail(SR_EINVAL, "gram_bwd: C must be a multiple of 8, at most 512");
  if (N > 65535) return sr_fail(SR_EINVAL, "gram_bwd: at most 65535 images");
  if (((uintptr_t)F | (uintptr_t)dG | (uintptr_t)res | (uintptr_t)dF) & 15)
    return sr_fail(SR_EINVAL, "gram_bwd: tensors must be 16-byte aligned");
  if ((int64_t)N * HW * C * (dtype == SR_BF16 ? 2 : 4) >= 0x80000000ll || (int64_t)N * C * C >= 0x80000000ll)
    return sr_fail(SR_ETOOBIG, "gram_bwd: tensor too large");
  const int row_tiles = (HW + GR_TILE - 1) / GR_TILE, col_tiles = (C + GR_TILE - 1) / GR_TILE;
  // one K step (C <= 64): several row tiles per block share the staged Sym tile, once there are more than
  // GB_MIN_BLOCKS tiles to hand out
  int rpb = 1;
  if (C <= GR_TILE) {
    const int64_t want = (int64_t)row_tiles * N / GB_MIN_BLOCKS;
    rpb = (int)(want < 1 ? 1 : (want > 8 ? 8 : want));
  }
  const dim3 grid((unsigned)((row_tiles + rpb - 1) / rpb), (unsigned)col_tiles, (unsigned)N);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(gram_bwd_kernel<bf16_t>, grid, dim3(PC_THREADS), 0, s, (const bf16_t*)F, dG, (const bf16_t*)res,
                       (bf16_t*)dF, HW, C, rpb, alpha, beta);
  else
    hipLaunchKernelGGL(gram_bwd_kernel<float>, grid, dim3(PC_THREADS), 0, s, (const float*)F, dG, (const float*)res,
                       (float*)dF, HW, C, rpb, alpha, beta);
  return sr_check(hipGetLastError(), "gram_bwd launch");
}

}  // extern "C"
