// Kernels of the U-Net discriminator with spectral normalisation (basicsr/archs/discriminator_arch.py:91-150) that
// the conv engine and gan.hip do not cover: the grouped spectral normalisation of conv weights and the bilinear x2
// upsampling of NHWC maps.
//
// Spectral norm (torch.nn.utils.spectral_norm, one power iteration, eps 1e-12), GROUPED: one call serves up to
// SR_SN_MAX_PROBLEMS weight matrices M = weight_orig [R][K], so the launch count does not depend on their number.
// The problem table travels in the kernel-argument segment (no upload, nothing to keep alive); grid y = problem,
// blocks past a problem's own count leave at once.
//   sn_col_kernel   : t = M^T u.  A thread owns one column and walks the SN_RS rows of its row split in row order;
//                     fp32 partials part[split][K].
//   sn_v_kernel     : t[k] = the partials in split order; ||t|| by a fixed tree; v = t / max(||t||, eps), written to
//                     the persistent buffer and to this forward's copy.  Eval: the copy only.
//   sn_row_kernel   : s = M v, one wave per row, lanes stride the row (16-byte loads), fixed xor tree.
//   sn_u_kernel     : ||s||; u = s / max(||s||, eps) (training) written as v is; sigma = u . s by a fixed tree.
//   sn_scale_kernel : W = weight_orig / sigma in the nn.Conv2d layout.
//   sn_dot_kernel + sn_bwd_kernel : d = <G, W> over SN_DOT_BLOCKS contiguous chunks, summed in chunk order; then
//                     dweight_orig (=, +=) (G - d u v^T) / sigma.  A problem without G is skipped.
// Bilinear x2 (align_corners=False) of NHWC maps, 16-byte channel vectors, fp32 arithmetic, one rounding on store:
//   up2_fwd_kernel  : out[2i] = .25 in[max(i-1,0)] + .75 in[i], out[2i+1] = .75 in[i] + .25 in[min(i+1,n-1)] per axis.
//   up2_bwd_kernel  : the transpose as a gather: dx[j] = .25 dy[2j-1] + .75 dy[2j] + .75 dy[2j+1] + .25 dy[2j+2] per
//                     axis with the indices clamped to the map, so the clamped edge taps fold onto the edge pixel.
//
// No atomics, fixed summation orders: two runs give identical bits.  Nothing allocates or synchronises.
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int SN_T = 256;
constexpr int SN_RS = 32;           // rows per split of the column pass
constexpr int SN_DOT_BLOCKS = 64;   // chunks of the backward's dot
constexpr int SN_EW_BLOCKS = 256;   // blocks per problem of the element-wise passes
constexpr int UP_T = 256;
constexpr int UP_FWD_BLOCKS = 768;
constexpr int UP_BWD_BLOCKS = 192;

struct SnItem {
  const float* w;
  float *u, *v, *u_fwd, *v_fwd, *sigma, *out;
  const float* g;
  float *part, *s;
  int R, K, vec, ctiles, rsplits;
  FastDiv fd_k;
};
struct SnTable {
  SnItem it[SR_SN_MAX_PROBLEMS];
};

// sum over the block in a fixed tree; every thread gets it
SR_DEV float sn_block_sum(float s, float* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = SN_T / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__global__ void __launch_bounds__(SN_T) sn_col_kernel(SnTable t) {
  const SnItem& p = t.it[blockIdx.y];
  if ((int)blockIdx.x >= p.ctiles * p.rsplits) return;
  const int rs = blockIdx.x / p.ctiles, ct = blockIdx.x - rs * p.ctiles;
  const int k = ct * SN_T + threadIdx.x;
  if (k >= p.K) return;
  const int r0 = rs * SN_RS, r1 = min(p.R, r0 + SN_RS);
  const float* col = p.w + k;
  float acc = 0.f;
#pragma unroll 4
  for (int r = r0; r < r1; ++r) acc = fmaf(col[(size_t)r * p.K], p.u[r], acc);
  p.part[(size_t)rs * p.K + k] = acc;
}

__global__ void __launch_bounds__(SN_T) sn_v_kernel(SnTable t, int iterate, float eps) {
  __shared__ float red[SN_T];
  const SnItem& p = t.it[blockIdx.x];
  const int tid = threadIdx.x;
  if (!iterate) {
    for (int k = tid; k < p.K; k += SN_T) p.v_fwd[k] = p.v[k];
    return;
  }
  float ss = 0.f;
  for (int k = tid; k < p.K; k += SN_T) {
    float a = 0.f;
    for (int rs = 0; rs < p.rsplits; ++rs) a += p.part[(size_t)rs * p.K + k];
    p.part[k] = a;  // split 0's slot of this thread's own column
    ss = fmaf(a, a, ss);
  }
  const float d = fmaxf(sqrtf(sn_block_sum(ss, red)), eps);
  for (int k = tid; k < p.K; k += SN_T) {
    const float vv = p.part[k] / d;
    p.v[k] = vv;
    p.v_fwd[k] = vv;
  }
}

__global__ void __launch_bounds__(SN_T) sn_row_kernel(SnTable t) {
  const SnItem& p = t.it[blockIdx.y];
  const int lane = threadIdx.x & 63, r = blockIdx.x * (SN_T / 64) + (threadIdx.x >> 6);
  if (r >= p.R) return;
  const float* row = p.w + (size_t)r * p.K;
  const float* v = p.v_fwd;
  float acc = 0.f;
  if (p.vec) {
    for (int k = lane * 4; k < p.K; k += 256) {
      const f32x4 a = *(const f32x4*)(row + k), b = *(const f32x4*)(v + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(a[j], b[j], acc);
    }
  } else {
    for (int k = lane; k < p.K; k += 64) acc = fmaf(row[k], v[k], acc);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) p.s[r] = acc;
}

__global__ void __launch_bounds__(SN_T) sn_u_kernel(SnTable t, int iterate, float eps) {
  __shared__ float red[SN_T];
  const SnItem& p = t.it[blockIdx.x];
  const int tid = threadIdx.x;
  float d = 1.f;
  if (iterate) {
    float ss = 0.f;
    for (int r = tid; r < p.R; r += SN_T) ss = fmaf(p.s[r], p.s[r], ss);
    d = fmaxf(sqrtf(sn_block_sum(ss, red)), eps);
  }
  float dot = 0.f;
  for (int r = tid; r < p.R; r += SN_T) {
    const float sr = p.s[r];
    float uu;
    if (iterate) {
      uu = sr / d;
      p.u[r] = uu;
    } else {
      uu = p.u[r];
    }
    p.u_fwd[r] = uu;
    dot = fmaf(uu, sr, dot);
  }
  const float sig = sn_block_sum(dot, red);
  if (tid == 0) *p.sigma = sig;
}

__global__ void __launch_bounds__(SN_T) sn_scale_kernel(SnTable t) {
  const SnItem& p = t.it[blockIdx.y];
  const uint32_t total = (uint32_t)p.R * (uint32_t)p.K;
  const float sig = *p.sigma;
  if (p.vec) {
    for (uint32_t i = (blockIdx.x * SN_T + threadIdx.x) * 4u; i < total; i += gridDim.x * SN_T * 4u) {
      f32x4 a = *(const f32x4*)(p.w + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = a[j] / sig;
      *(f32x4*)(p.out + i) = a;
    }
  } else {
    for (uint32_t i = blockIdx.x * SN_T + threadIdx.x; i < total; i += gridDim.x * SN_T) p.out[i] = p.w[i] / sig;
  }
}

// part[b] = the dot of chunk b of G and W (p.w: the forward's normalised weight)
__global__ void __launch_bounds__(SN_T) sn_dot_kernel(SnTable t) {
  __shared__ float red[SN_T];
  const SnItem& p = t.it[blockIdx.y];
  if (!p.g) return;
  const uint32_t total = (uint32_t)p.R * (uint32_t)p.K;
  const uint32_t per = ((total + SN_DOT_BLOCKS - 1) / SN_DOT_BLOCKS + 3u) & ~3u;
  const uint32_t i0 = min(total, blockIdx.x * per), i1 = min(total, i0 + per);
  float acc = 0.f;
  if (p.vec) {
    for (uint32_t i = i0 + threadIdx.x * 4u; i < i1; i += SN_T * 4u) {
      const f32x4 a = *(const f32x4*)(p.g + i), b = *(const f32x4*)(p.w + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(a[j], b[j], acc);
    }
  } else {
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += SN_T) acc = fmaf(p.g[i], p.w[i], acc);
  }
  const float sum = sn_block_sum(acc, red);
  if (threadIdx.x == 0) p.part[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(SN_T) sn_bwd_kernel(SnTable t, int accumulate) {
  const SnItem& p = t.it[blockIdx.y];
  if (!p.g) return;
  const uint32_t total = (uint32_t)p.R * (uint32_t)p.K;
  float d = 0.f;
  for (int b = 0; b < SN_DOT_BLOCKS; ++b) d += p.part[b];
  const float sig = *p.sigma;
  if (p.vec) {
    for (uint32_t i = (blockIdx.x * SN_T + threadIdx.x) * 4u; i < total; i += gridDim.x * SN_T * 4u) {
      const uint32_t r = fdiv(i, p.fd_k), k = i - r * (uint32_t)p.K;  // K % 4 == 0: the four share the row
      const float du = d * p.u_fwd[r];
      const f32x4 g = *(const f32x4*)(p.g + i), v = *(const f32x4*)(p.v_fwd + k);
      f32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = (g[j] - du * v[j]) / sig;
      if (accumulate) {
        const f32x4 c = *(const f32x4*)(p.out + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = c[j] + o[j];
      }
      *(f32x4*)(p.out + i) = o;
    }
  } else {
    for (uint32_t i = blockIdx.x * SN_T + threadIdx.x; i < total; i += gridDim.x * SN_T) {
      const uint32_t r = fdiv(i, p.fd_k), k = i - r * (uint32_t)p.K;
      const float o = (p.g[i] - d * p.u_fwd[r] * p.v_fwd[k]) / sig;
      p.out[i] = accumulate ? p.out[i] + o : o;
    }
  }
}

size_t sn_align4(size_t n) { return (n + 3) & ~(size_t)3; }

// floats of problem i's workspace share: the column-pass partials (or the dot partials) and s
size_t sn_part_floats(int R, int K) {
  const size_t fwd = (size_t)((R + SN_RS - 1) / SN_RS) * K;
  return sn_align4(fwd > (size_t)SN_DOT_BLOCKS ? fwd : (size_t)SN_DOT_BLOCKS);
}

bool sn_shape_ok(const sr_sn_problem& q) { return q.R > 0 && q.K > 0 && (int64_t)q.R * q.K < 0x40000000ll; }

// validates and fills the by-value table; returns SR_OK or fails
int sn_table(const char* what, const sr_sn_problem* pr, int n, int bwd, void* ws, size_t ws_bytes, SnTable& t, int& max_r,
             int& max_colblocks) {
  static thread_local char msg[160];
  auto fail = [&](const char* why) {
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    return sr_fail(SR_EINVAL, msg);
  };
  if (!pr || !ws) return fail("null pointer");
  if (n <= 0 || n > SR_SN_MAX_PROBLEMS) return fail("between 1 and SR_SN_MAX_PROBLEMS problems per call");
  if ((uintptr_t)ws & 15) return fail("the workspace must be 16-byte aligned");
  if (ws_bytes < sr_spectral_norm_workspace(pr, n)) return fail("workspace smaller than sr_spectral_norm_workspace()");
  float* wp = (float*)ws;
  max_r = 0, max_colblocks = 0;
  for (int i = 0; i < n; ++i) {
    const sr_sn_problem& q = pr[i];
    SnItem& it = t.it[i];
    if (!sn_shape_ok(q)) return fail("R and K must be positive with R * K below 2^30");
    if (!q.w || !q.u_fwd || !q.v_fwd || !q.sigma) return fail("null pointer in a problem");
    if (!bwd && (!q.u || !q.v || !q.out)) return fail("null pointer in a problem");
    if (bwd && q.g && !q.out) return fail("a problem with a gradient needs its target");
    if (((uintptr_t)q.w | (uintptr_t)q.u | (uintptr_t)q.v | (uintptr_t)q.u_fwd | (uintptr_t)q.v_fwd | (uintptr_t)q.sigma |
         (uintptr_t)q.out | (uintptr_t)q.g) & 3)
      return fail("pointers must be 4-byte aligned");
    it.w = q.w, it.u = q.u, it.v = q.v, it.u_fwd = q.u_fwd, it.v_fwd = q.v_fwd, it.sigma = q.sigma, it.out = q.out;
    it.g = bwd ? q.g : nullptr;
    it.R = q.R, it.K = q.K;
    it.vec = q.K % 4 == 0 && !(((uintptr_t)q.w | (uintptr_t)q.v_fwd | (uintptr_t)q.out | (uintptr_t)it.g) & 15);
    it.ctiles = (q.K + SN_T - 1) / SN_T, it.rsplits = (q.R + SN_RS - 1) / SN_RS;
    it.fd_k = make_fastdiv((uint32_t)q.K);
    it.part = wp;
    wp += sn_part_floats(q.R, q.K);
    it.s = wp;
    wp += sn_align4((size_t)q.R);
    if (q.R > max_r) max_r = q.R;
    if (it.ctiles * it.rsplits > max_colblocks) max_colblocks = it.ctiles * it.rsplits;
  }
  return SR_OK;
}

// --------------------------------------------------------------------------------------------- bilinear x2

template <typename T, int V>
SR_DEV void up_ld(const T* __restrict__ p, float (&v)[V]) {
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
SR_DEV void up_st(T* __restrict__ p, const float (&v)[V]) {
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

struct UpArgs {
  int H, W, CV;      // the SMALL map and its 16-byte vectors per pixel
  uint32_t total;    // vectors of the map a thread writes
  FastDiv fd_cv, fd_w, fd_h;  // of the written map: vectors per pixel, width, height
  float scale;       // the SCALED kernels multiply the fp32 result by it before the store
};

// one thread per output vector: y[n][oy][ox] from the 2 x 2 input pixels (near .75, far .25 per axis)
template <typename T, bool SCALED>
__global__ void __launch_bounds__(UP_T) up2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, UpArgs a) {
  constexpr int V = Elt<T>::PER16;
  const int W2 = 2 * a.W, H2 = 2 * a.H;
  for (uint32_t i = blockIdx.x * UP_T + threadIdx.x; i < a.total; i += gridDim.x * UP_T) {
    const uint32_t pix = fdiv(i, a.fd_cv), cv = i - pix * a.CV;
    const uint32_t row = fdiv(pix, a.fd_w), ox = pix - row * W2;
    const uint32_t n = fdiv(row, a.fd_h), oy = row - n * H2;
    const int iy = oy >> 1, ix = ox >> 1;
    const int yf = (oy & 1) ? min(iy + 1, a.H - 1) : max(iy - 1, 0);
    const int xf = (ox & 1) ? min(ix + 1, a.W - 1) : max(ix - 1, 0);
    const T* base = x + (size_t)n * a.H * a.W * a.CV * V + (size_t)cv * V;
    float nn[V], nf[V], fn[V], ff[V], o[V];
    up_ld<T, V>(base + ((size_t)iy * a.W + ix) * a.CV * V, nn);
    up_ld<T, V>(base + ((size_t)iy * a.W + xf) * a.CV * V, nf);
    up_ld<T, V>(base + ((size_t)yf * a.W + ix) * a.CV * V, fn);
    up_ld<T, V>(base + ((size_t)yf * a.W + xf) * a.CV * V, ff);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float rn = fmaf(0.75f, nn[k], 0.25f * nf[k]), rf = fmaf(0.75f, fn[k], 0.25f * ff[k]);
      o[k] = fmaf(0.75f, rn, 0.25f * rf);
      if constexpr (SCALED) o[k] *= a.scale;
    }
    up_st<T, V>(y + (size_t)i * V, o);
  }
}

// one thread per dx vector: the 4 x 4 dy pixels 2j - 1 .. 2j + 2 per axis (clamped), weights .25 .75 .75 .25
template <typename T, bool SCALED>
__global__ void __launch_bounds__(UP_T) up2_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, UpArgs a) {
  constexpr int V = Elt<T>::PER16;
  const int W2 = 2 * a.W, H2 = 2 * a.H;
  for (uint32_t i = blockIdx.x * UP_T + threadIdx.x; i < a.total; i += gridDim.x * UP_T) {
    const uint32_t pix = fdiv(i, a.fd_cv), cv = i - pix * a.CV;
    const uint32_t row = fdiv(pix, a.fd_w), ix = pix - row * a.W;
    const uint32_t n = fdiv(row, a.fd_h), iy = row - n * a.H;
    const int ys[4] = {max(2 * (int)iy - 1, 0), 2 * (int)iy, 2 * (int)iy + 1, min(2 * (int)iy + 2, H2 - 1)};
    const int xs[4] = {max(2 * (int)ix - 1, 0), 2 * (int)ix, 2 * (int)ix + 1, min(2 * (int)ix + 2, W2 - 1)};
    const T* base = dy + (size_t)n * H2 * W2 * a.CV * V + (size_t)cv * V;
    float outer[V], inner[V], o[V];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const T* rp = base + (size_t)ys[r] * W2 * a.CV * V;
      float p0[V], p1[V], p2[V], p3[V];
      up_ld<T, V>(rp + (size_t)xs[0] * a.CV * V, p0);
      up_ld<T, V>(rp + (size_t)xs[1] * a.CV * V, p1);
      up_ld<T, V>(rp + (size_t)xs[2] * a.CV * V, p2);
      up_ld<T, V>(rp + (size_t)xs[3] * a.CV * V, p3);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float tr = fmaf(0.75f, p1[k] + p2[k], 0.25f * (p0[k] + p3[k]));
        if (r == 0) outer[k] = tr;
        else if (r == 1) inner[k] = tr;
        else if (r == 2) inner[k] += tr;
        else outer[k] += tr;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      o[k] = fmaf(0.75f, inner[k], 0.25f * outer[k]);
      if constexpr (SCALED) o[k] *= a.scale;
    }
    up_st<T, V>(dx + (size_t)i * V, o);
  }
}

int up_check(const char* what, int dtype, const void* a, const void* b, int N, int H, int W, int C, UpArgs& u, bool bwd) {
  static thread_local char msg[160];
  auto fail = [&](int code, const char* why) {
    snprintf(msg, sizeof msg, "%s: %s", what, why);
    return sr_fail(code, msg);
  };
  if (!a || !b) return fail(SR_EINVAL, "null pointer");
  if (dtype != SR_F32 && dtype != SR_BF16) return fail(SR_EINVAL, "dtype must be fp32 or bf16");
  if (N <= 0 || H <= 0 || W <= 0 || C < 8 || C % 8) return fail(SR_EINVAL, "bad arguments (C a multiple of 8)");
  if (((uintptr_t)a | (uintptr_t)b) & 15) return fail(SR_EINVAL, "tensors must be 16-byte aligned");
  const int64_t esz = dtype == SR_BF16 ? 2 : 4;
  if ((int64_t)N * 4 * H * W * C * esz >= 0x80000000ll) return fail(SR_ETOOBIG, "tensor too large");
  const int V = dtype == SR_BF16 ? 8 : 4;
  u.H = H, u.W = W, u.CV = C / V;
  u.fd_cv = make_fastdiv((uint32_t)u.CV);
  if (bwd) {
    u.total = (uint32_t)((int64_t)N * H * W * u.CV);
    u.fd_w = make_fastdiv((uint32_t)W), u.fd_h = make_fastdiv((uint32_t)H);
  } else {
    u.total = (uint32_t)((int64_t)N * 4 * H * W * u.CV);
    u.fd_w = make_fastdiv((uint32_t)(2 * W)), u.fd_h = make_fastdiv((uint32_t)(2 * H));
  }
  return SR_OK;
}

unsigned up_grid(uint32_t total, int cap) {
  const uint32_t g = (total + UP_T - 1) / UP_T;
  return g > (uint32_t)cap ? (unsigned)cap : (g < 1 ? 1u : g);
}

}  // namespace

extern "C" {

size_t sr_spectral_norm_workspace(const sr_sn_problem* problems, int n) {
  if (!problems || n <= 0 || n > SR_SN_MAX_PROBLEMS) return 0;
  size_t f = 0;
  for (int i = 0; i < n; ++i) {
    if (!sn_shape_ok(problems[i])) return 0;
    f += sn_part_floats(problems[i].R, problems[i].K) + sn_align4((size_t)problems[i].R);
  }
  return f * sizeof(float);
}

int sr_spectral_norm_fwd(const sr_sn_problem* problems, int n, int iterate, float eps, void* ws, size_t ws_bytes,
                         void* stream) {
  SnTable t = {};
  int max_r, max_cb;
  if (int rc = sn_table("spectral_norm_fwd", problems, n, 0, ws, ws_bytes, t, max_r, max_cb)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (iterate) hipLaunchKernelGGL(sn_col_kernel, dim3((unsigned)max_cb, (unsigned)n), dim3(SN_T), 0, s, t);
  hipLaunchKernelGGL(sn_v_kernel, dim3((unsigned)n), dim3(SN_T), 0, s, t, iterate, eps);
  hipLaunchKernelGGL(sn_row_kernel, dim3((unsigned)((max_r + SN_T / 64 - 1) / (SN_T / 64)), (unsigned)n), dim3(SN_T), 0, s,
                     t);
  hipLaunchKernelGGL(sn_u_kernel, dim3((unsigned)n), dim3(SN_T), 0, s, t, iterate, eps);
  hipLaunchKernelGGL(sn_scale_kernel, dim3(SN_EW_BLOCKS, (unsigned)n), dim3(SN_T), 0, s, t);
  return sr_check(hipGetLastError(), "spectral_norm_fwd launch");
}

int sr_spectral_norm_bwd(const sr_sn_problem* problems, int n, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  SnTable t = {};
  int max_r, max_cb;
  if (int rc = sn_table("spectral_norm_bwd", problems, n, 1, ws, ws_bytes, t, max_r, max_cb)) return rc;
  bool any = false;
  for (int i = 0; i < n; ++i) any = any || t.it[i].g;
  if (!any) return SR_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sn_dot_kernel, dim3(SN_DOT_BLOCKS, (unsigned)n), dim3(SN_T), 0, s, t);
  hipLaunchKernelGGL(sn_bwd_kernel, dim3(SN_EW_BLOCKS, (unsigned)n), dim3(SN_T), 0, s, t, accumulate);
  return sr_check(hipGetLastError(), "spectral_norm_bwd launch");
}

int sr_bilinear_up2_fwd(int dtype, const void* x, int N, int H, int W, int C, void* y, void* stream) {
  UpArgs u;
  u.scale = 1.f;
  if (int rc = up_check("bilinear_up2_fwd", dtype, x, y, N, H, W, C, u, false)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(up_grid(u.total, UP_FWD_BLOCKS));
  if (dtype == SR_BF16)
    hipLaunchKernelGGL((up2_fwd_kernel<bf16_t, false>), grid, dim3(UP_T), 0, s, (const bf16_t*)x, (bf16_t*)y, u);
  else
    hipLaunchKernelGGL((up2_fwd_kernel<float, false>), grid, dim3(UP_T), 0, s, (const float*)x, (float*)y, u);
  return sr_check(hipGetLastError(), "bilinear_up2_fwd launch");
}

int sr_bilinear_up2_bwd(int dtype, const void* dy, int N, int H, int W, int C, void* dx, void* stream) {
  UpArgs u;
  u.scale = 1.f;
  if (int rc = up_check("bilinear_up2_bwd", dtype, dy, dx, N, H, W, C, u, true)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(up_grid(u.total, UP_BWD_BLOCKS));
  if (dtype == SR_BF16)
    hipLaunchKernelGGL((up2_bwd_kernel<bf16_t, false>), grid, dim3(UP_T), 0, s, (const bf16_t*)dy, (bf16_t*)dx, u);
  else
    hipLaunchKernelGGL((up2_bwd_kernel<float, false>), grid, dim3(UP_T), 0, s, (const float*)dy, (float*)dx, u);
  return sr_check(hipGetLastError(), "bilinear_up2_bwd launch");
}

int sr_bilinear_up2_fwd_scaled(int dtype, const void* x, int N, int H, int W, int C, float scale, void* y, void* stream) {
  UpArgs u;
  u.scale = scale;
  if (int rc = up_check("bilinear_up2_fwd_scaled", dtype, x, y, N, H, W, C, u, false)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(up_grid(u.total, UP_FWD_BLOCKS));
  if (dtype == SR_BF16)
    hipLaunchKernelGGL((up2_fwd_kernel<bf16_t, true>), grid, dim3(UP_T), 0, s, (const bf16_t*)x, (bf16_t*)y, u);
  else
    hipLaunchKernelGGL((up2_fwd_kernel<float, true>), grid, dim3(UP_T), 0, s, (const float*)x, (float*)y, u);
  return sr_check(hipGetLastError(), "bilinear_up2_fwd launch");
}

int sr_bilinear_up2_bwd_scaled(int dtype, const void* dy, int N, int H, int W, int C, float scale, void* dx, void* stream) {
  UpArgs u;
  u.scale = scale;
  if (int rc = up_check("bilinear_up2_bwd_scaled", dtype, dy, dx, N, H, W, C, u, true)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(up_grid(u.total, UP_BWD_BLOCKS));
  if (dtype == SR_BF16)
    hipLaunchKernelGGL((up2_bwd_kernel<bf16_t, true>), grid, dim3(UP_T), 0, s, (const bf16_t*)dy, (bf16_t*)dx, u);
  else
    hipLaunchKernelGGL((up2_bwd_kernel<float, true>), grid, dim3(UP_T), 0, s, (const float*)dy, (float*)dx, u);
  return sr_check(hipGetLastError(), "bilinear_up2_bwd launch");
}

}  // extern "C"
