// Pixel-loss family of the SR train step: L1, MSE and Charbonnier with an optional per-pixel weight map
// (basicsr/losses/basic_loss.py:12-114, weight_reduce_loss of loss_util.py:26-55), fused with the gradient
// w.r.t. the prediction.
//
//   pixel_loss_kernel : one streaming pass; per element d = pred - target, phi(d) and phi'(d) of the kind,
//       times the weight (none, [N,1,H,W] broadcast over channels, or [N,C,H,W]).  Reads pred and target
//       once, writes the gradient (and the elementwise map of reduction 'none') once, leaves one fp32
//       partial sum per block.
//   wsum_partial_kernel + wsum_final_kernel : the weighted mean's denominator (sum w, times C for a
//       one-channel map), folded in double and left in the workspace with the gradient scale
//       loss_weight / denom -- the main pass reads it from there, so it never visits the host.
//   loss_final_kernel : fold of the block partials in double (as l1_final_kernel of eltwise.hip).
//   gan_loss_kernel : the GANLoss family (basicsr/losses/gan_loss.py:89-112: vanilla, lsgan, wgan, wgan_softplus,
//       hinge) over a prediction of any shape, the same streaming pass and fold: the mean loss and its gradient.
//
// Every sum has a fixed order (per thread in element order, LDS tree per block, strided fold over the
// blocks): no atomics, two runs are bit-identical, and the launches can be captured in a HIP graph.
// A thread owns V consecutive elements (16 bytes of pred) per trip; a pointer that is 16-byte aligned is
// accessed with 16-byte vectors, one that is only element-aligned (a storage-offset view) with V scalar
// accesses -- the element-to-thread map and the arithmetic are the same, so the results are the same bits.
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int PL_THREADS = 256;
constexpr int PL_MAX_BLOCKS = 4096;
constexpr int PL_BLOCKS_PER_CU = 8;
// workspace: [0, 8) double denom, [8, 12) float gradient scale, [16, ...) loss partials, then weight partials
constexpr size_t PL_HEAD_BYTES = 16;

enum { AL_PRED = 1, AL_TGT = 2, AL_W = 4, AL_OUT = 8, AL_GRAD = 16 };

// v[0..V) = p[e0 .. e0 + cnt) as floats (the rest zero): 16-byte vector loads when `vec` (p + e0 is 16-byte
// aligned and cnt == V), scalar loads otherwise
template <typename T, int V>
SR_DEV void load_v(const T* __restrict__ p, int64_t e0, int cnt, bool vec, float (&v)[V]) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int j = 0; j < V / 4; ++j) {
        const f32x4 x = ((const f32x4*)(p + e0))[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * j + k] = x[k];
      }
    } else {
      static_assert(V == 8, "bf16 vectors carry 8 elements");
      const u32x4 x = *(const u32x4*)(p + e0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[2 * k] = bf16_to_f32((unsigned short)(x[k] & 0xffff));
        v[2 * k + 1] = bf16_to_f32((unsigned short)(x[k] >> 16));
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = k < cnt ? Elt<T>::to_f(p[e0 + k]) : 0.f;
  }
}

template <typename T, int V>
SR_DEV void store_v(T* __restrict__ p, int64_t e0, int cnt, bool vec, const float (&v)[V]) {
  if (vec) {
    if constexpr (sizeof(T) == 4) {
      static_assert(V == 4, "fp32 outputs carry 4 elements");
      f32x4 x;
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = v[k];
      *(f32x4*)(p + e0) = x;
    } else {
      static_assert(V == 8, "bf16 vectors carry 8 elements");
      u32x4 x;
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
      *(u32x4*)(p + e0) = x;
    }
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k)
      if (k < cnt) p[e0 + k] = Elt<T>::from_f(v[k]);
  }
}

// block sum of one float per thread in a fixed order -> partial[blockIdx.x]
SR_DEV void block_sum_store(float s, float* __restrict__ partial) {
  __shared__ float red[PL_THREADS];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = PL_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// WM: 0 no weight, 1 weight [N,1,H,W] (index n * HW + hw of element (n, c, hw)), 2 weight [N,C,H,W].
// out (may be null): lw * w * phi in pred's dtype; grad (may be null): w * phi' * gs, gs = *gs_dev when
// given (the weighted mean, written by wsum_final_kernel earlier on the stream), gs_arg otherwise.
template <int KIND, typename PT, typename TT, int WM>
__global__ void __launch_bounds__(PL_THREADS)
    pixel_loss_kernel(const PT* __restrict__ pred, const TT* __restrict__ tgt, const float* __restrict__ wt,
                      int64_t n, uint32_t HW, FastDiv fd_hw, FastDiv fd_c, float eps, float lw, float gs_arg,
                      const float* __restrict__ gs_dev, PT* __restrict__ out, PT* __restrict__ grad,
                      float* __restrict__ partial, unsigned al) {
  constexpr int V = Elt<PT>::PER16;
  const float gs = gs_dev ? *gs_dev : gs_arg;
  const int64_t nv = (n + V - 1) / V;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * PL_THREADS) {
    const int64_t e0 = i * V;
    const int cnt = n - e0 >= V ? V : (int)(n - e0);
    const bool full = cnt == V;
    float p[V], t[V], w[V], ov[V], gv[V];
    load_v<PT, V>(pred, e0, cnt, full && (al & AL_PRED), p);
    load_v<TT, V>(tgt, e0, cnt, full && (al & AL_TGT), t);
    if constexpr (WM == 2) {
      load_v<float, V>(wt, e0, cnt, full && (al & AL_W), w);
    } else if constexpr (WM == 1) {
      // plane = n * C + c of the first element; the V elements may run over a channel or image boundary
      const uint32_t plane = fdiv((uint32_t)e0, fd_hw);
      uint32_t hw = (uint32_t)e0 - plane * HW;
      uint32_t img = fdiv(plane, fd_c);
      const int64_t w0 = (int64_t)img * HW + hw;
      if (full && hw + V <= HW && (al & AL_W) && (w0 & 3) == 0) {
        load_v<float, V>(wt, w0, V, true, w);
      } else {
        uint32_t c = plane - img * fd_c.d;
#pragma unroll
        for (int k = 0; k < V; ++k) {
          w[k] = k < cnt ? wt[(int64_t)img * HW + hw] : 0.f;
          if (++hw == HW) {
            hw = 0;
            if (++c == fd_c.d) {
              c = 0;
              ++img;
            }
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float d = p[k] - t[k];
      float phi, dphi;
      if constexpr (KIND == SR_LOSS_L1) {
        phi = fabsf(d);
        dphi = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      } else if constexpr (KIND == SR_LOSS_MSE) {
        phi = d * d;
        dphi = d + d;
      } else {
        phi = sqrtf(d * d + eps);
        dphi = d / phi;
      }
      if constexpr (WM != 0) {
        phi *= w[k];
        dphi *= w[k];
      }
      if (k < cnt) s += phi;
      ov[k] = lw * phi;
      gv[k] = dphi * gs;
    }
    if (out) store_v<PT, V>(out, e0, cnt, full && (al & AL_OUT), ov);
    if (grad) store_v<PT, V>(grad, e0, cnt, full && (al & AL_GRAD), gv);
  }
  block_sum_store(s, partial);
}

__global__ void __launch_bounds__(PL_THREADS)
    wsum_partial_kernel(const float* __restrict__ wt, int64_t n, bool vec, float* __restrict__ partial) {
  const int64_t nv = (n + 3) / 4;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * PL_THREADS) {
    const int64_t e0 = i * 4;
    const int cnt = n - e0 >= 4 ? 4 : (int)(n - e0);
    float w[4];
    load_v<float, 4>(wt, e0, cnt, vec && cnt == 4, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) s += w[k];  // elements past the end were loaded as zeros
  }
  block_sum_store(s, partial);
}

SR_DEV double fold_partials(const float* __restrict__ partial, int nb) {
  __shared__ double red[PL_THREADS];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += PL_THREADS) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = PL_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

// denom = mult * sum w (mult = C for a one-channel map); gs = lw / denom
__global__ void __launch_bounds__(PL_THREADS)
    wsum_final_kernel(const float* __restrict__ partial, int nb, double mult, double lw, double* denom, float* gs) {
  const double sw = fold_partials(partial, nb);
  if (threadIdx.x == 0) {
    *denom = sw * mult;
    *gs = (float)(lw / (sw * mult));
  }
}

__global__ void __launch_bounds__(PL_THREADS)
    loss_final_kernel(const float* __restrict__ partial, int nb, double lw, double denom_arg,
                      const double* __restrict__ denom_dev, float* loss) {
  const double sum = fold_partials(partial, nb);
  if (threadIdx.x == 0) *loss = (float)(sum * lw / (denom_dev ? *denom_dev : denom_arg));
}

// GAN loss terms (basicsr/losses/gan_loss.py:89-112), one element x of the prediction -> (l, dl/dx).
// FORM 0: BCE with logits against the label t, max(x, 0) - x t + log1p(exp(-|x|)), gradient sigmoid(x) - t;
// FORM 1: (x - t)^2; FORM 2: sg * x; FORM 3: softplus(sg * x); FORM 4: relu(1 + sg * x).
SR_DEV float gl_sigmoid(float z) {
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
template <int FORM>
SR_DEV void gan_term(float x, float t, float sg, float& l, float& d) {
  if constexpr (FORM == 0) {
    l = fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
    d = gl_sigmoid(x) - t;
  } else if constexpr (FORM == 1) {
    l = (x - t) * (x - t);
    d = 2.f * (x - t);
  } else if constexpr (FORM == 2) {
    l = sg * x;
    d = sg;
  } else if constexpr (FORM == 3) {
    const float z = sg * x;
    l = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
    d = sg * gl_sigmoid(z);
  } else {
    const float z = 1.f + sg * x;
    l = z > 0.f ? z : 0.f;
    d = z > 0.f ? sg : 0.f;
  }
}

// one streaming pass: grad (may be null) = dl/dx * gs in pred's dtype, one fp32 partial sum of l per block
template <int FORM, typename PT>
__global__ void __launch_bounds__(PL_THREADS)
    gan_loss_kernel(const PT* __restrict__ pred, int64_t n, float t, float sg, float gs, PT* __restrict__ grad,
                    float* __restrict__ partial, unsigned al) {
  constexpr int V = Elt<PT>::PER16;
  const int64_t nv = (n + V - 1) / V;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; i < nv; i += (int64_t)gridDim.x * PL_THREADS) {
    const int64_t e0 = i * V;
    const int cnt = n - e0 >= V ? V : (int)(n - e0);
    const bool full = cnt == V;
    float p[V], gv[V];
    load_v<PT, V>(pred, e0, cnt, full && (al & AL_PRED), p);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      float l, d;
      gan_term<FORM>(p[k], t, sg, l, d);
      if (k < cnt) s += l;
      gv[k] = d * gs;
    }
    if (grad) store_v<PT, V>(grad, e0, cnt, full && (al & AL_GRAD), gv);
  }
  block_sum_store(s, partial);
}

template <int FORM>
void launch_gan(int dtype, unsigned grid, hipStream_t s, const void* pred, int64_t n, float t, float sg, float gs,
                void* grad, float* partial, unsigned al) {
  if (dtype == SR_BF16)
    hipLaunchKernelGGL((gan_loss_kernel<FORM, bf16_t>), dim3(grid), dim3(PL_THREADS), 0, s, (const bf16_t*)pred, n, t, sg, gs,
                       (bf16_t*)grad, partial, al);
  else
    hipLaunchKernelGGL((gan_loss_kernel<FORM, float>), dim3(grid), dim3(PL_THREADS), 0, s, (const float*)pred, n, t, sg, gs,
                       (float*)grad, partial, al);
}

// blocks of a streaming pass over nv vectors: PL_BLOCKS_PER_CU per CU, fewer when the work is smaller
unsigned loss_grid(int64_t nv) {
  int64_t g = (int64_t)sr_device_cus() * PL_BLOCKS_PER_CU;
  if (g > PL_MAX_BLOCKS) g = PL_MAX_BLOCKS;
  const int64_t need = (nv + PL_THREADS - 1) / PL_THREADS;
  if (g > need) g = need;
  return (unsigned)(g < 1 ? 1 : g);
}

struct LossArgs {
  const void *pred, *tgt;
  const float* wt;
  int64_t n;
  uint32_t HW;
  FastDiv fd_hw, fd_c;
  float eps, lw, gs_arg;
  const float* gs_dev;
  void *out, *grad;
  float* partial;
  unsigned al, grid;
  hipStream_t s;
};

template <int KIND, typename PT, typename TT, int WM>
void launch_loss(const LossArgs& a) {
  hipLaunchKernelGGL((pixel_loss_kernel<KIND, PT, TT, WM>), dim3(a.grid), dim3(PL_THREADS), 0, a.s, (const PT*)a.pred,
                     (const TT*)a.tgt, a.wt, a.n, a.HW, a.fd_hw, a.fd_c, a.eps, a.lw, a.gs_arg, a.gs_dev, (PT*)a.out,
                     (PT*)a.grad, a.partial, a.al);
}
template <int KIND, typename PT, typename TT>
void launch_loss_w(const LossArgs& a, int wm) {
  if (wm == 0) launch_loss<KIND, PT, TT, 0>(a);
  else if (wm == 1) launch_loss<KIND, PT, TT, 1>(a);
  else launch_loss<KIND, PT, TT, 2>(a);
}
template <int KIND>
void launch_loss_t(const LossArgs& a, int pdt, int tdt, int wm) {
  if (pdt == SR_F32) launch_loss_w<KIND, float, float>(a, wm);
  else if (tdt == SR_F32) launch_loss_w<KIND, bf16_t, float>(a, wm);
  else launch_loss_w<KIND, bf16_t, bf16_t>(a, wm);
}

}  // namespace

extern "C" {

size_t sr_pixel_loss_workspace(int64_t n) {
  (void)n;
  return PL_HEAD_BYTES + 2 * PL_MAX_BLOCKS * sizeof(float);
}

int sr_pixel_loss(int kind, int reduction, int pred_dtype, int target_dtype, const void* pred, const void* target,
                  const float* weight, int weight_channels, int N, int C, int H, int W, float loss_weight, float eps,
                  float* loss, void* out, void* grad, void* workspace, size_t ws_bytes, void* stream) {
  if (!pred || !target || !workspace || N <= 0 || C <= 0 || H <= 0 || W <= 0)
    return sr_fail(SR_EINVAL, "pixel_loss: bad arguments");
  if (kind != SR_LOSS_L1 && kind != SR_LOSS_MSE && kind != SR_LOSS_CHARBONNIER)
    return sr_fail(SR_EINVAL, "pixel_loss: unknown loss kind");
  if (reduction != SR_REDUCE_NONE && reduction != SR_REDUCE_MEAN && reduction != SR_REDUCE_SUM)
    return sr_fail(SR_EINVAL, "pixel_loss: unknown reduction");
  if ((pred_dtype != SR_F32 && pred_dtype != SR_BF16) || (target_dtype != SR_F32 && target_dtype != pred_dtype))
    return sr_fail(SR_EINVAL, "pixel_loss: pred must be fp32 or bf16, target fp32 or pred's dtype");
  if (weight ? (weight_channels != 1 && weight_channels != C) : weight_channels != 0)
    return sr_fail(SR_EINVAL, "pixel_loss: the weight map has 1 or C channels (0 without a map)");
  if (reduction == SR_REDUCE_NONE ? !out : !loss)
    return sr_fail(SR_EINVAL, "pixel_loss: reduction 'none' needs out, 'mean' / 'sum' need loss");
  if (ws_bytes < sr_pixel_loss_workspace(0)) return sr_fail(SR_EINVAL, "pixel_loss: workspace too small");
  if ((uintptr_t)workspace & 7) return sr_fail(SR_EINVAL, "pixel_loss: workspace must be 8-byte aligned");
  const int psize = pred_dtype == SR_BF16 ? 2 : 4, tsize = target_dtype == SR_BF16 ? 2 : 4;
  if ((((uintptr_t)pred | (uintptr_t)out | (uintptr_t)grad) & (psize - 1)) || ((uintptr_t)target & (tsize - 1)) ||
      (((uintptr_t)weight | (uintptr_t)loss) & 3))
    return sr_fail(SR_EINVAL, "pixel_loss: tensors must be element-aligned");
  const int64_t HW = (int64_t)H * W, n = (int64_t)N * C * HW;
  if (n >= 0xffffffffll - 8) return sr_fail(SR_ETOOBIG, "pixel_loss: tensor too large");

  hipStream_t s = (hipStream_t)stream;
  double* denom_dev = (double*)workspace;
  float* gs_dev = (float*)((char*)workspace + 8);
  float* part_loss = (float*)((char*)workspace + PL_HEAD_BYTES);
  float* part_w = part_loss + PL_MAX_BLOCKS;
  const int wm = !weight ? 0 : (weight_channels == 1 && C > 1 ? 1 : 2);
  const bool wmean = weight && reduction == SR_REDUCE_MEAN;
  if (wmean) {
    const int64_t nw = (int64_t)N * weight_channels * HW;
    const unsigned gw = loss_grid((nw + 3) / 4);
    hipLaunchKernelGGL(wsum_partial_kernel, dim3(gw), dim3(PL_THREADS), 0, s, weight, nw, ((uintptr_t)weight & 15) == 0,
                       part_w);
    hipLaunchKernelGGL(wsum_final_kernel, dim3(1), dim3(PL_THREADS), 0, s, (const float*)part_w, (int)gw,
                       (double)(C / weight_channels), (double)loss_weight, denom_dev, gs_dev);
  }
  const int V = 16 / psize;
  const double denom = reduction == SR_REDUCE_MEAN ? (double)n : 1.0;
  LossArgs a;
  a.pred = pred, a.tgt = target, a.wt = weight, a.n = n, a.HW = (uint32_t)HW;
  a.fd_hw = make_fastdiv((uint32_t)HW), a.fd_c = make_fastdiv((uint32_t)C);
  a.eps = eps, a.lw = loss_weight, a.gs_arg = (float)((double)loss_weight / denom), a.gs_dev = wmean ? gs_dev : nullptr;
  a.out = reduction == SR_REDUCE_NONE ? out : nullptr, a.grad = grad, a.partial = part_loss;
  a.al = (((uintptr_t)pred & 15) ? 0 : AL_PRED) | (((uintptr_t)target & 15) ? 0 : AL_TGT) |
         (((uintptr_t)weight & 15) ? 0 : AL_W) | (((uintptr_t)out & 15) ? 0 : AL_OUT) |
         (((uintptr_t)grad & 15) ? 0 : AL_GRAD);
  a.grid = loss_grid((n + V - 1) / V), a.s = s;
  if (kind == SR_LOSS_L1) launch_loss_t<SR_LOSS_L1>(a, pred_dtype, target_dtype, wm);
  else if (kind == SR_LOSS_MSE) launch_loss_t<SR_LOSS_MSE>(a, pred_dtype, target_dtype, wm);
  else launch_loss_t<SR_LOSS_CHARBONNIER>(a, pred_dtype, target_dtype, wm);
  if (reduction != SR_REDUCE_NONE)
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(PL_THREADS), 0, s, (const float*)part_loss, (int)a.grid,
                       (double)loss_weight, denom, wmean ? (const double*)denom_dev : nullptr, loss);
  return sr_check(hipGetLastError(), "pixel_loss launch");
}

size_t sr_gan_loss_workspace(int64_t n) {
  (void)n;
  return PL_MAX_BLOCKS * sizeof(float);
}

int sr_gan_loss_block(int pred_dtype) { return PL_THREADS * (pred_dtype == SR_BF16 ? 8 : 4); }

int sr_gan_loss(int kind, int pred_dtype, const void* pred, int64_t n, float target_val, int target_is_real, int is_disc,
                float loss_weight, float* loss, void* grad, void* workspace, size_t ws_bytes, void* stream) {
  if (!pred || !loss || !workspace || n <= 0) return sr_fail(SR_EINVAL, "gan_loss: bad arguments");
  if (kind < SR_GAN_VANILLA || kind > SR_GAN_HINGE) return sr_fail(SR_EINVAL, "gan_loss: unknown kind");
  if (pred_dtype != SR_F32 && pred_dtype != SR_BF16) return sr_fail(SR_EINVAL, "gan_loss: pred must be fp32 or bf16");
  if (ws_bytes < sr_gan_loss_workspace(n)) return sr_fail(SR_EINVAL, "gan_loss: workspace too small");
  const int psize = pred_dtype == SR_BF16 ? 2 : 4;
  if ((((uintptr_t)pred | (uintptr_t)grad) & (psize - 1)) || (((uintptr_t)loss | (uintptr_t)workspace) & 3))
    return sr_fail(SR_EINVAL, "gan_loss: tensors must be element-aligned");
  if (n >= 0xffffffffll - 8) return sr_fail(SR_ETOOBIG, "gan_loss: tensor too large");
  // loss_weight is for generators only (gan_loss.py:111-112)
  const double lw = is_disc ? 1.0 : (double)loss_weight;
  const float gs = (float)(lw / (double)n);
  const float sg_real = target_is_real ? -1.f : 1.f;
  const int V = 16 / psize;
  const unsigned grid = loss_grid((n + V - 1) / V);
  const unsigned al = (((uintptr_t)pred & 15) ? 0 : AL_PRED) | (((uintptr_t)grad & 15) ? 0 : AL_GRAD);
  float* partial = (float*)workspace;
  hipStream_t s = (hipStream_t)stream;
  if (kind == SR_GAN_VANILLA) launch_gan<0>(pred_dtype, grid, s, pred, n, target_val, 0.f, gs, grad, partial, al);
  else if (kind == SR_GAN_LSGAN) launch_gan<1>(pred_dtype, grid, s, pred, n, target_val, 0.f, gs, grad, partial, al);
  else if (kind == SR_GAN_WGAN) launch_gan<2>(pred_dtype, grid, s, pred, n, 0.f, sg_real, gs, grad, partial, al);
  else if (kind == SR_GAN_WGAN_SOFTPLUS) launch_gan<3>(pred_dtype, grid, s, pred, n, 0.f, sg_real, gs, grad, partial, al);
  else if (is_disc) launch_gan<4>(pred_dtype, grid, s, pred, n, 0.f, sg_real, gs, grad, partial, al);
  else launch_gan<2>(pred_dtype, grid, s, pred, n, 0.f, -1.f, gs, grad, partial, al);  // hinge generator: -mean(x)
  hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(PL_THREADS), 0, s, (const float*)partial, (int)grid, lw, (double)n,
                     (const double*)nullptr, loss);
  return sr_check(hipGetLastError(), "gan_loss launch");
}

}  // extern "C"
