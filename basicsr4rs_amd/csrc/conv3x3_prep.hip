// Weight images of the conv / linear GEMMs: prep_kernel and prep_batch_kernel build the padded forward rows,
// the flipped transposed dgrad rows and the padded bias from an fp32 weight, one conv or a batch of them per
// launch; the sr_conv_prep_* / sr_conv3x3_prep entry points launch them.
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

// One element (n, ci, tap) of the padded GEMM images of a conv / linear weight (and, for i <
// Cout, its bias entry): wf [Cout][taps*Cin] forward rows, wd [Cin][taps*Cout] the flipped
// transposed dgrad rows; row_map / col_map (or the PixelShuffle permutation) give the source
// output / input channel of each padded row / column (-1: zero padding).
template <typename T>
SR_DEV void prep_elem(const float* w, const float* bias, int Cout_real, int Cin_real, int Cout, int Cin, int out_ps,
                      int taps, const int* row_map, const int* col_map, T* wf, T* wd, float* bias_g, int64_t i) {
  const int64_t total = (int64_t)Cout * Cin * taps;
  const int r2 = out_ps > 0 ? out_ps * out_ps : 1;
  const int cps = Cout_real / r2;
  auto row_of = [&](int n) -> int {
    if (row_map) return row_map[n];
    if (n >= Cout_real) return -1;
    return out_ps > 0 ? (n % cps) * r2 + n / cps : n;
  };
  if (i < total) {
    const int tap = (int)(i % taps);
    const int ci = (int)((i / taps) % Cin);
    const int n = (int)(i / ((int64_t)taps * Cin));
    const int co = row_of(n);
    const int cs = col_map ? col_map[ci] : (ci < Cin_real ? ci : -1);
    float v = 0.f;
    if (co >= 0 && cs >= 0) v = w[((size_t)co * Cin_real + cs) * taps + tap];
    if (wf) wf[(size_t)n * taps * Cin + (size_t)tap * Cin + ci] = Elt<T>::from_f(v);
    if (wd) wd[(size_t)ci * taps * Cout + (size_t)(taps - 1 - tap) * Cout + n] = Elt<T>::from_f(v);
  }
  if (bias_g && i < Cout) {
    const int n = (int)i;
    const int co = row_of(n);
    bias_g[n] = (co >= 0 && bias) ? bias[co] : 0.f;
  }
}

template <typename T>
__global__ void prep_kernel(const float* w, const float* bias, int Cout_real, int Cin_real, int Cout, int Cin,
                            int out_ps, int taps, const int* row_map, const int* col_map, T* wf, T* wd,
                            float* bias_g) {
  prep_elem<T>(w, bias, Cout_real, Cin_real, Cout, Cin, out_ps, taps, row_map, col_map, wf, wd, bias_g,
               (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// All of a net's cached GEMM images in one launch (after an optimizer step): block b belongs
// to the item whose [block_start[k], block_start[k+1]) range holds it, and owns a 32 (GEMM row n)
// x 32 (channel ci) tile of it, all taps.  The tile is read coalesced along (ci, tap) -- the
// fp32 [Cout][Cin][taps] layout -- into LDS, then written as 64-B runs along ci (wf rows) and
// along n (wd rows), instead of one scattered 2-B store per element per image.
constexpr int PREP_T = 32;
template <typename T>
__global__ __launch_bounds__(256) void prep_batch_kernel(const sr_prep_item* __restrict__ items,
                                                         const int* __restrict__ block_start, int n) {
  __shared__ float tile[PREP_T][9][PREP_T + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  int lo = 0, hi = n - 1;  // last k with block_start[k] <= b
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (block_start[mid] <= b) lo = mid; else hi = mid - 1;
  }
  const sr_prep_item it = items[lo];
  // ksize 5 / 7 / 9 (the k x k convs of convk.hip): the tile goes through LDS nine taps at a time
  const int taps_all = it.ksize == 1 ? 1 : (it.ksize > 3 ? it.ksize * it.ksize : 9);
  const int tci = (it.Cin + PREP_T - 1) / PREP_T;
  const int t = b - block_start[lo];
  const int n0 = (t / tci) * PREP_T, c0 = (t % tci) * PREP_T;
  const int r2 = it.out_ps > 0 ? it.out_ps * it.out_ps : 1;
  const int cps = it.Cout_real / r2;
  auto row_of = [&](int nn) -> int {
    if (it.row_map) return it.row_map[nn];
    if (nn >= it.Cout_real) return -1;
    return it.out_ps > 0 ? (nn % cps) * r2 + nn / cps : nn;
  };
  if (it.bias_g && c0 == 0 && tid < PREP_T) {
    const int nn = n0 + tid;
    if (nn < it.Cout) {
      const int co = row_of(nn);
      it.bias_g[nn] = (co >= 0 && it.bias) ? it.bias[co] : 0.f;
    }
  }
  T* wf = (T*)it.wf;
  T* wd = (T*)it.wd;
  for (int t0 = 0; t0 < taps_all; t0 += 9) {
    const int taps = taps_all - t0 < 9 ? taps_all - t0 : 9;  // taps t0 .. t0 + taps - 1 this pass
    if (t0) __syncthreads();
    const int per = PREP_T * taps;  // elements per GEMM row of the tile
    for (int idx = tid; idx < PREP_T * per; idx += 256) {
      const int nl = idx / per, rem = idx - nl * per;
      const int cil = rem / taps, tap = rem - cil * taps;
      const int nn = n0 + nl, ci = c0 + cil;
      float v = 0.f;
      if (nn < it.Cout && ci < it.Cin) {
        const int co = row_of(nn);
        const int cs = it.col_map ? it.col_map[ci] : (ci < it.Cin_real ? ci : -1);
        if (co >= 0 && cs >= 0) v = it.w[((size_t)co * it.Cin_real + cs) * taps_all + t0 + tap];
      }
      tile[nl][tap][cil] = v;
    }
    __syncthreads();
    if (Elt<T>::SIZE == 2 && it.Cin % 8 == 0 && it.Cout % 8 == 0) {
      // bf16: 8 consecutive GEMM-row elements per thread, one 16-B store (with Cin and Cout multiples of
      // 8 and the tile origins of 32, an 8-run lies wholly inside or outside the image; a pixel-shuffled
      // conv's Cout -- 27 at x3 -- takes the element loop below); the 2-B stores of that loop ran at
      // ~1.5 TB/s (EDSR: 227 us per step)
      constexpr int G8 = PREP_T / 8;
      for (int g = tid; g < PREP_T * taps * G8; g += 256) {
        const int a0 = g / (taps * G8), r = g - a0 * (taps * G8);
        const int tap = r / G8, e8 = (r - tap * G8) * 8;
        const int gt = t0 + tap;
        if (wf) {  // wf[n][tap][ci]: n = n0 + a0, ci = c0 + e8 ..
          const int nn = n0 + a0, ci = c0 + e8;
          if (nn < it.Cout && ci < it.Cin) {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(tile[a0][tap][e8 + 2 * j], tile[a0][tap][e8 + 2 * j + 1]);
            *(u32x4*)(wf + (size_t)nn * taps_all * it.Cin + (size_t)gt * it.Cin + ci) = o;
          }
        }
        if (wd) {  // wd[ci][taps - 1 - tap][n]: ci = c0 + a0, n = n0 + e8 ..
          const int ci = c0 + a0, nn = n0 + e8;
          if (nn < it.Cout && ci < it.Cin) {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(tile[e8 + 2 * j][tap][a0], tile[e8 + 2 * j + 1][tap][a0]);
            *(u32x4*)(wd + (size_t)ci * taps_all * it.Cout + (size_t)(taps_all - 1 - gt) * it.Cout + nn) = o;
          }
        }
      }
      continue;
    }
    for (int idx = tid; idx < PREP_T * per; idx += 256) {
      if (wf) {  // wf[n][tap][ci]: runs along ci
        const int nl = idx / per, rem = idx - nl * per;
        const int tap = rem / PREP_T, cil = rem - tap * PREP_T;
        const int nn = n0 + nl, ci = c0 + cil;
        if (nn < it.Cout && ci < it.Cin)
          wf[(size_t)nn * taps_all * it.Cin + (size_t)(t0 + tap) * it.Cin + ci] = Elt<T>::from_f(tile[nl][tap][cil]);
      }
      if (wd) {  // wd[ci][taps - 1 - tap][n]: runs along n
        const int cil = idx / per, rem = idx - cil * per;
        const int tap = rem / PREP_T, nl = rem - tap * PREP_T;
        const int nn = n0 + nl, ci = c0 + cil;
        if (nn < it.Cout && ci < it.Cin)
          wd[(size_t)ci * taps_all * it.Cout + (size_t)(taps_all - 1 - t0 - tap) * it.Cout + nn] =
              Elt<T>::from_f(tile[nl][tap][cil]);
      }
    }
  }
}

}  // namespace

extern "C" {

int sr_conv_prep_mapped(int dtype, int ksize, const float* w, const float* bias, int Cout_real, int Cin_real,
                        int Cout, int Cin, int out_ps, const int* row_map, const int* col_map, void* wf, void* wd,
                        float* bias_g, void* stream) {
  if (!w) return sr_fail(SR_EINVAL, "conv_prep: null weight");
  if (ksize != 1 && ksize != 3 && ksize != 5 && ksize != 7 && ksize != 9)
    return sr_fail(SR_EINVAL, "conv_prep: ksize must be 1, 3, 5, 7 or 9");
  if ((!row_map && Cout < Cout_real) || (!col_map && Cin < Cin_real)) return sr_fail(SR_EINVAL, "conv_prep: padded < real");
  if (out_ps > 0 && (Cout_real % (out_ps * out_ps) || Cout != Cout_real || row_map))
    return sr_fail(SR_EINVAL, "conv_prep: shuffled conv needs Cout == Cout_real divisible by r^2");
  const int taps = ksize * ksize;
  const int64_t total = (int64_t)Cout * Cin * taps;
  const int64_t work = total > Cout ? total : Cout;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(prep_kernel<bf16_t>, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, w, bias, Cout_real,
                       Cin_real, Cout, Cin, out_ps, taps, row_map, col_map, (bf16_t*)wf, (bf16_t*)wd, bias_g);
  else
    hipLaunchKernelGGL(prep_kernel<float>, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, w, bias, Cout_real,
                       Cin_real, Cout, Cin, out_ps, taps, row_map, col_map, (float*)wf, (float*)wd, bias_g);
  return sr_check(hipGetLastError(), "conv_prep launch");
}

int sr_conv_prep_blocks(const sr_prep_item* it) {
  return ((it->Cout + PREP_T - 1) / PREP_T) * ((it->Cin + PREP_T - 1) / PREP_T);
}

int sr_conv_prep_batch(int dtype, const sr_prep_item* items, const int* block_start, int n, int total_blocks,
                       void* stream) {
  if (!items || !block_start || n <= 0 || total_blocks <= 0) return sr_fail(SR_EINVAL, "conv_prep_batch: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(prep_batch_kernel<bf16_t>, dim3(total_blocks), dim3(256), 0, s, items, block_start, n);
  else
    hipLaunchKernelGGL(prep_batch_kernel<float>, dim3(total_blocks), dim3(256), 0, s, items, block_start, n);
  return sr_check(hipGetLastError(), "conv_prep_batch launch");
}

int sr_conv3x3_prep(int dtype, const float* w, const float* bias, int Cout_real, int Cin_real, int Cout, int Cin,
                    int out_ps, void* wf, void* wd, float* bias_g, void* stream) {
  return sr_conv_prep_mapped(dtype, 3, w, bias, Cout_real, Cin_real, Cout, Cin, out_ps, nullptr, nullptr, wf, wd,
                             bias_g, stream);
}

}  // extern "C"
