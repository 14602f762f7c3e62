// ECBSR (basicsr/archs/ecbsr_arch.py) trained on its collapsed form.  An ECB block is five parallel branches
// (3x3; 1x1 -> 3x3; 1x1 -> Sobel-x / Sobel-y / Laplacian, every 1x1 output padded with its own bias) whose sum
// is exactly one 3x3 convolution.  Here the train step runs that one convolution per layer:
//
//   sr_ecb_rep_fwd   all blocks of a net in one launch: the collapsed fp32 weight RK [Cout][Cin][3][3] and bias
//                    RB [Cout] from the block's parameters, and their GEMM images (forward rows, flipped
//                    transposed input-gradient rows, padded bias) in the feature dtype; bf16 rows carry
//                    RK as hi + lo, [hi taps 0..8][lo taps 0..8], and the conv walks the nine taps twice.
//   sr_ecb_conv      3x3 conv on narrow NHWC maps (padded channels <= 64) with three epilogues: per-channel
//                    PReLU (y and the pre-activation z stored), the network tail (shortcut + PixelShuffle into
//                    fp32 NCHW) and the input gradient gated by the producer's z, with per-block partial sums
//                    of g * min(z, 0) for the slope gradient.
//   sr_ecb_da_reduce the slope gradients of all layers from those partials, in a fixed order.
//   sr_ecb_tail_bwd  fp32 NCHW dOut -> the NHWC dz of the last block (pixel-unshuffle).
//   sr_ecb_rep_bwd   the transpose of sr_ecb_rep_fwd: dRK / dRB of all blocks -> the gradients of their 18
//                    trainable tensors, one launch, every output element owned by one thread (no atomics).
//
// The conv kernel is convk_fwd_kernel (convk.hip) with k = 3: a block of 4 waves stages a pixel tile and its
// halo of one image in LDS (zeros outside the image), the weight rows are the MFMA A operand, the LDS halo the
// B operand; v_mfma_f32_16x16x32_bf16 for bf16 maps and the exact v_mfma_f32_16x16x4_f32 for fp32.
#include "sr_common.h"
#include "sr_internal.h"

namespace {

constexpr int kEcbMaxMid = 256;  // one thread per mid channel in the bias reduction
constexpr int kEcbMaxCh = 64;

// ------------------------------------------------------------------------------------------------
// Collapse.  Grid (max Cout_p, L): block (o, l) owns output channel o of ECB block l.
//   RK[o][i][t] = W3 + sum_m k1[o][m][t] k0[m][i] + sum_e (scale_e[o] mask_e[o][t]) k0_e[o][i] + idt
//   RB[o] = b3 + (sum_m (sum_t k1[o][m][t]) b0[m] + b1) + sum_e ((scale_e[o] sum_t mask_e[o][t]) b0_e[o] + bias_e[o])
// fp32, fixed order: the m sum is serial per element, the bias sum a fixed tree over 256 lanes.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ecb_rep_fwd_kernel(const sr_ecb_block* tab) {
  __shared__ float red[256];
  const sr_ecb_block b = tab[blockIdx.y];
  const int o = blockIdx.x, tid = threadIdx.x;
  if (o >= b.Cout_p) return;
  const int Cin = b.Cin, Cout = b.Cout, Cin_p = b.Cin_p, Cout_p = b.Cout_p, mid = b.mid;
  T* wf = (T*)b.wf;
  T* wd = (T*)b.wd;
  const bool real = o < Cout;
  // bf16 images carry RK as hi + lo (two bf16 terms, nine more "taps"): the collapsed weight is no bf16 number even
  // when every parameter is, and its rounding would flip PReLU gates that the reference's five branches do not
  constexpr int NP = Elt<T>::SIZE == 2 ? 2 : 1;
  for (int idx = tid; idx < 9 * Cin_p; idx += 256) {
    const int t = idx / Cin_p, ci = idx - t * Cin_p;
    float v = 0.f;
    if (real && ci < Cin) {
      float s = 0.f;
      for (int m = 0; m < mid; ++m) s = fmaf(b.k1[((size_t)o * mid + m) * 9 + t], b.k0[(size_t)m * Cin + ci], s);
      v = b.w3[((size_t)o * Cin + ci) * 9 + t] + s;
#pragma unroll
      for (int e = 0; e < 3; ++e) v += (b.escale[e][o] * b.emask[e][o * 9 + t]) * b.ek0[e][(size_t)o * Cin + ci];
      if (b.with_idt && ci == o && t == 4) v += 1.f;
      b.rk[((size_t)o * Cin + ci) * 9 + t] = v;
    }
    // padded rows and columns: exactly zero
    const T hi = Elt<T>::from_f(v);
    wf[(size_t)o * NP * 9 * Cin_p + idx] = hi;
    wd[(size_t)ci * NP * 9 * Cout_p + (size_t)(8 - t) * Cout_p + o] = hi;
    if constexpr (NP == 2) {
      const T lo = Elt<T>::from_f(v - Elt<T>::to_f(hi));
      wf[(size_t)o * 18 * Cin_p + 9 * Cin_p + idx] = lo;
      wd[(size_t)ci * 18 * Cout_p + (size_t)(9 + 8 - t) * Cout_p + o] = lo;
    }
  }
  float p = 0.f;
  if (real && tid < mid) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) s += b.k1[((size_t)o * mid + tid) * 9 + t];
    p = s * b.b0[tid];
  }
  red[tid] = p;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  if (tid == 0) {
    float v = 0.f;
    if (real) {
      v = b.b3[o] + (red[0] + b.b1[o]);
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        float ms = 0.f;  // the mask taps first, then the product
#pragma unroll
        for (int t = 0; t < 9; ++t) ms += b.emask[e][o * 9 + t];
        v += (b.escale[e][o] * ms) * b.eb0[e][o] + b.ebias[e][o];
      }
      b.rb[o] = v;
    }
    b.bias_g[o] = v;
  }
}

// ------------------------------------------------------------------------------------------------
// Transpose of the collapse.  Grid (max Cout + mid, L): unit u < Cout owns everything indexed by output
// channel o = u (dW3[o], db3, db1, dk1[o], and row o of the edge branches); unit Cout + m owns dk0[m] and db0[m]
// of the 1x1 -> 3x3 branch.  Every gradient element is written by exactly one thread.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ecb_rep_bwd_kernel(const sr_ecb_block* tab, int accumulate) {
  const sr_ecb_block b = tab[blockIdx.y];
  const int u = blockIdx.x, tid = threadIdx.x;
  const int Cin = b.Cin, Cout = b.Cout, mid = b.mid;
  auto put = [&](float* p, float v) { *p = accumulate ? *p + v : v; };
  if (u < Cout) {
    const int o = u;
    const float* drk = b.drk + (size_t)o * Cin * 9;
    const float drb = b.drb[o];
    for (int idx = tid; idx < Cin * 9; idx += 256) put(b.g_w3 + (size_t)o * Cin * 9 + idx, drk[idx]);
    for (int idx = tid; idx < mid * 9; idx += 256) {
      const int m = idx / 9, t = idx - m * 9;
      float s = 0.f;
      for (int i = 0; i < Cin; ++i) s = fmaf(drk[i * 9 + t], b.k0[(size_t)m * Cin + i], s);
      put(b.g_k1 + (size_t)o * mid * 9 + idx, s + drb * b.b0[m]);
    }
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float sc = b.escale[e][o];
      const float* mk = b.emask[e] + o * 9;
      for (int i = tid; i < Cin; i += 256) {
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) s = fmaf(mk[t], drk[i * 9 + t], s);
        put(b.g_ek0[e] + (size_t)o * Cin + i, sc * s);
      }
      if (tid == 64 + e) {  // the scalars of branch e, one lane each
        float ms = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) ms += mk[t];
        float s = 0.f;
        for (int i = 0; i < Cin; ++i) {
          float q = 0.f;
#pragma unroll
          for (int t = 0; t < 9; ++t) q = fmaf(drk[i * 9 + t], mk[t], q);
          s = fmaf(q, b.ek0[e][(size_t)o * Cin + i], s);
        }
        put(b.g_escale[e] + o, s + (drb * ms) * b.eb0[e][o]);
        put(b.g_eb0[e] + o, (sc * ms) * drb);
        put(b.g_ebias[e] + o, drb);
      }
    }
    if (tid == 0) {
      put(b.g_b3 + o, drb);
      put(b.g_b1 + o, drb);
    }
  } else if (u < Cout + mid) {
    const int m = u - Cout;
    for (int i = tid; i < Cin; i += 256) {
      float s = 0.f;
      for (int o = 0; o < Cout; ++o)
#pragma unroll
        for (int t = 0; t < 9; ++t) s = fmaf(b.drk[((size_t)o * Cin + i) * 9 + t], b.k1[((size_t)o * mid + m) * 9 + t], s);
      put(b.g_k0 + (size_t)m * Cin + i, s);
    }
    if (tid == 64) {
      float s = 0.f;
      for (int o = 0; o < Cout; ++o) {
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < 9; ++t) q += b.k1[((size_t)o * mid + m) * 9 + t];
        s = fmaf(b.drb[o], q, s);
      }
      put(b.g_b0 + m, s);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The conv.  MODE 0: PReLU / ReLU / linear forward; 1: network tail; 2: gated input gradient.
// ------------------------------------------------------------------------------------------------
struct EcbConvArgs {
  const char* x;
  const char* w;
  const float* bias;   // GEMM-order bias [Cout] (padded entries zero) or null
  const float* slope;  // per-channel slopes [Cout_real] or null (linear)
  char* y;             // modes 0 / 2: the NHWC output
  char* z;             // mode 0: the pre-activation (written, may be null); mode 2: the producer's z (read)
  float* parts;        // mode 2: [blocks][64] partial sums of g * min(z, 0), or null
  const float* img;    // mode 1: the fp32 NCHW input image [N][img_c][H][W]
  float* out;          // mode 1: the fp32 NCHW output [N][Cout_real / ps^2][H ps][W ps]
  int ps, img_c;
  int N, H, W, Cin, Cout, Cout_real;
  int tiles_x, tiles_y;
  int pstride, cpp, nchunk, ldw;
};

template <typename T, int PT, int TWT, int MODE>
__global__ __launch_bounds__(256) void ecb_conv_kernel(const EcbConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  __shared__ float wred[4][kEcbMaxCh];
  constexpr int SZ = Elt<T>::SIZE;
  constexpr int TW = 16 * TWT, RW = PT / TWT, TH = 4 * RW;
  constexpr int HWp = TW + 2, HH = TH + 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  int b = blockIdx.x;
  const int tx = b % a.tiles_x;
  b /= a.tiles_x;
  const int ty = b % a.tiles_y;
  const int n = b / a.tiles_y;
  const int x0 = tx * TW, y0 = ty * TH;

  // the tile and its halo, zeros outside the image
  const int total = HH * HWp * a.cpp;
  for (int idx = tid; idx < total; idx += 256) {
    const int pix = idx / a.cpp, c = idx - pix * a.cpp;
    const int hy = pix / HWp, hx = pix - hy * HWp;
    const int gy = y0 + hy - 1, gx = x0 + hx - 1;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
      v = *(const u32x4*)(a.x + (((size_t)n * a.H + gy) * a.W + gx) * (size_t)(a.Cin * SZ) + (size_t)c * 16);
    *(u32x4*)(lds + (size_t)pix * a.pstride + c * 16) = v;
  }
  __syncthreads();

  f32x4 acc[4][PT];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int i = 0; i < PT; ++i) acc[ct][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int CT = (a.Cout + 15) >> 4;
  const size_t wrow = (size_t)a.ldw * SZ;

  if constexpr (SZ == 2) {
    // four 16-byte chunks (8 channels of one tap each) per MFMA: lane group g takes chunk 4 * step + g; the weight
    // row is [hi taps 0..8][lo taps 0..8], K = 18 Cin
    const int nsteps = (a.nchunk + 3) >> 2;
    int c = g % a.cpp, tap = g / a.cpp;
    int ky = (tap / 3) % 3, kx = tap % 3;
    for (int step = 0; step < nsteps; ++step) {
      const int kc = step * 4 + g;
      const bool valid = kc < a.nchunk;
      u32x4 fa[4], fb[PT];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int co = ct * 16 + l16;
        fa[ct] = u32x4{0u, 0u, 0u, 0u};
        if (ct < CT && valid && co < a.Cout) fa[ct] = *(const u32x4*)(a.w + (size_t)co * wrow + (size_t)kc * 16);
      }
#pragma unroll
      for (int i = 0; i < PT; ++i) {
        const int row = wave * RW + i / TWT, col = (i % TWT) * 16 + l16;
        fb[i] = u32x4{0u, 0u, 0u, 0u};  // a chunk past K multiplies nothing, not even a NaN
        if (valid) fb[i] = *(const u32x4*)(lds + (size_t)((row + ky) * HWp + col + kx) * a.pstride + c * 16);
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (ct < CT) {
#pragma unroll
          for (int i = 0; i < PT; ++i)
            acc[ct][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, fa[ct]),
                                                                 __builtin_bit_cast(s16x8, fb[i]), acc[ct][i], 0, 0, 0);
        }
      c += 4;  // this lane's chunk of the next step
      while (c >= a.cpp) {
        c -= a.cpp;
        if (++kx == 3) {
          kx = 0;
          if (++ky == 3) ky = 0;  // the lo half of the weight row walks the same nine taps again
        }
      }
    }
  } else {
    // exact f32: one chunk (4 channels of one tap) per v_mfma_f32_16x16x4_f32, lane group g its channel g
    int c = 0, kx = 0, ky = 0;
    for (int kc = 0; kc < a.nchunk; ++kc) {
      float fa[4], fb[PT];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int co = ct * 16 + l16;
        fa[ct] = 0.f;
        if (ct < CT && co < a.Cout) fa[ct] = *(const float*)(a.w + (size_t)co * wrow + (size_t)kc * 16 + g * 4);
      }
#pragma unroll
      for (int i = 0; i < PT; ++i) {
        const int row = wave * RW + i / TWT, col = (i % TWT) * 16 + l16;
        fb[i] = *(const float*)(lds + (size_t)((row + ky) * HWp + col + kx) * a.pstride + c * 16 + g * 4);
      }
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (ct < CT) {
#pragma unroll
          for (int i = 0; i < PT; ++i)
            acc[ct][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[ct], fb[i], acc[ct][i], 0, 0, 0);
        }
      if (++c == a.cpp) {
        c = 0;
        if (++kx == 3) {
          kx = 0;
          ++ky;
        }
      }
    }
  }

  // epilogue: lane = pixel l16 of tile i, output channels ct * 16 + 4 g .. + 3
  float psum[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) psum[ct][j] = 0.f;
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int gy = y0 + wave * RW + i / TWT, gx = x0 + (i % TWT) * 16 + l16;
    if (gy >= a.H || gx >= a.W) continue;
    const size_t pix = ((size_t)n * a.H + gy) * a.W + gx;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int co = ct * 16 + 4 * g;
      if (co >= a.Cout) continue;  // Cout is a multiple of 8: a lane's 4 channels are all in or all out
      if constexpr (MODE == 1) {
        const int s2 = a.ps * a.ps, Co = a.Cout_real / s2;
        const size_t Ws = (size_t)a.W * a.ps;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = co + j;
          if (q >= a.Cout_real) continue;
          const int ch = q / s2, r = q - ch * s2, ii = r / a.ps, jj = r - ii * a.ps;
          const float xin = a.img[(((size_t)n * a.img_c + (a.img_c == 1 ? 0 : ch)) * a.H + gy) * a.W + gx];
          a.out[(((size_t)n * Co + ch) * a.H * a.ps + (size_t)gy * a.ps + ii) * Ws + (size_t)gx * a.ps + jj] =
              acc[ct][i][j] + a.bias[q] + xin;
        }
      } else if constexpr (MODE == 0) {
        float zv[4], yv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool real = co + j < a.Cout_real;
          const float t = acc[ct][i][j] + (a.bias ? a.bias[co + j] : 0.f);
          const float sl = a.slope && real ? a.slope[co + j] : 1.f;
          zv[j] = real ? t : 0.f;  // padded channels: exactly zero
          yv[j] = real ? (t > 0.f ? t : sl * t) : 0.f;
        }
        if constexpr (SZ == 2) {
          *(u32x2*)(a.y + pix * (size_t)(a.Cout * 2) + co * 2) = u32x2{pack_bf16x2(yv[0], yv[1]), pack_bf16x2(yv[2], yv[3])};
          if (a.z)
            *(u32x2*)(a.z + pix * (size_t)(a.Cout * 2) + co * 2) =
                u32x2{pack_bf16x2(zv[0], zv[1]), pack_bf16x2(zv[2], zv[3])};
        } else {
          *(f32x4*)(a.y + pix * (size_t)(a.Cout * 4) + co * 4) = f32x4{yv[0], yv[1], yv[2], yv[3]};
          if (a.z) *(f32x4*)(a.z + pix * (size_t)(a.Cout * 4) + co * 4) = f32x4{zv[0], zv[1], zv[2], zv[3]};
        }
      } else {
        float zv[4] = {1.f, 1.f, 1.f, 1.f}, dv[4];
        if (a.z) {
          if constexpr (SZ == 2) {
            const u32x2 zz = *(const u32x2*)(a.z + pix * (size_t)(a.Cout * 2) + co * 2);
            zv[0] = bf16_to_f32((unsigned short)(zz[0] & 0xffffu)), zv[1] = bf16_to_f32((unsigned short)(zz[0] >> 16));
            zv[2] = bf16_to_f32((unsigned short)(zz[1] & 0xffffu)), zv[3] = bf16_to_f32((unsigned short)(zz[1] >> 16));
          } else {
            const f32x4 zz = *(const f32x4*)(a.z + pix * (size_t)(a.Cout * 4) + co * 4);
            zv[0] = zz[0], zv[1] = zz[1], zv[2] = zz[2], zv[3] = zz[3];
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool real = co + j < a.Cout_real;
          const float gr = acc[ct][i][j];
          const float sl = a.slope && real ? a.slope[co + j] : 1.f;
          // the gate of torch's PReLU backward: 1 where z > 0, else the slope (also at z == 0)
          dv[j] = real ? (zv[j] > 0.f ? gr : sl * gr) : 0.f;
          if (real) psum[ct][j] += gr * fminf(zv[j], 0.f);
        }
        if constexpr (SZ == 2) {
          *(u32x2*)(a.y + pix * (size_t)(a.Cout * 2) + co * 2) = u32x2{pack_bf16x2(dv[0], dv[1]), pack_bf16x2(dv[2], dv[3])};
        } else {
          *(f32x4*)(a.y + pix * (size_t)(a.Cout * 4) + co * 4) = f32x4{dv[0], dv[1], dv[2], dv[3]};
        }
      }
    }
  }
  if constexpr (MODE == 2) {
    if (a.parts) {  // block-uniform
      // over the 16 pixels of a lane group (the same butterfly in every lane), then over the 4 waves in order
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = psum[ct][j];
          v += __shfl_xor(v, 1);
          v += __shfl_xor(v, 2);
          v += __shfl_xor(v, 4);
          v += __shfl_xor(v, 8);
          if (l16 == 0) wred[wave][ct * 16 + 4 * g + j] = v;
        }
      __syncthreads();
      if (tid < kEcbMaxCh)
        a.parts[(size_t)blockIdx.x * kEcbMaxCh + tid] = ((wred[0][tid] + wred[1][tid]) + wred[2][tid]) + wred[3][tid];
    }
  }
}

// da[c] (+)= sum over the blocks' partials of layer l; grid (layers), thread (c, part q of 16): part q sums blocks
// q, q + 16, ... and the sixteen parts are added in order
constexpr int kDaParts = 16;
__global__ __launch_bounds__(64 * kDaParts) void ecb_da_reduce_kernel(const sr_ecb_block* tab, const float* parts,
                                                                      int nblocks, int accumulate) {
  __shared__ float red[kDaParts][kEcbMaxCh];
  const sr_ecb_block b = tab[blockIdx.x];
  const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
  const float* src = parts + (size_t)blockIdx.x * nblocks * kEcbMaxCh;
  float s = 0.f;
  for (int i = q; i < nblocks; i += kDaParts) s += src[(size_t)i * kEcbMaxCh + c];
  red[q][c] = s;
  __syncthreads();
  if (q == 0 && b.g_act && c < b.Cout) {
    float v = red[0][c];
#pragma unroll
    for (int k = 1; k < kDaParts; ++k) v += red[k][c];
    b.g_act[c] = accumulate ? b.g_act[c] + v : v;
  }
}

// dz[n][h][w][q] = dOut[n][q / s^2][h s + i][w s + j] (q < C s^2; padded channels zero)
template <typename T>
__global__ void ecb_tail_bwd_kernel(const float* __restrict__ dout, int N, int C, int H, int W, int s, int Cp,
                                    T* __restrict__ dz) {
  const int64_t total = (int64_t)N * H * W * Cp;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int q = (int)(idx % Cp);
  int64_t p = idx / Cp;
  const int w = (int)(p % W);
  p /= W;
  const int h = (int)(p % H);
  const int n = (int)(p / H);
  float v = 0.f;
  const int s2 = s * s;
  if (q < C * s2) {
    const int ch = q / s2, r = q - ch * s2, i = r / s, j = r - i * s;
    v = dout[(((size_t)n * C + ch) * H * s + (size_t)h * s + i) * ((size_t)W * s) + (size_t)w * s + j];
  }
  dz[idx] = Elt<T>::from_f(v);
}

int ecb_pixel_stride(int channels, int size) {
  const int b = channels * size;
  return b % 64 == 0 ? b + 16 : b;
}

const char* ecb_conv_check(const sr_ecb_conv_desc* d) {
  if (d->dtype != SR_F32 && d->dtype != SR_BF16) return "ecb_conv: dtype must be SR_F32 or SR_BF16";
  if (d->mode < 0 || d->mode > 2) return "ecb_conv: mode must be 0 (activated), 1 (tail) or 2 (gated input gradient)";
  if (d->N < 1 || d->H < 1 || d->W < 1) return "ecb_conv: N, H, W must be >= 1";
  if (d->Cin < 8 || d->Cout < 8 || d->Cin % 8 || d->Cout % 8) return "ecb_conv: channel counts must be multiples of 8";
  if (d->Cin > kEcbMaxCh || d->Cout > kEcbMaxCh) return "ecb_conv: padded channel counts above 64 are not supported";
  if (d->Cout_real < 1 || d->Cout_real > d->Cout) return "ecb_conv: real channel count must be in 1 .. padded";
  if (d->mode == 1) {
    if (d->ps < 1 || d->Cout_real % (d->ps * d->ps)) return "ecb_conv: tail needs Cout_real = channels * ps^2";
    if (d->img_c != 1 && d->img_c != d->Cout_real / (d->ps * d->ps))
      return "ecb_conv: tail shortcut needs 1 image channel or as many as the output";
    if ((int64_t)d->H * d->ps > 0x7fffffff || (int64_t)d->W * d->ps > 0x7fffffff) return "ecb_conv: output too large";
  }
  return nullptr;
}

template <int PT, int TWT>
int64_t ecb_conv_tiles(const sr_ecb_conv_desc* d) {
  constexpr int TW = 16 * TWT, TH = 4 * PT / TWT;
  return (int64_t)((d->W + TW - 1) / TW) * ((d->H + TH - 1) / TH) * d->N;
}

template <typename T, int PT, int TWT, int MODE>
int launch_ecb_conv(const sr_ecb_conv_desc* d, EcbConvArgs a, hipStream_t s) {
  constexpr int TW = 16 * TWT, TH = 4 * PT / TWT;
  a.N = d->N, a.H = d->H, a.W = d->W, a.Cin = d->Cin, a.Cout = d->Cout, a.Cout_real = d->Cout_real;
  a.ps = d->ps, a.img_c = d->img_c;
  a.tiles_x = (d->W + TW - 1) / TW;
  a.tiles_y = (d->H + TH - 1) / TH;
  a.pstride = ecb_pixel_stride(d->Cin, Elt<T>::SIZE);
  a.cpp = d->Cin / Elt<T>::PER16;
  constexpr int NP = Elt<T>::SIZE == 2 ? 2 : 1;  // bf16 weight rows: hi and lo halves
  a.nchunk = NP * 9 * a.cpp;
  a.ldw = NP * 9 * d->Cin;
  const int64_t blocks = ecb_conv_tiles<PT, TWT>(d);
  if (blocks > 0x7fffffff) return sr_fail(SR_ETOOBIG, "ecb_conv: too many tiles");
  const size_t lds = (size_t)(TH + 2) * (TW + 2) * a.pstride;  // at most 10 x 34 x 144 B
  hipLaunchKernelGGL((ecb_conv_kernel<T, PT, TWT, MODE>), dim3((unsigned)blocks), dim3(256), lds, s, a);
  return sr_check(hipGetLastError(), "ecb_conv launch");
}

template <typename T, int PT, int TWT>
int launch_ecb_conv_mode(const sr_ecb_conv_desc* d, const EcbConvArgs& a, hipStream_t s) {
  if (d->mode == 0) return launch_ecb_conv<T, PT, TWT, 0>(d, a, s);
  if (d->mode == 1) return launch_ecb_conv<T, PT, TWT, 1>(d, a, s);
  return launch_ecb_conv<T, PT, TWT, 2>(d, a, s);
}

}  // namespace

extern "C" {

int sr_ecb_table_check(const sr_ecb_block* host_table, int L) {
  if (!host_table || L < 1) return sr_fail(SR_EINVAL, "ecb_table_check: null table or no blocks");
  for (int l = 0; l < L; ++l) {
    const sr_ecb_block& b = host_table[l];
    if (b.Cin < 1 || b.Cout < 1 || b.Cin > kEcbMaxCh || b.Cout > kEcbMaxCh)
      return sr_fail(SR_EINVAL, "ecb_table_check: channel counts must be in 1 .. 64");
    if (b.Cin_p != (b.Cin + 7) / 8 * 8 || b.Cout_p != (b.Cout + 7) / 8 * 8)
      return sr_fail(SR_EINVAL, "ecb_table_check: padded channel counts must be the next multiples of 8");
    if (b.mid < 1 || b.mid > kEcbMaxMid) return sr_fail(SR_EINVAL, "ecb_table_check: mid_planes must be in 1 .. 256");
    if (b.with_idt && b.Cin != b.Cout) return sr_fail(SR_EINVAL, "ecb_table_check: with_idt needs Cin == Cout");
    bool ok = b.w3 && b.b3 && b.k0 && b.b0 && b.k1 && b.b1 && b.rk && b.rb && b.wf && b.wd && b.bias_g;
    for (int e = 0; e < 3; ++e) ok = ok && b.ek0[e] && b.eb0[e] && b.escale[e] && b.ebias[e] && b.emask[e];
    if (!ok) return sr_fail(SR_EINVAL, "ecb_table_check: null parameter or image pointer");
    if (((uintptr_t)b.wf | (uintptr_t)b.wd) & 15) return sr_fail(SR_EINVAL, "ecb_table_check: images must be 16-byte aligned");
  }
  return SR_OK;
}

int sr_ecb_rep_fwd(int dtype, const sr_ecb_block* table, int L, int max_cout_p, void* stream) {
  if (!table || L < 1) return sr_fail(SR_EINVAL, "ecb_rep_fwd: null table or no blocks");
  if (dtype != SR_F32 && dtype != SR_BF16) return sr_fail(SR_EINVAL, "ecb_rep_fwd: dtype must be SR_F32 or SR_BF16");
  if (max_cout_p < 8 || max_cout_p > kEcbMaxCh || max_cout_p % 8 || L > 65535)
    return sr_fail(SR_EINVAL, "ecb_rep_fwd: max_cout_p must be a multiple of 8 in 8 .. 64, L <= 65535");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(ecb_rep_fwd_kernel<bf16_t>, dim3(max_cout_p, L), dim3(256), 0, s, table);
  else
    hipLaunchKernelGGL(ecb_rep_fwd_kernel<float>, dim3(max_cout_p, L), dim3(256), 0, s, table);
  return sr_check(hipGetLastError(), "ecb_rep_fwd launch");
}

int sr_ecb_rep_bwd(const sr_ecb_block* table, int L, int max_units, int accumulate, void* stream) {
  if (!table || L < 1) return sr_fail(SR_EINVAL, "ecb_rep_bwd: null table or no blocks");
  if (max_units < 2 || max_units > kEcbMaxCh + kEcbMaxMid || L > 65535)
    return sr_fail(SR_EINVAL, "ecb_rep_bwd: max_units (Cout + mid_planes) must be in 2 .. 320, L <= 65535");
  hipLaunchKernelGGL(ecb_rep_bwd_kernel, dim3(max_units, L), dim3(256), 0, (hipStream_t)stream, table, accumulate & 1);
  return sr_check(hipGetLastError(), "ecb_rep_bwd launch");
}

int sr_ecb_conv_blocks(const sr_ecb_conv_desc* d) {
  if (!d || ecb_conv_check(d)) return 0;
  const int64_t t = d->dtype == SR_BF16 ? ecb_conv_tiles<4, 2>(d) : ecb_conv_tiles<1, 1>(d);
  return t > 0x7fffffff ? 0 : (int)t;
}

int sr_ecb_conv(const sr_ecb_conv_desc* d, const void* x, const void* w, const float* bias, const float* slope, void* y,
                void* z, float* parts, const float* img, float* out, void* stream) {
  if (!d) return sr_fail(SR_EINVAL, "ecb_conv: null descriptor");
  if (const char* e = ecb_conv_check(d)) return sr_fail(SR_EINVAL, e);
  if (!x || !w) return sr_fail(SR_EINVAL, "ecb_conv: null pointer");
  if (d->mode == 1 ? (!img || !out || !bias) : !y) return sr_fail(SR_EINVAL, "ecb_conv: null pointer");
  if (d->mode == 2 && parts && !z) return sr_fail(SR_EINVAL, "ecb_conv: slope-gradient partials need the producer's z");
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)z) & 15)
    return sr_fail(SR_EINVAL, "ecb_conv: pointers must be 16-byte aligned");
  EcbConvArgs a{};
  a.x = (const char*)x, a.w = (const char*)w, a.bias = bias, a.slope = slope;
  a.y = (char*)y, a.z = (char*)z, a.parts = parts, a.img = img, a.out = out;
  hipStream_t s = (hipStream_t)stream;
  if (d->dtype == SR_BF16) return launch_ecb_conv_mode<bf16_t, 4, 2>(d, a, s);
  return launch_ecb_conv_mode<float, 1, 1>(d, a, s);
}

int sr_ecb_da_reduce(const sr_ecb_block* table, int layers, const float* parts, int nblocks, int accumulate, void* stream) {
  if (!table || !parts || layers < 1 || layers > 65535 || nblocks < 1)
    return sr_fail(SR_EINVAL, "ecb_da_reduce: null pointer or empty problem");
  hipLaunchKernelGGL(ecb_da_reduce_kernel, dim3(layers), dim3(64 * kDaParts), 0, (hipStream_t)stream, table, parts, nblocks,
                     accumulate & 1);
  return sr_check(hipGetLastError(), "ecb_da_reduce launch");
}

int sr_ecb_tail_bwd(int dtype, const float* dout, int N, int C, int H, int W, int s, int Cp, void* dz, void* stream) {
  if (!dout || !dz) return sr_fail(SR_EINVAL, "ecb_tail_bwd: null pointer");
  if (dtype != SR_F32 && dtype != SR_BF16) return sr_fail(SR_EINVAL, "ecb_tail_bwd: dtype must be SR_F32 or SR_BF16");
  if (N < 1 || C < 1 || H < 1 || W < 1 || s < 1 || Cp < C * s * s || Cp > kEcbMaxCh)
    return sr_fail(SR_EINVAL, "ecb_tail_bwd: bad shape");
  const int64_t blocks = ((int64_t)N * H * W * Cp + 255) / 256;
  if (blocks > 0x7fffffff) return sr_fail(SR_ETOOBIG, "ecb_tail_bwd: map too large");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(ecb_tail_bwd_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, dout, N, C, H, W, s, Cp,
                       (bf16_t*)dz);
  else
    hipLaunchKernelGGL(ecb_tail_bwd_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, dout, N, C, H, W, s, Cp,
                       (float*)dz);
  return sr_check(hipGetLastError(), "ecb_tail_bwd launch");
}

}  // extern "C"
