// k x k convolution (odd k in {3, 5, 7, 9}, stride 1, zero padding k / 2) for narrow channel counts
// (Cin_p, Cout_p <= 64) and the bicubic upsampler: the kernels of SRCNN (bicubic -> 9x9 -> 5x5 -> 5x5).
//
//   sr_convk_fwd    y = alpha * act(conv(x, w) + bias) on NHWC maps; the input gradient is the same
//                   kernel on the flipped, transposed weight image (wd of sr_conv_prep_mapped).
//   sr_convk_wgrad  dw / db in the nn.Conv2d parameter layout: split over pixel tiles into fp32 slabs,
//                   reduced in a fixed order (no atomics: two runs are bit-identical).
//   sr_bicubic_up   F.interpolate(mode='bicubic', align_corners=True) by an integer scale, fp32 NCHW in,
//                   NHWC feature map out.
//   sr_bicubic_up_hp  the align_corners=False form, fp32 NCHW in and out, written into a channel range
//                   of a wider tensor (the ground-truth assembly of L2SSingleModel.feed_data).
//
// Forward.  A block of 4 waves owns a TH x TW tile of output pixels of ONE image and stages the tile
// plus its k - 1 halo of x in LDS once; pixels outside the image are written as zeros there, so no
// lane ever reads another image's rows and a non-finite input pixel reaches only the k x k outputs
// around it.  The GEMM is D[co][pixel] = sum_K w[co][K] * x[pixel + tap][ci] with K = tap * Cin + ci
// walked in 16-byte chunks (8 bf16 / 4 f32 channels of one tap): the weight rows are the MFMA A
// operand (16-byte loads of the GEMM image, shared by the block's waves through L1/L2 and prefetched
// one step ahead), the LDS halo the B operand.  One v_mfma_f32_16x16x32_bf16 takes four chunks, i.e.
// for Cin_p = 8 four consecutive taps of the flattened (ky, kx) order: the 9x9 x 8 first layer runs
// 21 full-width MFMAs per tile pair instead of 81 quarter-filled ones.  A lane ends up with 4
// consecutive output channels of one pixel (one 8-byte bf16 / 16-byte f32 store).
// The LDS pixel stride is Cin * size + 16 B when that size is a multiple of 64 B: 16 consecutive
// pixels' 16-byte reads then fall in 16 distinct bank groups (144 B stride: 36 dwords, a
// permutation of the 64 banks in steps of 4).
#include "sr_common.h"
#include "sr_internal.h"

namespace {

struct KFwdArgs {
  const char* x;
  const char* w;
  const float* bias;
  char* y;
  int N, H, W, k, Cin, Cout, Cout_real, act;
  float alpha;
  int tiles_x, tiles_y;
  int pstride;  // LDS bytes per halo pixel
  int cpp;      // 16-byte chunks per pixel (Cin / PER16)
  int nchunk;   // k * k * cpp
  int ldw;      // k * k * Cin: elements per weight row
};

// PT pixel tiles (16 px of one row) per wave, TWT tiles per tile row: TW = 16 * TWT pixels,
// a wave owns PT / TWT rows, the block TH = 4 * PT / TWT rows.
template <typename T, int PT, int TWT>
__global__ __launch_bounds__(256) void convk_fwd_kernel(const KFwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int SZ = Elt<T>::SIZE;
  constexpr int TW = 16 * TWT, RW = PT / TWT, TH = 4 * RW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int k = a.k, pad = k >> 1;
  const int HWp = TW + k - 1, HH = TH + k - 1;
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
    const int gy = y0 + hy - pad, gx = x0 + hx - pad;
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
    // four chunks per MFMA: lane group g takes chunk 4 * step + g
    const int nsteps = (a.nchunk + 3) >> 2;
    int c = g % a.cpp, tap = g / a.cpp;
    int ky = tap / k, kx = tap - ky * k;
    auto load_a = [&](int step, u32x4 (&fa)[4]) {
      const int kc = step * 4 + g;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int co = ct * 16 + l16;
        fa[ct] = u32x4{0u, 0u, 0u, 0u};
        if (ct < CT && kc < a.nchunk && co < a.Cout) fa[ct] = *(const u32x4*)(a.w + (size_t)co * wrow + (size_t)kc * 16);
      }
    };
    u32x4 fa[4], fn[4];
    load_a(0, fa);
    for (int step = 0; step < nsteps; ++step) {
      if (step + 1 < nsteps) load_a(step + 1, fn);
      const bool valid = step * 4 + g < a.nchunk;
      u32x4 fb[PT];
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
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) fa[ct] = fn[ct];
      c += 4;  // this lane's chunk of the next step
      while (c >= a.cpp) {
        c -= a.cpp;
        if (++kx == k) {
          kx = 0;
          ++ky;
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
        if (++kx == k) {
          kx = 0;
          ++ky;
        }
      }
    }
  }

  // epilogue: lane = pixel l16 of tile i, output channels ct * 16 + 4 g .. + 3
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int gy = y0 + wave * RW + i / TWT, gx = x0 + (i % TWT) * 16 + l16;
    if (gy >= a.H || gx >= a.W) continue;
    char* yp = a.y + (((size_t)n * a.H + gy) * a.W + gx) * (size_t)(a.Cout * SZ);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int co = ct * 16 + 4 * g;
      if (co >= a.Cout) continue;  // Cout is a multiple of 8: a lane's 4 channels are all in or all out
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float t = acc[ct][i][j] + (a.bias ? a.bias[co + j] : 0.f);
        if (a.act == 1) t = t < 0.f ? 0.f : t;  // a NaN stays a NaN, as torch.relu
        v[j] = co + j < a.Cout_real ? t * a.alpha : 0.f;  // padded channels: exactly zero
      }
      if constexpr (SZ == 2) {
        *(u32x2*)(yp + co * 2) = u32x2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
      } else {
        *(f32x4*)(yp + co * 4) = f32x4{v[0], v[1], v[2], v[3]};
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient.  GEMM D[co][ci] (per tap) = sum over pixels dy[p][co] * x[p + tap][ci]: M = Cout,
// N = Cin per tap, K = pixels.  Grid (S pixel splits, k kernel rows): block (s, ky) walks the 4 x 32
// pixel tiles s, s + S, ... (a fixed assignment), stages dy's tile and the x rows shifted by ky (with
// the k - 1 column halo, zeros outside the image) in LDS, and wave w accumulates output-channel tile
// w x all ci tiles x the k taps of its kernel row in registers (up to 9 x 4 accumulators).  A K step
// is 32 pixels of one tile row; the fragments (8 pixels of one channel per lane) are gathered from the
// pixel-major LDS image with 2-byte reads -- x as one 8 + k - 1 pixel window per ci tile that all k
// taps of the row slice.  The partial [taps][Cout][Cin] results go to slab s of the workspace and a
// second kernel sums the S slabs in order into the parameter layout.
// ------------------------------------------------------------------------------------------------
struct KWgArgs {
  const char* dy;
  const char* x;
  float* ws;
  float* wsb;
  int N, H, W, k, Cin, Cout;
  int tiles_x, tiles_y, ntiles, S;
  int psx, psy;  // LDS bytes per pixel of the x / dy images
};

constexpr int WG_TH = 4, WG_TW = 32;

template <typename T>
__global__ __launch_bounds__(256) void convk_wgrad_kernel(const KWgArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int SZ = Elt<T>::SIZE, P16 = Elt<T>::PER16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int k = a.k, pad = k >> 1;
  const int s = blockIdx.x, ky = blockIdx.y;
  const int XW = WG_TW + k - 1;
  char* xs = lds;
  char* ys = lds + (size_t)WG_TH * XW * a.psx;
  const int cpx = a.Cin / P16, cpy = a.Cout / P16;
  const int IT = (a.Cin + 15) >> 4;
  const int co0 = wave * 16;
  const bool active = co0 < a.Cout;
  // clamped channel of this lane (rows / columns past Cout / Cin are computed on a copy and dropped)
  const int co_l = min(co0 + l16, a.Cout - 1);

  f32x4 acc[9][4];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;

  for (int t = s; t < a.ntiles; t += a.S) {
    int b = t;
    const int tx = b % a.tiles_x;
    b /= a.tiles_x;
    const int ty = b % a.tiles_y;
    const int n = b / a.tiles_y;
    const int x0 = tx * WG_TW, y0 = ty * WG_TH;
    __syncthreads();  // the previous tile's fragment reads are done
    for (int idx = tid; idx < WG_TH * XW * cpx; idx += 256) {
      const int pix = idx / cpx, c = idx - pix * cpx;
      const int r = pix / XW, hx = pix - r * XW;
      const int gy = y0 + r + ky - pad, gx = x0 + hx - pad;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
        v = *(const u32x4*)(a.x + (((size_t)n * a.H + gy) * a.W + gx) * (size_t)(a.Cin * SZ) + (size_t)c * 16);
      *(u32x4*)(xs + (size_t)pix * a.psx + c * 16) = v;
    }
    for (int idx = tid; idx < WG_TH * WG_TW * cpy; idx += 256) {
      const int pix = idx / cpy, c = idx - pix * cpy;
      const int r = pix / WG_TW, px = pix - r * WG_TW;
      const int gy = y0 + r, gx = x0 + px;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (gy < a.H && gx < a.W)
        v = *(const u32x4*)(a.dy + (((size_t)n * a.H + gy) * a.W + gx) * (size_t)(a.Cout * SZ) + (size_t)c * 16);
      *(u32x4*)(ys + (size_t)pix * a.psy + c * 16) = v;
    }
    __syncthreads();
    if (!active) continue;
    for (int r = 0; r < WG_TH; ++r) {
      if (y0 + r >= a.H) break;  // rows past the image hold zeros only
      if constexpr (SZ == 2) {
        // A: dy[pixels 8 g .. 8 g + 7][co]
        unsigned short ya[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          ya[j] = *(const unsigned short*)(ys + (size_t)(r * WG_TW + 8 * g + j) * a.psy + co_l * 2);
        if (ky == 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bsum += bf16_to_f32(ya[j]);
        }
        u32x4 fa;
#pragma unroll
        for (int j = 0; j < 4; ++j) fa[j] = (unsigned)ya[2 * j] | ((unsigned)ya[2 * j + 1] << 16);
#pragma unroll
        for (int it = 0; it < 4; ++it) {
          if (it >= IT) continue;
          const int ci_l = min(it * 16 + l16, a.Cin - 1);
          // x window: pixels 8 g .. 8 g + 8 + k - 2 of the halo row, all k taps slice it
          unsigned short xw[16];
#pragma unroll
          for (int m = 0; m < 16; ++m) {
            xw[m] = 0;
            if (m < 8 + k - 1) xw[m] = *(const unsigned short*)(xs + (size_t)(r * XW + 8 * g + m) * a.psx + ci_l * 2);
          }
#pragma unroll
          for (int kx = 0; kx < 9; ++kx) {
            if (kx >= k) continue;
            u32x4 fb;
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = (unsigned)xw[kx + 2 * j] | ((unsigned)xw[kx + 2 * j + 1] << 16);
            acc[kx][it] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, fa),
                                                                  __builtin_bit_cast(s16x8, fb), acc[kx][it], 0, 0, 0);
          }
        }
      } else {
        for (int q = 0; q < WG_TW / 4; ++q) {
          const int px = 4 * q + g;
          const float fa = *(const float*)(ys + (size_t)(r * WG_TW + px) * a.psy + co_l * 4);
          if (ky == 0) bsum += fa;
#pragma unroll
          for (int it = 0; it < 4; ++it) {
            if (it >= IT) continue;
            const int ci_l = min(it * 16 + l16, a.Cin - 1);
#pragma unroll
            for (int kx = 0; kx < 9; ++kx) {
              if (kx >= k) continue;
              const float fb = *(const float*)(xs + (size_t)(r * XW + px + kx) * a.psx + ci_l * 4);
              acc[kx][it] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa, fb, acc[kx][it], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  if (!active) return;
  // D[co = 4 g + j][ci = l16] of every (kx, ci tile) into slab s
  const int taps = k * k;
#pragma unroll
  for (int kx = 0; kx < 9; ++kx) {
    if (kx >= k) continue;
    float* slab = a.ws + ((size_t)s * taps + (ky * k + kx)) * a.Cout * a.Cin;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      if (it >= IT) continue;
      const int ci = it * 16 + l16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int co = co0 + 4 * g + j;
        if (co < a.Cout && ci < a.Cin) slab[(size_t)co * a.Cin + ci] = acc[kx][it][j];
      }
    }
  }
  if (ky == 0 && a.wsb) {
    // the lane groups hold partial sums of the same channel: fold them (same order in every lane)
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    if (g == 0 && co0 + l16 < a.Cout) a.wsb[(size_t)s * a.Cout + co0 + l16] = bsum;
  }
}

// dw[co][ci][tap] (+)= scale * sum_s slab[s][tap][co][ci], db[co] (+)= scale * sum_s wsb[s][co]
__global__ void convk_wgrad_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ wsb, int S, int taps,
                                          int Cout, int Cin, int Cout_real, int Cin_real, float scale, int accumulate,
                                          float* __restrict__ dw, float* __restrict__ db) {
  const int64_t nw = (int64_t)taps * Cout_real * Cin_real;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nw) {
    const int ci = (int)(i % Cin_real);
    const int co = (int)((i / Cin_real) % Cout_real);
    const int tap = (int)(i / ((int64_t)Cin_real * Cout_real));
    const float* src = ws + ((size_t)tap * Cout + co) * Cin + ci;
    const size_t stride = (size_t)taps * Cout * Cin;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += src[(size_t)s * stride];
    float* d = dw + ((size_t)co * Cin_real + ci) * taps + tap;
    *d = sum * scale + (accumulate ? *d : 0.f);
  } else if (db && i < nw + Cout_real) {
    const int co = (int)(i - nw);
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += wsb[(size_t)s * Cout + co];
    db[co] = sum * scale + (accumulate ? db[co] : 0.f);
  }
}

// ------------------------------------------------------------------------------------------------
// Bicubic upsampling, align_corners = True (torch.nn.functional.interpolate semantics): source
// coordinate o * (in - 1) / (out - 1) (0 when out == 1), cubic convolution weights with A = -0.75,
// the four tap indices clamped to the image, rows first interpolated along x, then along y; fp32.
// One thread per output element of the NHWC map (channel fastest: coalesced stores, padded
// channels zero); the LR planes it gathers from are small and stay in cache.
// ------------------------------------------------------------------------------------------------
SR_DEV void cubic_coeffs(float t, float (&c)[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x1 = t, x2 = 1.f - t, x3 = 2.f - t;
  c[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  c[1] = ((A + 2.f) * x1 - (A + 3.f)) * x1 * x1 + 1.f;
  c[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  c[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

template <typename T>
__global__ void bicubic_up_kernel(const float* __restrict__ x, int N, int C, int H, int W, int s, int Cp,
                                  T* __restrict__ y) {
  const int Ho = H * s, Wo = W * s;
  const int64_t total = (int64_t)N * Ho * Wo * Cp;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % Cp);
  int64_t p = i / Cp;
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho);
  const int n = (int)(p / Ho);
  float v = 0.f;
  if (c < C) {
    const float sy = Ho > 1 ? (float)(H - 1) / (float)(Ho - 1) : 0.f;
    const float sx = Wo > 1 ? (float)(W - 1) / (float)(Wo - 1) : 0.f;
    const float ry = sy * (float)oy, rx = sx * (float)ox;
    const float fy = floorf(ry), fx = floorf(rx);
    const int iy = (int)fy, ix = (int)fx;
    float cy[4], cx[4];
    cubic_coeffs(ry - fy, cy);
    cubic_coeffs(rx - fx, cx);
    const float* plane = x + ((size_t)n * C + c) * (size_t)H * W;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int yy = min(max(iy - 1 + r, 0), H - 1);
      const float* row = plane + (size_t)yy * W;
      float h = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xx = min(max(ix - 1 + q, 0), W - 1);
        h += row[xx] * cx[q];
      }
      v += h * cy[r];
    }
  }
  y[i] = Elt<T>::from_f(v);
}

// Bicubic upsampling, align_corners = False ("half-pixel" centres, F.interpolate's default): source
// coordinate (d + 0.5) / s - 0.5, not clamped; its floor and fraction t; the same A = -0.75 weights and
// clamped taps.  With an integer scale d = q * s + p gives the coordinate q + f, f = (p + 0.5) / s - 0.5
// in (-0.5, 0.5): floor q - 1 and t = f + 1 for f < 0, else floor q and t = f -- t is a function of the
// phase p alone and is formed from small integers, so it carries no error that grows with d.
// fp32 NCHW in, fp32 NCHW out into channels [c0, c0 + C) of a [N, Cy, H s, W s] tensor (a fused cat).
SR_DEV void hp_phase(int d, int s, int& i0, float (&c)[4]) {
  const int q = d / s, p = d - q * s;
  const float f = ((float)p + 0.5f) / (float)s - 0.5f;
  i0 = f < 0.f ? q - 1 : q;
  cubic_coeffs(f < 0.f ? f + 1.f : f, c);
}

__global__ void bicubic_up_hp_kernel(const float* __restrict__ x, int N, int C, int H, int W, int s,
                                     float* __restrict__ y, int Cy, int c0) {
  const int Ho = H * s, Wo = W * s;
  const int64_t total = (int64_t)N * C * Ho * Wo;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % Wo);
  int64_t p = i / Wo;
  const int oy = (int)(p % Ho);
  p /= Ho;
  const int c = (int)(p % C);
  const int n = (int)(p / C);
  int iy, ix;
  float cy[4], cx[4];
  hp_phase(oy, s, iy, cy);
  hp_phase(ox, s, ix, cx);
  const float* plane = x + ((size_t)n * C + c) * (size_t)H * W;
  float v = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int yy = min(max(iy - 1 + r, 0), H - 1);
    const float* row = plane + (size_t)yy * W;
    float h = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int xx = min(max(ix - 1 + q, 0), W - 1);
      h += row[xx] * cx[q];
    }
    v += h * cy[r];
  }
  y[(((size_t)n * Cy + c0 + c) * Ho + oy) * (size_t)Wo + ox] = v;
}

int lds_pixel_stride(int channels, int size) {
  const int b = channels * size;
  return b % 64 == 0 ? b + 16 : b;
}

constexpr int kMaxLds = 160 * 1024;

// The support envelope of the k x k kernels (checked before any launch).
const char* convk_check(const sr_convk_desc* d) {
  if (d->dtype != SR_F32 && d->dtype != SR_BF16) return "convk: dtype must be SR_F32 or SR_BF16";
  if (d->k != 3 && d->k != 5 && d->k != 7 && d->k != 9) return "convk: k must be odd, 3 <= k <= 9";
  if (d->N < 1 || d->H < 1 || d->W < 1) return "convk: N, H, W must be >= 1";
  if (d->Cin < 8 || d->Cout < 8 || d->Cin % 8 || d->Cout % 8) return "convk: channel counts must be multiples of 8";
  if (d->Cin > 64 || d->Cout > 64) return "convk: padded channel counts above 64 are not supported";
  if (d->Cin_real < 1 || d->Cin_real > d->Cin || d->Cout_real < 1 || d->Cout_real > d->Cout)
    return "convk: real channel counts must be in 1 .. padded";
  if (d->act != SR_ACT_NONE && d->act != SR_ACT_RELU) return "convk: act must be none or ReLU";
  return nullptr;
}

template <typename T, int PT, int TWT>
int launch_convk_fwd(const sr_convk_desc* d, const void* x, const void* w, const float* bias, void* y, hipStream_t s) {
  constexpr int TW = 16 * TWT, TH = 4 * PT / TWT;
  KFwdArgs a;
  a.x = (const char*)x;
  a.w = (const char*)w;
  a.bias = bias;
  a.y = (char*)y;
  a.N = d->N, a.H = d->H, a.W = d->W, a.k = d->k, a.Cin = d->Cin, a.Cout = d->Cout, a.Cout_real = d->Cout_real;
  a.act = d->act;
  a.alpha = d->alpha;
  a.tiles_x = (d->W + TW - 1) / TW;
  a.tiles_y = (d->H + TH - 1) / TH;
  a.pstride = lds_pixel_stride(d->Cin, Elt<T>::SIZE);
  a.cpp = d->Cin / Elt<T>::PER16;
  a.nchunk = d->k * d->k * a.cpp;
  a.ldw = d->k * d->k * d->Cin;
  const int64_t blocks = (int64_t)a.tiles_x * a.tiles_y * d->N;
  if (blocks > 0x7fffffff) return sr_fail(SR_ETOOBIG, "convk_fwd: too many tiles");
  const size_t lds = (size_t)(TH + d->k - 1) * (TW + d->k - 1) * a.pstride;
  if (lds > (size_t)kMaxLds) return sr_fail(SR_EINVAL, "convk_fwd: halo tile exceeds LDS");
  auto kern = convk_fwd_kernel<T, PT, TWT>;
  if (lds > 65536 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return sr_fail(SR_ELAUNCH, "convk_fwd: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, s, a);
  return sr_check(hipGetLastError(), "convk_fwd launch");
}

int wgrad_splits(const sr_convk_desc* d, int* ntiles) {
  const int64_t tx = (d->W + WG_TW - 1) / WG_TW, ty = (d->H + WG_TH - 1) / WG_TH;
  const int64_t nt = tx * ty * d->N;
  *ntiles = nt > 0x7fffffff ? -1 : (int)nt;
  const int target = 512 / d->k > 1 ? 512 / d->k : 1;  // ~512 blocks over the k kernel rows
  return (int)(nt < target ? nt : target);
}

template <typename T>
int launch_convk_wgrad(const sr_convk_desc* d, const void* dy, const void* x, float* ws, float* wsb, hipStream_t s) {
  KWgArgs a;
  a.dy = (const char*)dy;
  a.x = (const char*)x;
  a.ws = ws;
  a.wsb = wsb;
  a.N = d->N, a.H = d->H, a.W = d->W, a.k = d->k, a.Cin = d->Cin, a.Cout = d->Cout;
  a.tiles_x = (d->W + WG_TW - 1) / WG_TW;
  a.tiles_y = (d->H + WG_TH - 1) / WG_TH;
  a.S = wgrad_splits(d, &a.ntiles);
  a.psx = lds_pixel_stride(d->Cin, Elt<T>::SIZE);
  a.psy = lds_pixel_stride(d->Cout, Elt<T>::SIZE);
  const size_t lds = (size_t)WG_TH * (WG_TW + d->k - 1) * a.psx + (size_t)WG_TH * WG_TW * a.psy;
  if (lds > (size_t)kMaxLds) return sr_fail(SR_EINVAL, "convk_wgrad: tiles exceed LDS");
  auto kern = convk_wgrad_kernel<T>;
  if (lds > 65536 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return sr_fail(SR_ELAUNCH, "convk_wgrad: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL(kern, dim3(a.S, d->k), dim3(256), lds, s, a);
  return sr_check(hipGetLastError(), "convk_wgrad launch");
}

}  // namespace

extern "C" {

int sr_convk_fwd(const sr_convk_desc* d, const void* x, const void* w, const float* bias, void* y, void* stream) {
  if (!d) return sr_fail(SR_EINVAL, "convk_fwd: null descriptor");
  if (const char* e = convk_check(d)) return sr_fail(SR_EINVAL, e);
  if (!x || !w || !y) return sr_fail(SR_EINVAL, "convk_fwd: null pointer");
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y) & 15) return sr_fail(SR_EINVAL, "convk_fwd: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (d->dtype == SR_BF16) return launch_convk_fwd<bf16_t, 4, 2>(d, x, w, bias, y, s);
  return launch_convk_fwd<float, 1, 1>(d, x, w, bias, y, s);
}

size_t sr_convk_wgrad_workspace(const sr_convk_desc* d) {
  if (!d || convk_check(d)) return 0;
  int nt;
  const size_t S = (size_t)wgrad_splits(d, &nt);
  if (nt < 0) return 0;
  return S * ((size_t)d->k * d->k * d->Cout * d->Cin + d->Cout) * sizeof(float);
}

int sr_convk_wgrad(const sr_convk_desc* d, const void* dy, const void* x, void* workspace, size_t ws_bytes, float* dw,
                   float* db, void* stream) {
  if (!d) return sr_fail(SR_EINVAL, "convk_wgrad: null descriptor");
  if (const char* e = convk_check(d)) return sr_fail(SR_EINVAL, e);
  if (!dy || !x || !workspace || !dw) return sr_fail(SR_EINVAL, "convk_wgrad: null pointer");
  if (((uintptr_t)x | (uintptr_t)dy | (uintptr_t)workspace) & 15)
    return sr_fail(SR_EINVAL, "convk_wgrad: pointers must be 16-byte aligned");
  int nt;
  const int S = wgrad_splits(d, &nt);
  if (nt < 0) return sr_fail(SR_ETOOBIG, "convk_wgrad: too many tiles");
  if (ws_bytes < sr_convk_wgrad_workspace(d)) return sr_fail(SR_EINVAL, "convk_wgrad: workspace too small");
  const int taps = d->k * d->k;
  float* ws = (float*)workspace;
  float* wsb = ws + (size_t)S * taps * d->Cout * d->Cin;
  hipStream_t s = (hipStream_t)stream;
  const int rc = d->dtype == SR_BF16 ? launch_convk_wgrad<bf16_t>(d, dy, x, ws, wsb, s)
                                     : launch_convk_wgrad<float>(d, dy, x, ws, wsb, s);
  if (rc) return rc;
  const int64_t work = (int64_t)taps * d->Cout_real * d->Cin_real + d->Cout_real;
  hipLaunchKernelGGL(convk_wgrad_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, ws, wsb, S, taps,
                     d->Cout, d->Cin, d->Cout_real, d->Cin_real, d->scale, d->accumulate & 1, dw, db);
  return sr_check(hipGetLastError(), "convk_wgrad reduce launch");
}

int sr_bicubic_up(int dtype, const float* x, int N, int C, int H, int W, int s, int Cp, void* y, void* stream) {
  if (!x || !y) return sr_fail(SR_EINVAL, "bicubic_up: null pointer");
  if (dtype != SR_F32 && dtype != SR_BF16) return sr_fail(SR_EINVAL, "bicubic_up: dtype must be SR_F32 or SR_BF16");
  if (N < 1 || C < 1 || H < 1 || W < 1 || s < 1 || Cp < C) return sr_fail(SR_EINVAL, "bicubic_up: bad shape");
  if ((int64_t)H * s > 0x7fffffff || (int64_t)W * s > 0x7fffffff) return sr_fail(SR_ETOOBIG, "bicubic_up: output too large");
  const int64_t total = (int64_t)N * H * s * W * s * Cp;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return sr_fail(SR_ETOOBIG, "bicubic_up: output too large");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SR_BF16)
    hipLaunchKernelGGL(bicubic_up_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, st, x, N, C, H, W, s, Cp,
                       (bf16_t*)y);
  else
    hipLaunchKernelGGL(bicubic_up_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, x, N, C, H, W, s, Cp,
                       (float*)y);
  return sr_check(hipGetLastError(), "bicubic_up launch");
}

int sr_bicubic_up_hp(const float* x, int N, int C, int H, int W, int s, float* y, int Cy, int c0, void* stream) {
  if (!x || !y) return sr_fail(SR_EINVAL, "bicubic_up_hp: null pointer");
  if (N < 1 || C < 1 || H < 1 || W < 1 || s < 1) return sr_fail(SR_EINVAL, "bicubic_up_hp: bad shape");
  if (c0 < 0 || (int64_t)c0 + C > Cy) return sr_fail(SR_EINVAL, "bicubic_up_hp: channels [c0, c0 + C) must lie in [0, Cy)");
  if ((int64_t)H * s > 0x7fffffff || (int64_t)W * s > 0x7fffffff) return sr_fail(SR_ETOOBIG, "bicubic_up_hp: output too large");
  const int64_t plane = (int64_t)H * s * W * s;
  if (plane > INT64_MAX / N / C) return sr_fail(SR_ETOOBIG, "bicubic_up_hp: output too large");
  const int64_t blocks = (plane * N * C + 255) / 256;
  if (blocks > 0x7fffffff) return sr_fail(SR_ETOOBIG, "bicubic_up_hp: output too large");
  hipLaunchKernelGGL(bicubic_up_hp_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, N, C, H, W, s, y,
                     Cy, c0);
  return sr_check(hipGetLastError(), "bicubic_up_hp launch");
}

}  // extern "C"
