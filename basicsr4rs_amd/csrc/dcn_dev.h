// Device helpers that more than one deformable-conv kernel family uses.  Internal linkage, as the kernels have.
#pragma once
#include "dcn_args.h"

namespace sr_dcn {
namespace {

// the two bf16 of one 32-bit word as floats
SR_DEV float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
SR_DEV float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

template <typename T, int V> struct Vec;
template <> struct Vec<bf16_t, 8> {
  SR_DEV static void load(const bf16_t* p, float* f) {
    const u32x4 u = *(const u32x4*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = bf_lo(u[i]);
      f[2 * i + 1] = bf_hi(u[i]);
    }
  }
  SR_DEV static void store(bf16_t* p, const float* f) {
    u32x4 u;
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
    *(u32x4*)p = u;
  }
};
template <> struct Vec<float, 4> {
  SR_DEV static void load(const float* p, float* f) {
    const f32x4 v = *(const f32x4*)p;
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = v[i];
  }
  SR_DEV static void store(float* p, const float* f) { *(f32x4*)p = f32x4{f[0], f[1], f[2], f[3]}; }
};
template <typename T> struct Vec<T, 1> {
  SR_DEV static void load(const T* p, float* f) { f[0] = Elt<T>::to_f(*p); }
  SR_DEV static void store(T* p, const float* f) { *p = Elt<T>::from_f(f[0]); }
};

// Bilinear sampling geometry of one (pixel, tap): the reference's validity rule
// (h > -1 && w > -1 && h < H && w < W, deform_conv_cuda_kernel.cu:619) and corner rules
// (dmcn_im2col_bilinear, :468-498).  Corner offsets are pixel indices within the image,
// -1 where the corner lies outside.
struct Sample {
  bool valid;
  float lh, lw, hh, hw;
  int o1, o2, o3, o4;
};

SR_DEV Sample make_sample(float h, float w, int H, int W) {
  Sample s;
  s.valid = (h > -1.f && w > -1.f && h < (float)H && w < (float)W);
  s.o1 = s.o2 = s.o3 = s.o4 = -1;
  s.lh = s.lw = s.hh = s.hw = 0.f;
  if (!s.valid) return s;
  const float fh = floorf(h), fw = floorf(w);
  const int hl = (int)fh, wl = (int)fw, hh_ = hl + 1, wh = wl + 1;
  s.lh = h - fh;
  s.lw = w - fw;
  s.hh = 1.f - s.lh;
  s.hw = 1.f - s.lw;
  if (hl >= 0 && wl >= 0) s.o1 = hl * W + wl;
  if (hl >= 0 && wh <= W - 1) s.o2 = hl * W + wh;
  if (hh_ <= H - 1 && wl >= 0) s.o3 = hh_ * W + wl;
  if (hh_ <= H - 1 && wh <= W - 1) s.o4 = hh_ * W + wh;
  return s;
}

// LDS tile of offsets ([DG*2K][TP]) followed by masks ([DG*K][TP]) for pixels
// [p0, p0+np) of image n; missing mask (DCNv1) reads as 1.
SR_DEV void load_tile(float* s_off, float* s_msk, const float* off, const float* msk, const DcnArgs& a, int n,
                      int p0, int np) {
  const int64_t HWo = (int64_t)a.Ho * a.Wo;
  const int noff = a.DG * 2 * a.K, nm = a.DG * a.K;
  for (int i = threadIdx.x; i < (noff + nm) * a.TP; i += blockDim.x) {
    const int ch = i / a.TP, px = i - ch * a.TP;
    float v = 0.f;
    if (px < np) {
      if (ch < noff) v = off[((int64_t)n * noff + ch) * HWo + p0 + px];
      else v = msk ? msk[((int64_t)n * nm + ch - noff) * HWo + p0 + px] : 1.f;
    }
    if (ch < noff) s_off[ch * a.TP + px] = v;
    else s_msk[(ch - noff) * a.TP + px] = v;
  }
}

SR_DEV void mfma_bf16(const u32x4& a, const u32x4& b, f32x4& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a), __builtin_bit_cast(s16x8, b), acc, 0,
                                                0, 0);
}

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// 4 bf16 channels [c, c + 4) of pixel q of the LDS window (slot layout of dcn_fwd_win_kernel)
SR_DEV u32x2 win_read4(const unsigned char* sX, int q, int c) {
  return *(const u32x2*)(sX + q * 128 + (((c >> 3) ^ (q & 7)) << 4) + ((c >> 2) & 1) * 8);
}
SR_DEV u32x2 glb_read4(__amdgpu_buffer_rsrc_t xr, int o, uint32_t pxb, int c) {
  const u32x4 v = buf_load16(xr, o >= 0 ? (uint32_t)o * pxb + (uint32_t)(c >> 3) * 16u : SR_OOB);
  return (c & 4) ? u32x2{v[2], v[3]} : u32x2{v[0], v[1]};
}
SR_DEV float bf16_round(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// Eight-channel lane layout.  The MFMA leaves a lane 4 channels (16 cb + 4 (lane >> 4) .. + 3) of ONE
// pixel (lane & 15) per 16-channel tile; a bilinear sample (offset / mask reads, corner geometry) for
// 4 channels measured 438 us for the coordinate kernel (SQ: half the wave time waiting, VALU-heavy).
// With two pixel tiles per wave (tile rows 2 w and 2 w + 1) a lane swaps with lane ^ 16 the row it does
// not keep: afterwards lane (g, pl) holds channels 16 cb + 8 (g >> 1) .. + 7 of pixel pl of row g & 1 --
// one 16-B channel vector, one sample per deformable-group vector (308 us).
SR_DEV void own8(const f32x4& a0, const f32x4& a1, int g, float (&o)[8]) {
  const bool odd = g & 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float recv = __shfl_xor(odd ? a0[i] : a1[i], 16);  // the partner's values of my row
    const float mine = odd ? a1[i] : a0[i];
    o[i] = bf16_round(odd ? recv : mine);
    o[4 + i] = bf16_round(odd ? mine : recv);
  }
}

}  // namespace
}  // namespace sr_dcn
