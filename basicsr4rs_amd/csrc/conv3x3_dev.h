// Device helpers and constants that more than one conv3x3 kernel family uses.  A helper of one family is in
// that family's file.  Internal linkage, as the kernels' own helpers have.
#pragma once
#include "conv3x3_args.h"

namespace sr_conv {
namespace {

// alpha of output row m: a.alpha, times the per-image row_scale when given
SR_DEV float row_alpha(const FwdArgs& a, int m) {
  return a.row_scale ? a.alpha * a.row_scale[fdiv((uint32_t)m, a.fd_hw)] : a.alpha;
}

template <typename T>
SR_DEV void mfma_chunk(const u32x4& a, const u32x4& b, f32x4& acc);

template <>
SR_DEV void mfma_chunk<bf16_t>(const u32x4& a, const u32x4& b, f32x4& acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, a),
                                                __builtin_bit_cast(s16x8, b), acc, 0, 0, 0);
}
template <>
SR_DEV void mfma_chunk<float>(const u32x4& a, const u32x4& b, f32x4& acc) {
  // one 16-byte chunk = 4 consecutive K elements per lane: 4 f32 MFMAs (K=4 each); the
  // lane->k assignment is the same for A and B so the permuted K order sums correctly.
#pragma unroll
  for (int s = 0; s < 4; ++s)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a[s]), __uint_as_float(b[s]), acc,
                                               0, 0, 0);
}

// Byte offset of chunk c of row r inside a [rows][128 B] swizzled image.
SR_DEV uint32_t swz128(uint32_t r, uint32_t c) { return r * 128u + ((c ^ (r & 7u)) << 4); }

// Fused epilogue over a [ROWS][BN] fp32 tile staged in LDS (row stride CSTR floats):
// bias, activation, gate, alpha, residual, then a plain / pixel-shuffled NHWC store of
// 8-channel (16-byte bf16 / 32-byte f32) groups, or the fp32 NCHW affine store.
template <typename T, int ROWS, int BN, int NT>
SR_DEV void epilogue_tile(const FwdArgs& a, const float* Cs, int CSTR, int m0, int n0, int tid) {
  constexpr int SZ = Elt<T>::SIZE;
  // tile row -> NHWC pixel: m0 + row, or (a.strip64: the pph kernel's column strips, tiles ordered
  // (image, strip, 4-row block)) row r of the 256-row tile is pixel (r / 64, r % 64) of its block
  int sbase = 0;
  if (a.strip64) {
    const int tm = m0 >> 8, tps = a.H >> 2, ns = a.W >> 6;
    const int img = tm / (tps * ns), rem = tm - img * tps * ns, j = rem / tps, yb = rem - j * tps;
    sbase = (img * a.H + yb * 4) * a.W + j * 64;
  }
  auto mpix = [&](int row) -> int {
    if (!a.strip64) return m0 + row;
    const int rr = (m0 & 255) + row;
    return sbase + (rr >> 6) * a.W + (rr & 63);
  };
  if (a.out_nchw) {
    float* y = (float*)a.y;
    const int HW = a.H * a.W;
    for (int idx = tid; idx < ROWS * BN; idx += NT) {
      const int row = idx % ROWS, col = idx / ROWS;
      const int m = mpix(row), n = n0 + col;
      if (m0 + row >= a.M || n >= a.Cout_real) continue;
      float v = Cs[row * CSTR + col] + (a.bias ? a.bias[n] : 0.f);
      v = act_apply(v, a.act, a.slope) * row_alpha(a, m);
      v = v * (a.aff_scale ? a.aff_scale[n] : 1.f) + (a.aff_shift ? a.aff_shift[n] : 0.f);
      const int img = m / HW, pix = m - img * HW;
      y[((size_t)img * a.Cout_real + n) * HW + pix] = v;
    }
    return;
  }
  constexpr int CG = BN / 8;  // 8-channel groups per row
  constexpr int IT = ROWS * CG / NT;  // groups per thread
  static_assert(ROWS * CG % NT == 0, "epilogue tiling");
  constexpr int NV = SZ == 2 ? 1 : 2;  // 16-B loads per 8-channel group
  const __amdgpu_buffer_rsrc_t gr = make_rsrc(a.gate, a.g_bytes);
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(a.res, a.r_bytes);
  const __amdgpu_buffer_rsrc_t rr2 = make_rsrc(a.res2, a.r2_bytes);
  // per batch of IB groups: first issue every gate / residual load (range-checked buffer
  // loads: invalid groups read zeros) so their HBM latency overlaps, then compute + store.
  constexpr int IB = (SZ == 2 ? 4 : 2) < IT ? (SZ == 2 ? 4 : 2) : IT;  // groups per load batch
  static_assert(IT % IB == 0, "epilogue batch");
  // colsum: this thread's 8 channels (cg is fixed: NT % CG == 0) summed over its rows, of the
  // value as stored (bf16-rounded); reduced over the wave's lanes of the same cg below.
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  static_assert(NT % CG == 0 && 64 % CG == 0, "colsum lane map");
#pragma unroll 1
  for (int it0 = 0; it0 < IT; it0 += IB) {
  u32x4 gv[IB][NV], rv1[IB][NV], rv2[IB][NV];
#pragma unroll
  for (int ib = 0; ib < IB; ++ib) {
    const int it = ib;
    const int idx = tid + (it0 + ib) * NT;
    const int row = idx / CG, cg = idx % CG;
    const int m = mpix(row), n = n0 + cg * 8;
    const bool ok = m0 + row < a.M && n < a.Cout;
    const bool okr = ok && n < a.rcols;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      if (a.gate) {
        const bool gok = ok && (a.gate_mode != 2 || (n >= a.gcol0 && n < a.gcol1));
        gv[it][v] = buf_load16(gr, gok ? (uint32_t)(((size_t)m * a.ldg + a.gcoff + n) * SZ) + 16u * v : SR_OOB);
      }
      if (a.res) rv1[it][v] = buf_load16(rr, okr ? (uint32_t)(((size_t)m * a.ldr + a.rcoff + n) * SZ) + 16u * v : SR_OOB);
      if (a.res2)
        rv2[it][v] = buf_load16(rr2, okr ? (uint32_t)(((size_t)m * a.ldr2 + a.r2coff + n) * SZ) + 16u * v : SR_OOB);
    }
  }
  auto unpack = [&](const u32x4* q, float* o) {
    if constexpr (SZ == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[2 * j] = bf16_to_f32(q[0][j] & 0xffff);
        o[2 * j + 1] = bf16_to_f32(q[0][j] >> 16);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) { o[j] = __uint_as_float(q[0][j]); o[4 + j] = __uint_as_float(q[NV - 1][j]); }
    }
  };
#pragma unroll
  for (int it = 0; it < IB; ++it) {
    const int idx = tid + (it0 + it) * NT;
    const int row = idx / CG, cg = idx % CG;
    const int m = mpix(row), n = n0 + cg * 8;
    if (m0 + row >= a.M || n >= a.Cout) continue;
    float v[8];
    const f32x4 c0 = *(const f32x4*)(Cs + row * CSTR + cg * 8);
    const f32x4 c1 = *(const f32x4*)(Cs + row * CSTR + cg * 8 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[j] = c0[j]; v[4 + j] = c1[j]; }
    if (a.bias) {
      const f32x4 b0 = *(const f32x4*)(a.bias + n);
      const f32x4 b1 = *(const f32x4*)(a.bias + n + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] += b0[j]; v[4 + j] += b1[j]; }
    }
    if (a.aux) {  // activation side output (act_aux_n: GELU' for GELU, which the backward's gate reads)
      float ax[8];
      act_aux_n(v, ax, a.act, a.slope);
      const size_t da = (size_t)m * a.ldy + a.ycoff + n;
      if constexpr (SZ == 2) {
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(ax[2 * j], ax[2 * j + 1]);
        *(u32x4*)((bf16_t*)a.aux + da) = o;
      } else {
        *(f32x4*)((float*)a.aux + da) = f32x4{ax[0], ax[1], ax[2], ax[3]};
        *(f32x4*)((float*)a.aux + da + 4) = f32x4{ax[4], ax[5], ax[6], ax[7]};
      }
    } else {
      act_apply_n(v, a.act, a.slope);
    }
    if (a.gate && a.gate_mode != 2) {
      float g[8];
      unpack(gv[it], g);
      if (a.gate_mode == 1) {  // the stored GELU' (the forward's aux)
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= g[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= (g[j] > 0.f ? 1.f : a.gate_slope);
      }
    }
    {
      const float al = row_alpha(a, m);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= al;
    }
    if (a.res && n < a.rcols) {
      float rv[8];
      unpack(rv1[it], rv);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = a.beta * rv[j] + v[j];
    }
    if (a.res2 && n < a.rcols) {
      float rv[8];
      unpack(rv2[it], rv);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = a.beta2 * rv[j] + v[j];
    }
    if (a.gate && a.gate_mode == 2 && n >= a.gcol0 && n < a.gcol1) {
      float g[8];
      unpack(gv[it], g);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= (g[j] > 0.f ? 1.f : a.gate_slope);
    }
    size_t dst;  // element offset of the 8-channel group
    if (a.out_ps == 0) {
      dst = (size_t)m * a.ldy + a.ycoff + n;
    } else {
      const int r = a.out_ps;
      const int s = (int)fdiv((uint32_t)n, a.fd_cps);
      const int c = n - s * a.fd_cps.d;
      const int si = s / r, sj = s - (s / r) * r;
      const int xq = (int)fdiv((uint32_t)m, a.fd_W);
      const int xx = m - xq * a.W;  // xq = n*H + y
      dst = ((size_t)(xq * r + si) * (a.W * r) + xx * r + sj) * a.ldy + a.ycoff + c;
    }
    if constexpr (SZ == 2) {
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
      *(u32x4*)((bf16_t*)a.y + dst) = o;
      if (a.colsum) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          cs[2 * j] += bf16_to_f32(o[j] & 0xffff);
          cs[2 * j + 1] += bf16_to_f32(o[j] >> 16);
        }
      }
    } else {
      *(f32x4*)((float*)a.y + dst) = f32x4{v[0], v[1], v[2], v[3]};
      *(f32x4*)((float*)a.y + dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
      if (a.colsum) {
#pragma unroll
        for (int j = 0; j < 8; ++j) cs[j] += v[j];
      }
    }
  }
  }
  if (a.colsum) {
    // lanes l, l ^ CG, l ^ 2CG, ... hold the same 8 channels: fixed-order butterfly, then
    // lane cg writes row (m0 / ROWS) * (NT / 64) + wave of the [parts][Cout] partial matrix.
    const int lane = tid & 63;
#pragma unroll
    for (int off = CG; off < 64; off <<= 1)
#pragma unroll
      for (int j = 0; j < 8; ++j) cs[j] += __shfl_xor(cs[j], off, 64);
    const int n = n0 + lane * 8;
    if (lane < CG && n < a.Cout) {
      float* dstp = a.colsum + (size_t)((m0 / ROWS) * (NT / 64) + (tid >> 6)) * a.Cout + n;
      *(f32x4*)dstp = f32x4{cs[0], cs[1], cs[2], cs[3]};
      *(f32x4*)(dstp + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
    }
  }
}

// bytes of one LDS stage of the 256 x 256 forward kernels (conv3x3_fwd_big_kernel, conv3x3_fwd_pp_kernel)
constexpr int BIG_STAGE = 65536;

// raw s_barrier that the compiler moves no memory access across (the phase-interleaved schedules)
SR_DEV void pp_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// s_waitcnt vmcnt(n) for a run-time n (wave-uniform): the immediate is chosen by a binary
// search over 0..63 (6 scalar branches; a linear compare chain cost ~40 cycles per step at one
// wave per SIMD); n > 63 waits for vmcnt(63), which only waits longer.
template <int LO, int HI>
SR_DEV void vm_wait_bs(int n) {
  if constexpr (LO == HI) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LO) : "memory");
  } else {
    constexpr int MID = (LO + HI) / 2;
    if (n <= MID) vm_wait_bs<LO, MID>(n);
    else vm_wait_bs<MID + 1, HI>(n);
  }
}
SR_DEV void vm_wait_dyn(int n) { vm_wait_bs<0, 63>(n < 0 ? 0 : (n > 63 ? 63 : n)); }

}  // namespace
}  // namespace sr_conv
