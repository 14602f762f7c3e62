// conv3x3 forward / dgrad, the generic tile kernel (any shape, bf16 and exact f32) and the narrow-conv halo
// kernel (Cout < 256 at W 64 / 128, the W 256 one-row form): conv3x3_fwd_kernel, conv3x3_fwd_halo_kernel and
// their launches.  The two share one instantiation of the fused epilogue (epilogue_tile<bf16_t, 128, 64, 256>),
// and the halo kernel compiles to other code without the tile kernel beside it, so they stay in one source.
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

template <typename T, int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv3x3_fwd_kernel(FwdArgs a) {
  constexpr int PER = Elt<T>::PER16;
  constexpr int SZ = Elt<T>::SIZE;
  constexpr int MI = BM / WM / 16;
  constexpr int NI = BN / WN / 16;
  constexpr int A_CH = BM * 8 / 256;                     // A chunks per thread
  constexpr int B_CH = (BN * 8 >= 256) ? BN * 8 / 256 : 1;  // B chunks per thread
  constexpr bool B_PART = BN * 8 < 256;                   // only some threads load B
  constexpr int STAGE = (BM + BN) * 128;
  constexpr int CSTR = BN + 4;  // epilogue fp32 row stride (floats)
  constexpr int SMEM = (2 * STAGE > BM * CSTR * 4) ? 2 * STAGE : BM * CSTR * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (int)(tile / a.tiles_n) * BM;
  const int n0 = (int)(tile % a.tiles_n) * BN;

  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(a.w, a.w_bytes);

  // ---- per-thread A rows: pixel coordinates, fixed for the whole K loop ----
  const int cA = tid & 7;
  int ay[A_CH], ax[A_CH], anh[A_CH];  // y, x, n*H (anh < 0: row beyond M)
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    int m = m0 + (tid >> 3) + 32 * i;
    if (m < a.M) {
      uint32_t q = fdiv((uint32_t)m, a.fd_W);
      ax[i] = m - (int)q * a.W;
      uint32_t n = fdiv(q, a.fd_H);
      ay[i] = (int)q - (int)n * a.H;
      anh[i] = (int)n * a.H;
    } else {
      ax[i] = 0; ay[i] = -100000; anh[i] = 0;
    }
  }
  const int bRow = tid >> 3;  // B rows bRow + 32*i

  u32x4 ra[A_CH], rb[B_CH];
  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (a.nkc + 7) >> 3;

  auto load = [&](int ks) {
    const int q = ks * 8 + cA;  // this thread's K chunk
    const int tap_i = (int)fdiv((uint32_t)q, a.fd_cpt);
    const int cc = q - tap_i * a.cpt;
    const int tap = tap_i + a.tap0;
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    const bool kval = q < a.nkc;
    const int ch = cc * PER;  // GEMM input channel of the chunk
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int yy = ay[i] + dy, xx = ax[i] + dx;
      const bool v = kval && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      uint32_t off;
      if (a.in_up > 1) {
        const int u = a.in_up;  // source grid is [N, H/u, W/u]
        off = (uint32_t)((((anh[i] / u + yy / u) * (a.W / u) + xx / u) * a.ldx + a.xcoff + ch) * SZ);
      } else if (a.in_ps == 0) {
        off = (uint32_t)((((anh[i] + yy) * a.W + xx) * a.ldx + a.xcoff + ch) * SZ);
      } else {
        const int r = a.in_ps;
        const int s = (int)fdiv((uint32_t)ch, a.fd_cps);
        const int c = ch - s * a.fd_cps.d;
        const int si = s / r, sj = s - (s / r) * r;
        const int Wr = a.W * r;
        off = (uint32_t)((((anh[i] + yy) * r + si) * Wr + xx * r + sj) * a.ldx + a.xcoff + c) * SZ;
      }
      ra[i] = buf_load16(xr, v ? off : SR_OOB);
    }
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const int row = n0 + bRow + 32 * i;
      const bool v = kval && row < a.Cout && (!B_PART || tid < BN * 8);
      const uint32_t off = (uint32_t)((row * a.ldw + q * PER) * SZ);
      rb[i] = buf_load16(wr, v ? off : SR_OOB);
    }
  };
  auto store = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + BM * 128;
#pragma unroll
    for (int i = 0; i < A_CH; ++i) *(u32x4*)(As + swz128((tid >> 3) + 32 * i, cA)) = ra[i];
#pragma unroll
    for (int i = 0; i < B_CH; ++i)
      if (!B_PART || tid < BN * 8) *(u32x4*)(Bs + swz128(bRow + 32 * i, cA)) = rb[i];
  };
  auto compute = [&](int buf) {
    const char* As = smem + buf * STAGE;
    const char* Bs = As + BM * 128;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const uint32_t c = kk * 4 + (lane >> 4);
      u32x4 fa[MI], fb[NI];
#pragma unroll
      for (int i = 0; i < MI; ++i)
        fa[i] = *(const u32x4*)(As + swz128(wm * (BM / WM) + i * 16 + (lane & 15), c));
#pragma unroll
      for (int j = 0; j < NI; ++j)
        fb[j] = *(const u32x4*)(Bs + swz128(wn * (BN / WN) + j * 16 + (lane & 15), c));
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) mfma_chunk<T>(fa[i], fb[j], acc[i][j]);
    }
  };

  load(0);
  store(0);
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const bool more = ks + 1 < nk;
    if (more) load(ks + 1);
    compute(ks & 1);
    if (more) store((ks + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: stage fp32 tile in LDS, then coalesced fused stores ----
  float* Cs = (float*)smem;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * (BM / WM) + i * 16 + (lane >> 4) * 4 + r;
        const int col = wn * (BN / WN) + j * 16 + (lane & 15);
        Cs[row * CSTR + col] = acc[i][j][r];
      }
  __syncthreads();
  epilogue_tile<T, BM, BN, 256>(a, Cs, CSTR, m0, n0, tid);
}

// ------------------------------------------------------------------------------------
// Forward / dgrad for narrow convs (Cout <= 64: RCAN / RRDB / SRResNet bodies at W 64 or
// 128).  A block computes 256 consecutive output pixels = R = 256 / W full rows of one image
// x all Cout channels.  Per 64-channel input chunk it stages the halo rows y0-1 .. y0+R,
// cols -1 .. W of that image once in LDS by LDS-DMA (XOR-swizzled 128-B rows, zero padding
// from the range check) and forms all nine taps from it: the A fragment of tap (ty, tx) is
// the row set shifted by ty*(W+2)+tx -- x is read from L2 once per chunk instead of once per
// tap.  Each wave owns CW co tiles x PT pixel tiles and keeps its weights in registers one
// kernel row (3 taps) at a time, the next row in flight, so the weight bytes cross L2 once
// per wave and chunk, not once per tap and pixel tile.  The fp32 tile goes
// through the shared fused epilogue (bias, activation, gate, residuals, pixel shuffle).
// ------------------------------------------------------------------------------------
// DIRECT (CO_T 4, plain store, no colsum): C = W x X^T with the two co tiles of a wave
// row-permuted (tile c row r -> channel 8(r/4) + 4c + r%4), so each lane ends with 8
// consecutive channels of one pixel and the fused epilogue stores 16 B from registers -- no
// LDS staging round trip (which cost ~1/3 of the kernel at nf 64).
template <int CO_T, bool W256 = false, bool DIRECT = false, int HALF = 0>
__global__ __launch_bounds__(256, HALF ? 3 : 2) void conv3x3_fwd_halo_kernel(FwdArgs a) {
  static_assert(!DIRECT || CO_T == 4, "direct epilogue: two co tiles per wave");
  constexpr int BN = CO_T * 16;
  constexpr int CSTR = BN + 4;
  constexpr int CW = CO_T >= 4 ? CO_T / 2 : 1;  // co tiles per wave
  constexpr int WC = CO_T / CW;                  // waves along co
  constexpr int WP = 4 / WC;                     // waves along pixels
  constexpr int PT = 16 / WP;                    // 16-pixel tiles per wave
  // >= (R+2)*(W+2) rounded up to 8: 400 (W 64), 520 (W 128), 776 (W 256: HR-resolution conv_last)
  constexpr int HROWS = W256 ? 776 : 528;
  constexpr int SMEM_H = HROWS * (HALF ? 64 : 128);
  constexpr int SMEM_E = 128 * CSTR * 4;
  constexpr int SMEM = SMEM_H > SMEM_E ? SMEM_H : SMEM_E;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = w % WC, wp = w / WC;
  const int g = lane >> 4, c16 = lane & 15;
  const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (int)tile * 256;
  const int n0 = blockIdx.y * BN;  // co tile (Cout > 64: one block row per 64 output channels)
  const int W = a.W, H = a.H;
  const int WPAD = W + 2;
  const int R = 256 / W;
  const int HR = (R + 2) * WPAD;
  const int q0 = m0 / W;  // n*H + y0
  const int n = q0 / H, y0 = q0 - n * H;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(a.w, a.w_bytes);

  int hb[PT];  // halo row of pixel 16*(PT*wp+i) + c16 at tap (0, 0)
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    const int q = 16 * (PT * wp + i) + c16;
    const int rr = q / W;
    hb[i] = rr * WPAD + (q - rr * W);
  }
  f32x4 acc[PT][CW];
#pragma unroll
  for (int i = 0; i < PT; ++i)
#pragma unroll
    for (int c = 0; c < CW; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lc8 = (lane & 7) ^ (lane >> 3);  // logical 16-B chunk of this lane's DMA slot
  constexpr int CCH = HALF ? 32 : 64;        // channels per chunk
  const int nch = (a.Cin + CCH - 1) / CCH;
  const int ninstr = HALF ? (HR + 15) >> 4 : (HR + 7) >> 3;
  const int rps = a.in_ps > 0 ? a.in_ps : 1;
  for (int ch = 0; ch < nch; ++ch) {
    const int ci0 = ch * CCH;
    if (ch) __syncthreads();  // every wave is done with the previous chunk's halo
    // in_ps = r (pixel-shuffled input: the upsample convs' dgrads): LR channel sl * C' + c of LR pixel
    // (y, x) is channel c of HR pixel (y r + si, x r + sj); a 64-channel chunk lies in one slot
    int si = 0, sj = 0, cch0 = ci0;
    if (a.in_ps > 0) {
      const int sl = (int)fdiv((uint32_t)ci0, a.fd_cps);
      si = sl / rps;
      sj = sl - si * rps;
      cch0 = ci0 - sl * a.fd_cps.d;
    }
    // the chunk's upper 32 channels exist (not for Cin 32: RRDB dense dgrads).  A runtime flag
    // even for Cin 64: measured 2-3 % faster on RCAN / RRDB than the constant-folded form
    const bool khi = !HALF && ci0 + 32 < a.Cin;
    for (int k = w; k < ninstr; k += 4) {
      // HALF: 64-B rows, 4 lanes per row, chunk swizzled by (row >> 2) & 3
      const int hr = HALF ? 16 * k + (lane >> 2) : 8 * k + (lane >> 3);
      const int lc = HALF ? (lane & 3) ^ ((hr >> 2) & 3) : lc8;
      const bool cv = ci0 + lc * 8 < a.Cin;
      const int hy = hr / WPAD, hx = hr - hy * WPAD;
      const int yy = y0 - 1 + hy, xx = hx - 1;
      const bool v = cv && hr < HR && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
      const int pix = a.in_ps > 0 ? ((n * H + yy) * rps + si) * (W * rps) + xx * rps + sj : (n * H + yy) * W + xx;
      const uint32_t off = (uint32_t)((pix * a.ldx + a.xcoff + cch0 + lc * 8) * 2);
      glds16(xr, smem + k * 1024, v ? off : SR_OOB);
    }
    // this wave's weights, one kernel row (3 taps x 2 K halves x CW co tiles) at a time, the
    // next row loaded while the current one computes; row 0 overlaps the halo DMA
    u32x4 bw[2][3][2][CW];
    auto load_row = [&](int ty, u32x4 (&dst)[3][2][CW]) {
#pragma unroll
      for (int tx = 0; tx < 3; ++tx)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int c = 0; c < CW; ++c) {
            const int co = DIRECT ? n0 + wc * CW * 16 + 8 * (c16 >> 2) + 4 * c + (c16 & 3)
                                  : n0 + (wc * CW + c) * 16 + c16;
            const int ci = ci0 + kk * 32 + 8 * g;
            const int tap = ty * 3 + tx;
            const bool v = co < a.Cout && ci < a.Cin;
            if (kk == 0 || khi)
              dst[tx][kk][c] = buf_load16(wr, v ? (uint32_t)((co * a.ldw + tap * a.Cin + ci) * 2) : SR_OOB);
          }
    };
    load_row(0, bw[0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // opaque 0: keeps the 9*2*PT fragment addresses from being hoisted out of the chunk loop
    // as loop invariants (they would pin ~144 VGPRs); recomputing them is ~4 VALU each
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
#pragma unroll
    for (int ty = 0; ty < 3; ++ty) {
      if (ty < 2) load_row(ty + 1, bw[(ty + 1) & 1]);
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        const int toff = ty * WPAD + tx;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          if (kk == 1 && !khi) continue;
#pragma unroll
          for (int i = 0; i < PT; ++i) {
            const uint32_t hrow = hb[i] + z + toff;
            const u32x4 fa = *(const u32x4*)(smem + (HALF ? hrow * 64u + ((g ^ ((hrow >> 2) & 3u)) << 4)
                                                          : swz128(hrow, kk * 4 + g)));
#pragma unroll
            for (int c = 0; c < CW; ++c) {
              if constexpr (DIRECT)
                mfma_chunk<bf16_t>(bw[ty & 1][tx][kk][c], fa, acc[i][c]);
              else
                mfma_chunk<bf16_t>(fa, bw[ty & 1][tx][kk][c], acc[i][c]);
            }
          }
        }
      }
    }
  }

  if constexpr (DIRECT) {
    // lane (g, c16): channels n0 + 32 wc + 8g .. +7 of pixel m0 + 16 (PT wp + i) + c16
    const int nn = n0 + wc * 32 + 8 * g;
    if (nn >= a.Cout) return;
    const __amdgpu_buffer_rsrc_t gr = make_rsrc(a.gate, a.g_bytes);
    const __amdgpu_buffer_rsrc_t rr = make_rsrc(a.res, a.r_bytes);
    const __amdgpu_buffer_rsrc_t rr2 = make_rsrc(a.res2, a.r2_bytes);
    float bv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bv[j] = 0.f;
    if (a.bias) {
      const f32x4 b0 = *(const f32x4*)(a.bias + nn), b1 = *(const f32x4*)(a.bias + nn + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) { bv[j] = b0[j]; bv[4 + j] = b1[j]; }
    }
    const bool gok = a.gate_mode != 2 || (nn >= a.gcol0 && nn < a.gcol1);
    const bool rok = nn < a.rcols;
    auto unpack8 = [](const u32x4& q, float* o) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[2 * j] = bf16_to_f32(q[j] & 0xffff);
        o[2 * j + 1] = bf16_to_f32(q[j] >> 16);
      }
    };
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int m = m0 + 16 * (PT * wp + i) + c16;
      if (m >= a.M) continue;
      u32x4 gv, rv, rv2;
      if (a.gate) gv = buf_load16(gr, gok ? (uint32_t)(((size_t)m * a.ldg + a.gcoff + nn) * 2) : SR_OOB);
      if (a.res) rv = buf_load16(rr, rok ? (uint32_t)(((size_t)m * a.ldr + a.rcoff + nn) * 2) : SR_OOB);
      if (a.res2) rv2 = buf_load16(rr2, rok ? (uint32_t)(((size_t)m * a.ldr2 + a.r2coff + nn) * 2) : SR_OOB);
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) { v[r] = acc[i][0][r] + bv[r]; v[4 + r] = acc[i][1][r] + bv[4 + r]; }
      if (a.aux) {  // activation side output (act_aux_n: GELU' for GELU)
        float ax[8];
        act_aux_n(v, ax, a.act, a.slope);
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(ax[2 * j], ax[2 * j + 1]);
        *(u32x4*)((bf16_t*)a.aux + (size_t)m * a.ldy + a.ycoff + nn) = o;
      } else {
        act_apply_n(v, a.act, a.slope);
      }
      float gf[8];
      if (a.gate) unpack8(gv, gf);
      if (a.gate && a.gate_mode == 1) {  // the stored GELU'
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= gf[j];
      } else if (a.gate && a.gate_mode == 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= gf[j] > 0.f ? 1.f : a.gate_slope;
      }
      const float al = row_alpha(a, m);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= al;
      if (a.res && rok) {
        float rf[8];
        unpack8(rv, rf);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = a.beta * rf[j] + v[j];
      }
      if (a.res2 && rok) {
        float rf[8];
        unpack8(rv2, rf);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = a.beta2 * rf[j] + v[j];
      }
      if (a.gate && a.gate_mode == 2 && gok) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= gf[j] > 0.f ? 1.f : a.gate_slope;
      }
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
      *(u32x4*)((bf16_t*)a.y + (size_t)m * a.ldy + a.ycoff + nn) = o;
    }
    return;
  }
  float* Cs = (float*)smem;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int row = 16 * (PT * wp + i) - 128 * h;  // pixel tile origin inside half h
      if (row >= 0 && row < 128) {
#pragma unroll
        for (int c = 0; c < CW; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(row + 4 * g + r) * CSTR + (wc * CW + c) * 16 + c16] = acc[i][c][r];
      }
    }
    __syncthreads();
    epilogue_tile<bf16_t, 128, BN, 256>(a, Cs, CSTR, m0 + h * 128, n0, tid);
  }
}

template <typename T, int BM, int BN, int WM, int WN>
hipError_t launch_fwd(const FwdArgs& a0, hipStream_t s) {
  FwdArgs a = a0;
  const int tm = (a.M + BM - 1) / BM;
  a.tiles_n = (a.Cout + BN - 1) / BN;
  a.tiles = tm * a.tiles_n;
  hipLaunchKernelGGL((conv3x3_fwd_kernel<T, BM, BN, WM, WN>), dim3(a.tiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_fwd_tile_t(const FwdArgs& a, FwdKind k, hipStream_t s) {
  switch (k) {
case FK_256_16: return launch_fwd<T, 256, 16, 4, 1>(a, s);
case FK_256_32: return launch_fwd<T, 256, 32, 4, 1>(a, s);
case FK_128_64: return launch_fwd<T, 128, 64, 2, 2>(a, s);
default: return launch_fwd<T, 128, 128, 2, 2>(a, s);
  }
}

}  // namespace

namespace sr_conv {

hipError_t launch_fwd_tile(const FwdArgs& a, FwdKind k, bool bf16, hipStream_t s) {
  return bf16 ? launch_fwd_tile_t<bf16_t>(a, k, s) : launch_fwd_tile_t<float>(a, k, s);
}

hipError_t launch_fwd_halo(const FwdArgs& a0, hipStream_t s) {
  FwdArgs a = a0;
  a.tiles_n = (a.Cout + 63) / 64;
  a.tiles = a.M / 256;
  const int ct = (a.Cout + 15) / 16;
  const dim3 grid(a.tiles, a.tiles_n);
  if (a.W == 256) hipLaunchKernelGGL((conv3x3_fwd_halo_kernel<1, true>), grid, dim3(256), 0, s, a);
  else if (ct == 1) hipLaunchKernelGGL(conv3x3_fwd_halo_kernel<1>, grid, dim3(256), 0, s, a);
  else if (ct == 2 && a.in_ps == 0)
    hipLaunchKernelGGL((conv3x3_fwd_halo_kernel<2, false, false, 3>), grid, dim3(256), 0, s, a);
  else if (ct == 2) hipLaunchKernelGGL(conv3x3_fwd_halo_kernel<2>, grid, dim3(256), 0, s, a);
  else if (!a.colsum && !a.out_nchw && a.out_ps == 0)
    hipLaunchKernelGGL((conv3x3_fwd_halo_kernel<4, false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(conv3x3_fwd_halo_kernel<4>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sr_conv
