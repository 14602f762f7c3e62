// 1x1 convs (linears over NHWC tokens): linear_wk_kernel and conv3x3_lin_kernel forward / dgrad, and the weight
// gradient linear_wgrad_kernel, with their launches.
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

// ------------------------------------------------------------------------------------
// linear_wk_kernel<E>: 1x1 convs streamed over K -- the SwinIR fc2 forward (360 -> 184), the fc1 /
// qkv dgrads (360 / 576 -> 184), and (K <= 192) the fc2 / proj dgrads and proj forward.  A block owns
// 128 tokens x one 192-wide tile of the output channels (Cout <= 576: the tiles of one token tile are
// consecutive blocks, so its token rows are read from L2 by the second) and streams K in 64-wide steps
// through two LDS stages (LDS-DMA of the token tile [128][128 B] and the weight tile [192][128 B], both
// K-contiguous, chunk ^ (row & 7) swizzle; 40 KB a stage, so two blocks share a CU).  C = W . X^T as in
// conv3x3_lin_kernel: the weight rows are permuted on load (32-row group p, tile t, row r -> channel
// 32p + 8(r/4) + 4t + r%4), so a lane ends with 8 consecutive channels of one token and stores them as
// one 16-B vector with the fused epilogue.  4 waves (2 channel x 2 token halves), each 96 channels x
// 64 tokens (6 x 4 accumulator tiles).  (The 64-token lin kernel it replaces on wide K re-read the
// whole weight image per 64 tokens -- 434 MB of L2 reads on the qkv dgrad -- and staged all of K
// before its first MFMA.)
// E: conv3x3_lin_kernel's epilogue codes (bits 0-1 act, 2-3 gate 1 / 2 pre-residual, 4 res, 6 aux, 7
// row scale) for 0 (plain), 8 (GELU' gate: fc2 dgrad), 16 (residual), 67 (GELU + pre-activation aux:
// fc1 forward), 144 (residual + row scale); the bias
// (GEMM column order), alpha and beta always.
// ------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(256, 2) void linear_wk_kernel(FwdArgs a) {
  constexpr int XI = 128 * 128, WI = 192 * 128, STAGE = XI + WI;
  constexpr int ACT = E & EPI_ACT, GATE = (E >> EPI_GATE_SHIFT) & EPI_GATE;
  constexpr bool RES = (E & EPI_RES) != 0, AUX = (E & EPI_AUX) != 0, RSC = (E & LIN_RSC) != 0;
  static_assert(GATE != 3 && (E & ~(EPI_ACT | (EPI_GATE << EPI_GATE_SHIFT) | EPI_RES | EPI_AUX | LIN_RSC)) == 0,
                "linear_wk: epilogue subset");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;
  const int nct = (a.Cout + 191) / 192;  // output-channel tiles (consecutive blocks)
  const int bt = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int tt = bt / nct, ct = bt - tt * nct;
  const int m0 = tt * 128, n0 = ct * 192;
  const int K = a.Cin, nk = (K + 63) >> 6;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(a.w, a.w_bytes);

  // DMA pieces of 64 lanes = 8 rows x 8 chunks: per stage 16 token pieces then 24 weight pieces,
  // wave w taking pieces w, w + 4, ...; lane: row rl of the piece, physical chunk pc = logical lc ^ rl
  const int rl = lane >> 3, lc = (lane & 7) ^ rl;
  int wch[6];  // source weight channel of this lane's row in weight pieces q = 4..9
#pragma unroll
  for (int q = 4; q < 10; ++q) {
    const int row = (w + 4 * q - 16) * 8 + rl;
    const int t = (row >> 4) & 1, r = row & 15;
    wch[q - 4] = n0 + (row >> 5) * 32 + 8 * (r >> 2) + 4 * t + (r & 3);
  }
  auto issue = [&](int ks, int stg) {
    char* st = smem + stg * STAGE;
    const int kc = ks * 8 + lc;
    const bool kv = kc * 8 < K;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = w + 4 * q, m = m0 + p * 8 + rl;
      glds16(xr, st + p * 1024, (kv && m < a.M) ? (uint32_t)((m * a.ldx + a.xcoff + kc * 8) * 2) : SR_OOB);
    }
#pragma unroll
    for (int q = 4; q < 10; ++q) {
      const int p = w + 4 * q - 16, ch = wch[q - 4];
      glds16(wrs, st + XI + p * 1024, (kv && ch < a.Cout) ? (uint32_t)((ch * a.ldw + kc * 8) * 2) : SR_OOB);
    }
  };

  const int c16 = lane & 15, g = lane >> 4;
  f32x4 acc[6][4];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto compute = [&](int stg) {
    const char* Xs = smem + stg * STAGE;
    const char* Ws = Xs + XI;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int phys = ((kk * 4 + g) ^ (c16 & 7)) << 4;  // every fragment row has row & 7 == c16 & 7
      u32x4 fa[6], fb[4];
#pragma unroll
      for (int i = 0; i < 6; ++i) fa[i] = *(const u32x4*)(Ws + (wr * 96 + i * 16 + c16) * 128 + phys);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = *(const u32x4*)(Xs + (wc * 64 + j * 16 + c16) * 128 + phys);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, fa[i]),
                                                              __builtin_bit_cast(s16x8, fb[j]), acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  };

  issue(0, 0);
  for (int ks = 0; ks < nk; ++ks) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pp_barrier();  // step ks landed for every wave; step ks - 1's stage is free
    if (ks + 1 < nk) issue(ks + 1, (ks + 1) & 1);
    compute(ks & 1);
  }

  // ---- epilogue: pair P (tiles 2P, 2P + 1) gives channels n = n0 + (3 wr + P) * 32 + 8g .. + 7 of
  // token m0 + 64 wc + 16 j + c16
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(a.res, a.r_bytes);
  const __amdgpu_buffer_rsrc_t gr = make_rsrc(a.gate, a.g_bytes);
  const size_t ybytes = (size_t)a.M * a.ldy * 2;
  const __amdgpu_buffer_rsrc_t yr = make_rsrc(a.y, ybytes < 0x80000000ull ? (uint32_t)ybytes : 0x7fffffffu);
  const __amdgpu_buffer_rsrc_t ar = make_rsrc(a.aux, AUX ? (ybytes < 0x80000000ull ? (uint32_t)ybytes : 0x7fffffffu) : 0u);
  const __amdgpu_buffer_rsrc_t br = make_rsrc(a.bias, a.bias ? (uint32_t)a.Cout * 4u : 0u);
  float alpha_blk = a.alpha;
  if constexpr (RSC) alpha_blk = a.alpha * a.row_scale[fdiv((uint32_t)m0, a.fd_hw)];
  u32x4 rv[3][4], gv[3][4];
  float bv[3][8];
#pragma unroll
  for (int P = 0; P < 3; ++P) {
    const int n = n0 + (3 * wr + P) * 32 + 8 * g;
    const u32x4 b0 = buf_load16(br, (uint32_t)n * 4u), b1 = buf_load16(br, (uint32_t)n * 4u + 16u);
#pragma unroll
    for (int r = 0; r < 4; ++r) { bv[P][r] = __uint_as_float(b0[r]); bv[P][4 + r] = __uint_as_float(b1[r]); }
    if constexpr (GATE != 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wc * 64 + j * 16 + c16;
        gv[P][j] = buf_load16(gr, (n < a.Cout && m < a.M) ? (uint32_t)(((size_t)m * a.ldg + a.gcoff + n) * 2) : SR_OOB);
      }
    }
    if constexpr (RES) {
      const bool rok = n < a.Cout && n < a.rcols;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int m = m0 + wc * 64 + j * 16 + c16;
        rv[P][j] = buf_load16(rr, (rok && m < a.M) ? (uint32_t)(((size_t)m * a.ldr + a.rcoff + n) * 2) : SR_OOB);
      }
    }
  }
#pragma unroll
  for (int P = 0; P < 3; ++P) {
    const int n = n0 + (3 * wr + P) * 32 + 8 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = m0 + wc * 64 + j * 16 + c16;
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        v[r] = acc[2 * P][j][r] + bv[P][r];
        v[4 + r] = acc[2 * P + 1][j][r] + bv[P][4 + r];
      }
      if constexpr (AUX) {  // activation side output (act_aux_n: GELU' for GELU)
        float ax[8];
        act_aux_n(v, ax, ACT, a.slope);
        u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = pack_bf16x2(ax[2 * q], ax[2 * q + 1]);
        __builtin_amdgcn_raw_buffer_store_b128(o, ar, (n < a.Cout && m < a.M) ? (uint32_t)(((size_t)m * a.ldy + a.ycoff + n) * 2) : SR_OOB, 0, 0);
      } else if constexpr (ACT == 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = v[q] > 0.f ? v[q] : 0.f;
      } else if constexpr (ACT == 2) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = v[q] > 0.f ? v[q] : v[q] * a.slope;
      } else if constexpr (ACT == 3) {
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = gelu_exact(v[q]);
      }
      if constexpr (GATE != 0) {
        float gf[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          gf[2 * q] = bf16_to_f32(gv[P][j][q] & 0xffff);
          gf[2 * q + 1] = bf16_to_f32(gv[P][j][q] >> 16);
        }
        if constexpr (GATE == 1) {
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] *= gf[q] > 0.f ? 1.f : a.gate_slope;
        } else {  // the stored GELU' (the forward's aux)
#pragma unroll
          for (int q = 0; q < 8; ++q) v[q] *= gf[q];
        }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] *= alpha_blk;
      if constexpr (RES) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          v[2 * q] += a.beta * bf16_to_f32(rv[P][j][q] & 0xffff);
          v[2 * q + 1] += a.beta * bf16_to_f32(rv[P][j][q] >> 16);
        }
      }
      u32x4 o;
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = pack_bf16x2(v[2 * q], v[2 * q + 1]);
      __builtin_amdgcn_raw_buffer_store_b128(o, yr, (n < a.Cout && m < a.M) ? (uint32_t)(((size_t)m * a.ldy + a.ycoff + n) * 2) : SR_OOB, 0, 0);
    }
  }
}

// ------------------------------------------------------------------------------------
// conv3x3_lin_kernel<MT>: 1x1 convs (nn.Linear over NHWC tokens: SwinIR qkv / proj / fc1 /
// fc2 and their dgrads, DCN column GEMMs) with a short K (<= 576).  These GEMMs are
// HBM-bound (AI ~ 100-150 FLOP/B); the 2-D tiled kernels re-read the token rows once per
// N tile and pay a full prologue / epilogue per 2-3 K-steps.  Here a block loads its MT
// token rows x all K ONCE into LDS (LDS-DMA, [K/64][MT][128 B] XOR-swizzled) and then
// sweeps every output channel, 128 per pass (32 per wave): W fragments come from L2
// straight into registers, X^T fragments from LDS, C = W x X^T so each lane ends with 8
// consecutive channels of one token (the W tile rows are permuted on load: tile t row r ->
// channel 8(r/4) + 4t + r%4) and stores 16 B directly, with the fused epilogue (bias,
// activation, pre-activation side output, gate, alpha, residuals) in registers.
// ------------------------------------------------------------------------------------
// E >= 0: the epilogue fixed at compile time (bits 0-1 act, 2-3 gate 0 none / 1 pre-residual
// (g > 0 ? 1 : gate_slope) / 2 pre-residual GELU'(g) / 3 post-residual on gcol0..gcol1, 4 res,
// 5 res2, 6 aux, 7 row_scale, uniform per block: H*W % MT == 0): its operand loads for a pass are
// issued before the pass's MFMAs, so they land under them; E = -1: run-time flags, loads next to
// their use (every combination).
template <int MT, int MAXCG, int NPASS, int E, bool LN = false>
__global__ __launch_bounds__(256, 2) void conv3x3_lin_kernel(FwdArgs a) {
  constexpr int NMT = MT / 16;  // token tiles per wave (every wave covers all MT tokens)
  constexpr bool CE = E >= 0;
  constexpr int ACT = E & EPI_ACT, GATE = (E >> EPI_GATE_SHIFT) & EPI_GATE;
  constexpr bool RES = (E & EPI_RES) != 0, RES2 = (E & EPI_RES2) != 0, AUX = (E & EPI_AUX) != 0, RSC = (E & LIN_RSC) != 0;
  __shared__ __attribute__((aligned(16))) char smem[MAXCG * MT * 128];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, c16 = lane & 15;
  const int m0 = (int)xcd_remap(blockIdx.x, gridDim.x) * MT;
  const int K = a.Cin, KC = K >> 3;  // 16-B chunks of a token row
  const int CG = (K + 63) >> 6;      // 128-B chunk groups
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(a.w, a.w_bytes);

  __shared__ float sgb[LN ? 2 * 192 : 1];  // LN: gamma, beta (channels < 192)
  if constexpr (LN) {
    for (int c = tid; c < 192; c += 256) {
      sgb[c] = c < a.ln_C ? a.ln_g[c] : 0.f;
      sgb[192 + c] = c < a.ln_C ? a.ln_b[c] : 0.f;
    }
  }
  // ---- stage the MT x K token tile: piece p = (chunk group cg, 8-row group rg)
  {
    const int npieces = CG * (MT / 8);
    const int rl = lane >> 3, pc = lane & 7;
    const int lc = pc ^ rl;  // logical chunk this lane fetches (row & 7 == rl)
    for (int p = w; p < npieces; p += 4) {
      const int cg = p / (MT / 8), rg = p - cg * (MT / 8);
      const int row = rg * 8 + rl, m = m0 + row, ch = cg * 8 + lc;
      const bool v = m < a.M && ch < KC;
      glds16(xr, smem + (cg * MT + rg * 8) * 128, v ? (uint32_t)(((size_t)m * a.ldx + a.xcoff + ch * 8) * 2) : SR_OOB);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
  if constexpr (LN) {
    // LayerNorm of the staged rows in place (fp32 statistics, two lanes per row over alternate
    // 16-B chunks held in registers: one LDS read per chunk), gamma / beta from LDS, the
    // normalised rows also stored to ln_out with the row mean / rstd: the standalone LN kernel's
    // read of x and this kernel's read of its output become one read
    constexpr int MAXQ = MAXCG * 4;  // chunks per lane (2 lanes per row, MAXCG * 8 chunks)
    const int row = tid >> 1, half = tid & 1, m = m0 + row;
    auto chunk_ptr = [&](int ch) -> u32x4* {
      return (u32x4*)(smem + (ch >> 3) * MT * 128 + row * 128 + (((ch & 7) ^ (row & 7)) << 4));
    };
    u32x4 raw[MAXQ];
    float sm = 0.f;
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
      const int ch = half + 2 * q;
      raw[q] = ch < KC ? *chunk_ptr(ch) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = ch * 8 + 2 * j;
        sm += (c < a.ln_C ? bf16_to_f32(raw[q][j] & 0xffff) : 0.f) + (c + 1 < a.ln_C ? bf16_to_f32(raw[q][j] >> 16) : 0.f);
      }
    }
    sm += __shfl_xor(sm, 1);
    const float mu = sm / a.ln_C;
    float sq = 0.f;
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
      const int ch = half + 2 * q;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = ch * 8 + 2 * j;
        const float d0 = c < a.ln_C ? bf16_to_f32(raw[q][j] & 0xffff) - mu : 0.f;
        const float d1 = c + 1 < a.ln_C ? bf16_to_f32(raw[q][j] >> 16) - mu : 0.f;
        sq += d0 * d0 + d1 * d1;
      }
    }
    sq += __shfl_xor(sq, 1);
    const float rs = rsqrtf(sq / a.ln_C + a.ln_eps);
    __syncthreads();  // gamma / beta staged (below the token DMA wait) by every wave
#pragma unroll
    for (int q = 0; q < MAXQ; ++q) {
      const int ch = half + 2 * q;
      if (ch >= KC) break;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = ch * 8 + j;
        const float xv = bf16_to_f32((raw[q][j >> 1] >> (16 * (j & 1))) & 0xffff);
        o[j] = c < a.ln_C ? (xv - mu) * rs * sgb[c] + sgb[192 + c] : 0.f;
      }
      u32x4 r;
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = pack_bf16x2(o[2 * j], o[2 * j + 1]);
      *chunk_ptr(ch) = r;
      if (m < a.M) *(u32x4*)((bf16_t*)a.ln_out + (size_t)m * K + ch * 8) = r;
    }
    if (half == 0 && m < a.M) {
      a.ln_mean[m] = mu;
      a.ln_rstd[m] = rs;
    }
    __syncthreads();
  }

  const __amdgpu_buffer_rsrc_t gr = make_rsrc(a.gate, a.g_bytes);
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(a.res, a.r_bytes);
  const __amdgpu_buffer_rsrc_t rr2 = make_rsrc(a.res2, a.r2_bytes);
  // output descriptors sized to the output (a lane past it stores at SR_OOB = 2^31, which must
  // fall outside the descriptor to be dropped)
  const size_t ybytes = (size_t)a.M * a.ldy * 2;
  const uint32_t yb = ybytes < 0x80000000ull ? (uint32_t)ybytes : 0x7fffffffu;
  const __amdgpu_buffer_rsrc_t yr = make_rsrc(a.y, yb);
  const __amdgpu_buffer_rsrc_t ar = make_rsrc(a.aux, a.aux ? yb : 0u);
  // compile-time epilogue: the block's row scale (all MT tokens in one image)
  float alpha_blk = a.alpha;
  if constexpr (CE && RSC) alpha_blk = a.alpha * a.row_scale[fdiv((uint32_t)m0, a.fd_hw)];
  const int nkk = (K + 31) >> 5;
  constexpr int npass = NPASS;  // (Cout + 127) / 128, fixed so the pass loop unrolls: the
  // compiler's own vmcnt waits are then exact (a rolled loop waited vmcnt(0) for the W loads,
  // i.e. for the previous pass's output stores too)
  constexpr int MAXKK = MAXCG * 2;
  // W fragments of a whole pass (all K) in registers, the next pass's loads in flight while the
  // current pass computes: an L2 round trip per K-step would otherwise set the pace
  u32x4 wb[MAXKK][2];
  auto wload_pass = [&](int pass) {
    const int r0 = pass * 128 + w * 32 + 8 * (c16 >> 2) + (c16 & 3);
    const bool wv0 = r0 < a.Cout, wv1 = r0 + 4 < a.Cout;
#pragma unroll
    for (int kk = 0; kk < MAXKK; ++kk) {
      const int k = kk * 32 + 8 * g;
      const bool kv = kk < nkk && k < K;
      wb[kk][0] = buf_load16(wr, (wv0 && kv) ? (uint32_t)((r0 * a.ldw + k) * 2) : SR_OOB);
      wb[kk][1] = buf_load16(wr, (wv1 && kv) ? (uint32_t)(((r0 + 4) * a.ldw + k) * 2) : SR_OOB);
    }
  };
  // the bias of every pass up front: a load in the epilogue would queue behind the next pass's
  // W loads (vector memory completes in order), exposing their latency per pass
  // (buffer loads, no branch: a missing bias or channels past Cout read zeros)
  const __amdgpu_buffer_rsrc_t br = make_rsrc(a.bias, a.bias ? (uint32_t)a.Cout * 4u : 0u);
  float bva[NPASS][8];
#pragma unroll
  for (int pass = 0; pass < NPASS; ++pass) {
    const uint32_t n = (uint32_t)(pass * 128 + w * 32 + 8 * g);
    const u32x4 b0 = buf_load16(br, n * 4u), b1 = buf_load16(br, n * 4u + 16u);
#pragma unroll
    for (int j = 0; j < 4; ++j) { bva[pass][j] = __uint_as_float(b0[j]); bva[pass][4 + j] = __uint_as_float(b1[j]); }
  }
  wload_pass(0);
#pragma unroll
  for (int pass = 0; pass < npass; ++pass) {
    const int nb = pass * 128 + w * 32;  // this wave's 32 channels (tile t row r -> nb + 8(r/4) + 4t + r%4)
    const int n = nb + 8 * g;
    const bool nok = n < a.Cout;
    // compile-time epilogue operands of this pass, issued now so they land under the MFMAs
    // (out-of-range lanes read zeros: buffer offsets past the descriptor)
    u32x4 gv[NMT], rv[NMT], rv2[NMT];
    if constexpr (CE) {
      const bool gok = nok && (GATE != 3 || (n >= a.gcol0 && n < a.gcol1));
      const bool rok = nok && n < a.rcols;
#pragma unroll
      for (int i = 0; i < NMT; ++i) {
        const int m = m0 + i * 16 + c16;
        const bool mok = m < a.M;
        if constexpr (GATE != 0)
          gv[i] = buf_load16(gr, (mok && gok) ? (uint32_t)(((size_t)m * a.ldg + a.gcoff + n) * 2) : SR_OOB);
        if constexpr (RES)
          rv[i] = buf_load16(rr, (mok && rok) ? (uint32_t)(((size_t)m * a.ldr + a.rcoff + n) * 2) : SR_OOB);
        if constexpr (RES2)
          rv2[i] = buf_load16(rr2, (mok && rok) ? (uint32_t)(((size_t)m * a.ldr2 + a.r2coff + n) * 2) : SR_OOB);
      }
    }
    f32x4 acc[NMT][2];
#pragma unroll
    for (int i = 0; i < NMT; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < MAXKK; ++kk) {
      // a guarded body, not a break: with MAXKK 12 / 18 (wide K) a break left the loop rolled and
      // the W fragments indexed dynamically (in scratch)
      if (kk < nkk) {
      const int ch = kk * 4 + g;  // logical 16-B chunk of the X^T fragment
      // [cg][row][128 B], physical chunk = logical ^ (row & 7); row & 7 == c16 & 7 for all i
      const char* base = smem + (ch >> 3) * MT * 128 + c16 * 128 + ((((ch & 7) ^ (c16 & 7))) << 4);
      // all NMT fragments of the K step first (in flight together), then the MFMAs
      u32x4 xf[NMT];
#pragma unroll
      for (int i = 0; i < NMT; ++i) xf[i] = *(const u32x4*)(base + i * 16 * 128);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < NMT; ++i) {
        acc[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wb[kk][0]),
                                                            __builtin_bit_cast(s16x8, xf[i]), acc[i][0], 0, 0, 0);
        acc[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(s16x8, wb[kk][1]),
                                                            __builtin_bit_cast(s16x8, xf[i]), acc[i][1], 0, 0, 0);
      }
      }
    }
    // the next pass's W fragments load while this pass's epilogue runs
    if (pass + 1 < npass) wload_pass(pass + 1);
    // ---- epilogue: lane (g, c16) holds channels nb + 8g .. +7 of token m0 + 16i + c16 and
    // stores them as one 16-B vector (4 lanes cover 64 contiguous bytes of a token row;
    // staging whole rows through LDS measured slower: 78 -> 95 us on the qkv shape)
    const float* bv = bva[pass];
    if constexpr (CE) {
      // branch-free over lanes: stores of out-of-range lanes go past the buffer descriptor
#pragma unroll
      for (int i = 0; i < NMT; ++i) {
        const int m = m0 + i * 16 + c16;
        const bool ok = nok && m < a.M;
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { v[r] = acc[i][0][r] + bv[r]; v[4 + r] = acc[i][1][r] + bv[4 + r]; }
        if constexpr (AUX) {  // activation side output (act_aux_n: GELU' for GELU)
          float ax[8];
          act_aux_n(v, ax, ACT, a.slope);
          u32x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(ax[2 * j], ax[2 * j + 1]);
          __builtin_amdgcn_raw_buffer_store_b128(o, ar,
                                                 ok ? (uint32_t)(((size_t)m * a.ldy + a.ycoff + n) * 2) : SR_OOB, 0, 0);
        } else if constexpr (ACT == 1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = v[j] > 0.f ? v[j] : 0.f;
        } else if constexpr (ACT == 2) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = v[j] > 0.f ? v[j] : v[j] * a.slope;
        } else if constexpr (ACT == 3) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = gelu_exact(v[j]);
        }
        float gf[8];
        if constexpr (GATE != 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            gf[2 * j] = bf16_to_f32(gv[i][j] & 0xffff);
            gf[2 * j + 1] = bf16_to_f32(gv[i][j] >> 16);
          }
        }
        if constexpr (GATE == 1) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= gf[j] > 0.f ? 1.f : a.gate_slope;
        } else if constexpr (GATE == 2) {  // the stored GELU' (the forward's aux)
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= gf[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= alpha_blk;
        if constexpr (RES) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[2 * j] += a.beta * bf16_to_f32(rv[i][j] & 0xffff);
            v[2 * j + 1] += a.beta * bf16_to_f32(rv[i][j] >> 16);
          }
        }
        if constexpr (RES2) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[2 * j] += a.beta2 * bf16_to_f32(rv2[i][j] & 0xffff);
            v[2 * j + 1] += a.beta2 * bf16_to_f32(rv2[i][j] >> 16);
          }
        }
        if constexpr (GATE == 3) {
          if (n >= a.gcol0 && n < a.gcol1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] *= gf[j] > 0.f ? 1.f : a.gate_slope;
          }
        }
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
        __builtin_amdgcn_raw_buffer_store_b128(o, yr,
                                               ok ? (uint32_t)(((size_t)m * a.ldy + a.ycoff + n) * 2) : SR_OOB, 0, 0);
      }
      continue;
    }
    if (!nok) continue;
#pragma unroll
    for (int i = 0; i < NMT; ++i) {  // fully unrolled: acc must stay register-indexed (no scratch)
      const int m = m0 + i * 16 + c16;
      if (m >= a.M) continue;
      u32x4 gv1, rv1, rv21;
      const bool rok = n < a.rcols;
      if (a.gate) gv1 = buf_load16(gr, (a.gate_mode != 2 || (n >= a.gcol0 && n < a.gcol1))
                                           ? (uint32_t)(((size_t)m * a.ldg + a.gcoff + n) * 2) : SR_OOB);
      if (a.res) rv1 = buf_load16(rr, rok ? (uint32_t)(((size_t)m * a.ldr + a.rcoff + n) * 2) : SR_OOB);
      if (a.res2) rv21 = buf_load16(rr2, rok ? (uint32_t)(((size_t)m * a.ldr2 + a.r2coff + n) * 2) : SR_OOB);
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) { v[r] = acc[i][0][r] + bv[r]; v[4 + r] = acc[i][1][r] + bv[4 + r]; }
      if (a.aux) {  // activation side output (act_aux_n: GELU' for GELU)
        float ax[8];
        act_aux_n(v, ax, a.act, a.slope);
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(ax[2 * j], ax[2 * j + 1]);
        *(u32x4*)((bf16_t*)a.aux + (size_t)m * a.ldy + a.ycoff + n) = o;
      } else {
        act_apply_n(v, a.act, a.slope);
      }
      if (a.gate && a.gate_mode != 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float g0 = bf16_to_f32(gv1[j] & 0xffff), g1 = bf16_to_f32(gv1[j] >> 16);
          if (a.gate_mode == 1) {  // the stored GELU'
            v[2 * j] *= g0;
            v[2 * j + 1] *= g1;
          } else {
            v[2 * j] *= g0 > 0.f ? 1.f : a.gate_slope;
            v[2 * j + 1] *= g1 > 0.f ? 1.f : a.gate_slope;
          }
        }
      }
      const float al = row_alpha(a, m);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= al;
      if (a.res) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[2 * j] += a.beta * bf16_to_f32(rv1[j] & 0xffff);
          v[2 * j + 1] += a.beta * bf16_to_f32(rv1[j] >> 16);
        }
      }
      if (a.res2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[2 * j] += a.beta2 * bf16_to_f32(rv21[j] & 0xffff);
          v[2 * j + 1] += a.beta2 * bf16_to_f32(rv21[j] >> 16);
        }
      }
      if (a.gate && a.gate_mode == 2 && n >= a.gcol0 && n < a.gcol1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[2 * j] *= bf16_to_f32(gv1[j] & 0xffff) > 0.f ? 1.f : a.gate_slope;
          v[2 * j + 1] *= bf16_to_f32(gv1[j] >> 16) > 0.f ? 1.f : a.gate_slope;
        }
      }
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
      *(u32x4*)((bf16_t*)a.y + (size_t)m * a.ldy + a.ycoff + n) = o;
    }
  }
}

// ------------------------------------------------------------------------------------
// Weight gradient of a 1x1 conv (the SwinIR linears: dW[co][ci] = sum_t dy[t][co] x[t][ci] over
// the tokens t, db[co] = sum_t dy[t][co]), bf16.  A block owns a 192 (co) x 192 (ci) tile over a
// token K-range (split-K): SwinIR-M's 576 / 184 / 360 / 192 channel counts are 3 / 1 / 2 / 1 such
// tiles (4-7 % padding, against 28-50 % in 256x256 tiles).  A 64-token K-step is six [64 tok][64 ch]
// LDS images (128-B rows; 32-B blocks XOR-swizzled by row bits 1 and 3, so the 8 rows a 32-lane
// half reads with ds_read_b64_tr_b16 land on 8 distinct bank groups): dy co sub-tiles 0-2, then x ci
// sub-tiles 0-2, DMA'd straight to LDS (wave w: rows 8w .. 8w + 7 of each, the swizzle applied to
// the lane's source channels).  Three stages, two steps in flight, one barrier per step.  8 waves
// (2 co x 4 ci), each 96 co x 48 ci (6 x 3 accumulator tiles).  Blocks of the first ci tile also
// sum dy against a ones operand for the bias (wave (wr, wc): co fragments wc and wc + 4).  Output:
// the pp kernel's fp32 slab ws[split][Cout][Cin] and bias slab (same reduce).
// ------------------------------------------------------------------------------------
SR_DEV uint32_t swz_tr128(uint32_t row, uint32_t byte_in_row) {
  const uint32_t g = ((row >> 1) & 1u) | (((row >> 3) & 1u) << 1);
  return row * 128u + ((((byte_in_row >> 5) ^ g) & 3u) << 5) + (byte_in_row & 31u);
}

__global__ __launch_bounds__(512) void linear_wgrad_kernel(WgArgs a) {
  constexpr int IMG = 8192;       // [64 tok][64 ch] bf16
  constexpr int STAGE = 6 * IMG;  // 48 KB
  constexpr int NST = 3;
  __shared__ __attribute__((aligned(16))) char smem[NST * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 2, wc = w & 3;
  const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
  const int ntile = a.tiles_co * a.tiles_ci;
  const int split = (int)b / ntile;
  const int rem = (int)b - split * ntile;
  const int cot = rem / a.tiles_ci, cit = rem - cot * a.tiles_ci;
  const int co0 = cot * 192, ci0 = cit * 192;
  const int p_begin = split * a.kper;
  const int p_end = min(a.M, p_begin + a.kper);
  const int nk = (p_end - p_begin + 63) / 64;
  const __amdgpu_buffer_rsrc_t dyr = make_rsrc(a.dy, a.dy_bytes);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);

  // DMA lane geometry: image row drow, physical 16-B slot lane & 7 = logical 32-B block
  // ((lane & 7) >> 1) ^ g(drow), half lane & 1
  const int drow = 8 * w + (lane >> 3);
  const int gsw = ((drow >> 1) & 1) | (((drow >> 3) & 1) << 1);
  const int lch = ((((lane & 7) >> 1) ^ gsw) << 4) + (lane & 1) * 8;
  uint32_t offy[3], offx[3];
  bool vy[3], vx[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int co = co0 + i * 64 + lch, ci = ci0 + i * 64 + lch;
    vy[i] = co < a.Cout;
    vx[i] = ci < a.Cin;
    offy[i] = (uint32_t)((drow * a.ldy + a.ycoff + co) * 2);
    offx[i] = (uint32_t)((drow * a.ldx + a.xcoff + ci) * 2);
  }
  auto issue = [&](int ks, int stg) {
    const int p0 = p_begin + ks * 64;
    char* st = smem + stg * STAGE + w * 1024;
    const bool tv = p0 + drow < p_end;
    const uint32_t by = (uint32_t)p0 * (uint32_t)a.ldy * 2u, bx = (uint32_t)p0 * (uint32_t)a.ldx * 2u;
#pragma unroll
    for (int i = 0; i < 3; ++i) glds16(dyr, st + i * IMG, tv && vy[i] ? by + offy[i] : SR_OOB);
#pragma unroll
    for (int i = 0; i < 3; ++i) glds16(xr, st + (3 + i) * IMG, tv && vx[i] ? bx + offx[i] : SR_OOB);
  };

  const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  auto tr8 = [&](const char* img, int r0, int col) -> s16x8 {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + swz_tr128(r0, col * 2)));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + swz_tr128(r0 + 4, col * 2)));
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  f32x4 acc[6][3];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const bool bias_here = a.wsb != nullptr && cit == 0;
  const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};

  auto compute = [&](int stg) {
    const char* st = smem + stg * STAGE;
    s16x8 fa[2][6], fb[2][3];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int r0 = kk * 32 + 8 * tg + tq;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const int c = wr * 96 + i * 16;
        fa[kk][i] = tr8(st + (c >> 6) * IMG, r0, (c & 63) + 4 * tp);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int c = wc * 48 + j * 16;
        fb[kk][j] = tr8(st + (3 + (c >> 6)) * IMG, r0, (c & 63) + 4 * tp);
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][i], fb[kk][j], acc[i][j], 0, 0, 0);
      if (bias_here) {
        // co fragments wc and wc + 4 of this wave's row block (wave-uniform branches: no indexed
        // fragment array, which would go to scratch)
        if (wc == 0) {
          accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][0], ones, accb[0], 0, 0, 0);
          accb[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][4], ones, accb[1], 0, 0, 0);
        } else if (wc == 1) {
          accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][1], ones, accb[0], 0, 0, 0);
          accb[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][5], ones, accb[1], 0, 0, 0);
        } else if (wc == 2) {
          accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][2], ones, accb[0], 0, 0, 0);
        } else {
          accb[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][3], ones, accb[0], 0, 0, 0);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  if (nk > 0) issue(0, 0);
  if (nk > 1) issue(1, 1);
  int stg = 0;
  for (int t = 0; t < nk; ++t) {
    if (t + 1 < nk)
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pp_barrier();  // step t landed for every wave; every wave finished reading step t - 1's stage
    if (t + 2 < nk) issue(t + 2, stg == 0 ? 2 : stg - 1);
    compute(stg);
    stg = stg == 2 ? 0 : stg + 1;
  }

  float* ws = a.ws + (size_t)split * a.Cout * a.Cin;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wr * 96 + i * 16 + (lane >> 4) * 4 + r;
        const int ci = ci0 + wc * 48 + j * 16 + (lane & 15);
        if (co < a.Cout && ci < a.Cin) ws[(size_t)co * a.Cin + ci] = acc[i][j][r];
      }
  if (bias_here && (lane & 15) == 0) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int i = k == 0 ? wc : wc + 4;
      if (i < 6) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = co0 + wr * 96 + i * 16 + (lane >> 4) * 4 + r;
          if (co < a.Cout) a.wsb[(size_t)split * a.Cout + co] = accb[k][r];
        }
      }
    }
  }
}

}  // namespace

namespace sr_conv {

// The forward / dgrad launch of a call on the linear kernels (FK_LIN).
hipError_t launch_lin(const FwdArgs& a, hipStream_t s) {
  FwdArgs b = a;
  const int e = lin_epi(a);
  if (lin_use_wk(a)) {  // 128-token x 192-channel tiles, K streamed
    const dim3 grid(((a.M + 127) / 128) * ((a.Cout + 191) / 192));
    if (e == 0) hipLaunchKernelGGL(linear_wk_kernel<0>, grid, dim3(256), 0, s, b);
    else if (e == 8) hipLaunchKernelGGL(linear_wk_kernel<8>, grid, dim3(256), 0, s, b);
    else if (e == 67) hipLaunchKernelGGL(linear_wk_kernel<67>, grid, dim3(256), 0, s, b);
    else if (e == 16) hipLaunchKernelGGL(linear_wk_kernel<16>, grid, dim3(256), 0, s, b);
    else hipLaunchKernelGGL(linear_wk_kernel<144>, grid, dim3(256), 0, s, b);
    return hipGetLastError();
  }
  if (a.Cin > 192) {  // wide K: 64-token tiles, the whole K (<= 384 / 576) staged
    b.tiles = (a.M + 63) / 64;
#define SR_LINW_E(CG_, NP_, E_) \
  case E_: hipLaunchKernelGGL((conv3x3_lin_kernel<64, CG_, NP_, E_>), dim3(b.tiles), dim3(256), 0, s, b); break;
#define SR_LINW(CG_, NP_) \
  case NP_: \
switch (e) { \
  SR_LINW_E(CG_, NP_, 0) SR_LINW_E(CG_, NP_, 16) SR_LINW_E(CG_, NP_, 144) \
  default: hipLaunchKernelGGL((conv3x3_lin_kernel<64, CG_, NP_, -1>), dim3(b.tiles), dim3(256), 0, s, b); \
} \
break;
    if (a.Cin <= 384) {
      switch ((a.Cout + 127) / 128) { SR_LINW(6, 1) SR_LINW(6, 2) SR_LINW(6, 3) default: return hipErrorInvalidValue; }
    } else {
      switch ((a.Cout + 127) / 128) { SR_LINW(9, 1) SR_LINW(9, 2) SR_LINW(9, 3) default: return hipErrorInvalidValue; }
    }
#undef SR_LINW
#undef SR_LINW_E
    return hipGetLastError();
  }
  b.tiles = (a.M + 127) / 128;
#define SR_LIN_E(NP_, E_) \
  case E_: hipLaunchKernelGGL((conv3x3_lin_kernel<128, 3, NP_, E_>), dim3(b.tiles), dim3(256), 0, s, b); break;
#define SR_LIN(NP_) \
  case NP_: \
switch (e) { \
  SR_LIN_E(NP_, 0) SR_LIN_E(NP_, 8) SR_LIN_E(NP_, 16) SR_LIN_E(NP_, 67) SR_LIN_E(NP_, 144) \
  default: hipLaunchKernelGGL((conv3x3_lin_kernel<128, 3, NP_, -1>), dim3(b.tiles), dim3(256), 0, s, b); \
} \
break;
  switch ((a.Cout + 127) / 128) {
    SR_LIN(1) SR_LIN(2) SR_LIN(3) SR_LIN(4) SR_LIN(5)
    default: return hipErrorInvalidValue;
  }
#undef SR_LIN
#undef SR_LIN_E
  return hipGetLastError();
}

// sr_linear_ln_fwd's launch: the 128-token lin kernel with the LayerNorm prologue, epilogue code e (0 or 67).
int launch_lin_ln(const FwdArgs& a, int e, hipStream_t s) {
#define SR_LNL(NP_)                                                                                       \
  case NP_:                                                                                               \
    if (e == 0) hipLaunchKernelGGL((conv3x3_lin_kernel<128, 3, NP_, 0, true>), dim3(a.tiles), dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((conv3x3_lin_kernel<128, 3, NP_, 67, true>), dim3(a.tiles), dim3(256), 0, s, a); \
    break;
  switch ((a.Cout + 127) / 128) {
    SR_LNL(1) SR_LNL(2) SR_LNL(3) SR_LNL(4) SR_LNL(5)
    default: return sr_fail(SR_EINVAL, "linear_ln_fwd: Cout > 640");
  }
#undef SR_LNL
  return sr_check(hipGetLastError(), "linear_ln_fwd launch");
}

hipError_t launch_wg_lin(WgArgs a, hipStream_t s) {
  const int S = a.splits;
  a.tiles_co = (a.Cout + 191) / 192;
  a.tiles_ci = (a.Cin + 191) / 192;
  hipLaunchKernelGGL(linear_wgrad_kernel, dim3(S * a.tiles_co * a.tiles_ci), dim3(512), 0, s, a);
  return hipGetLastError();
}

}  // namespace sr_conv
