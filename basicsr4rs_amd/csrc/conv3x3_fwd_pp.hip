// conv3x3 forward / dgrad on 256 x 256 tiles (bf16, Cout >= 256 or a wide 1x1): the two-barrier kernel
// conv3x3_fwd_big_kernel, the phase-interleaved conv3x3_fwd_pp_kernel and its halo-row form
// conv3x3_fwd_pph_kernel (whole-row tiles, 64-px column strips, persistent blocks), with their launches.
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

// ------------------------------------------------------------------------------------
// 256 x 256 tile forward / dgrad kernel for bf16 with Cout >= 256 (EDSR-L body and
// upsample convs).  8 waves as 2 (M) x 4 (N), each wave a 128 x 64 output sub-tile
// (8 x 4 v_mfma_f32_16x16x32_bf16 accumulators).  Operands go HBM/L2 -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds: no VGPR staging, the range check zero-fills the padding),
// two 64 KB stages in flight, each retired by a counted `s_waitcnt vmcnt` + raw s_barrier
// (cdna_hip_programming.md §5 "Pipelining across barriers").  The DMA image is lane-linear,
// so the XOR swizzle of the ds_read_b128 fragment reads is applied to the per-lane SOURCE
// chunk (rule 21).  Epilogue: the fp32 tile is staged through LDS in two 128-row halves.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void conv3x3_fwd_big_kernel(FwdArgs a) {
  constexpr int MI = 8, NI = 4;
  constexpr int CSTR = 256 + 4;
  constexpr int SMEM = 128 * CSTR * 4;  // epilogue half tile; >= 2 stages of 64 KB
  static_assert(SMEM >= 2 * BIG_STAGE, "LDS too small");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;
  const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (int)(tile / a.tiles_n) * 256;
  const int n0 = (int)(tile % a.tiles_n) * 256;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(a.w, a.w_bytes);

  // DMA image rows of this lane: w*32 + j*8 + (lane>>3), j = 0..3; logical 16-B chunk c
  const int c = (lane & 7) ^ (lane >> 3);
  int ay[4], ax[4], anh[4];
  uint32_t boff[4];
  bool bval[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = w * 32 + j * 8 + (lane >> 3);
    const int m = m0 + r;
    if (m < a.M) {
      uint32_t q = fdiv((uint32_t)m, a.fd_W);
      ax[j] = m - (int)q * a.W;
      uint32_t n = fdiv(q, a.fd_H);
      ay[j] = (int)q - (int)n * a.H;
      anh[j] = (int)n * a.H;
    } else {
      ax[j] = 0; ay[j] = -100000; anh[j] = 0;
    }
    const int n = n0 + r;
    bval[j] = n < a.Cout;
    boff[j] = (uint32_t)(n * a.ldw) * 2u + (uint32_t)c * 16u;
  }

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (a.nkc + 7) >> 3;

  auto issue = [&](int ks, int buf) {
    const int q = ks * 8 + c;
    const int tap_i = (int)fdiv((uint32_t)q, a.fd_cpt);
    const int cc = q - tap_i * a.cpt;
    const int tap = tap_i + a.tap0;
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    const bool kval = q < a.nkc;
    const int ch = cc * 8;
    char* As = smem + buf * BIG_STAGE + w * 4096;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yy = ay[j] + dy, xx = ax[j] + dx;
      const bool v = kval && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      uint32_t off;
      if (a.in_ps == 0) {
        off = (uint32_t)((((anh[j] + yy) * a.W + xx) * a.ldx + a.xcoff + ch) * 2);
      } else {
        const int r = a.in_ps;
        const int s = (int)fdiv((uint32_t)ch, a.fd_cps);
        const int cch = ch - s * a.fd_cps.d;
        const int si = s / r, sj = s - (s / r) * r;
        off = (uint32_t)((((anh[j] + yy) * r + si) * (a.W * r) + xx * r + sj) * a.ldx + a.xcoff + cch) * 2;
      }
      glds16(xr, As + j * 1024, v ? off : SR_OOB);
    }
    char* Bs = smem + buf * BIG_STAGE + 32768 + w * 4096;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      glds16(wr, Bs + j * 1024, (kval && bval[j]) ? boff[j] + (uint32_t)ks * 128u : SR_OOB);
  };

  auto compute = [&](int buf) {
    const char* As = smem + buf * BIG_STAGE;
    const char* Bs = As + 32768;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const uint32_t cq = kk * 4 + (lane >> 4);
      u32x4 fa[MI], fb[NI];
#pragma unroll
      for (int j = 0; j < NI; ++j) fb[j] = *(const u32x4*)(Bs + swz128(wn * 64 + j * 16 + (lane & 15), cq));
#pragma unroll
      for (int i = 0; i < MI; ++i) fa[i] = *(const u32x4*)(As + swz128(wm * 128 + i * 16 + (lane & 15), cq));
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) mfma_chunk<bf16_t>(fa[i], fb[j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
    }
  };

  issue(0, 0);
  if (nk > 1) issue(1, 1);
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    compute(ks & 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (ks + 2 < nk) issue(ks + 2, ks & 1);
  }

  float* Cs = (float*)smem;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
    if (wm == h) {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(i * 16 + (lane >> 4) * 4 + r) * CSTR + wn * 64 + j * 16 + (lane & 15)] = acc[i][j][r];
    }
    __syncthreads();
    epilogue_tile<bf16_t, 128, 256, 512>(a, Cs, CSTR, m0 + h * 128, n0, tid);
  }
}

// ------------------------------------------------------------------------------------
// 256 x 256 forward / dgrad kernel, phase-interleaved ("ping-pong") schedule.
//
// Same tile, waves, MFMA shape and LDS-DMA staging as conv3x3_fwd_big_kernel, but the
// K-step is cut into 4 phases (cdna_hip_programming.md §5 "256² 8-phase template"):
//   * LDS holds per buffer four 16 KB half-tiles A0 (tile rows 0-127), A1 (128-255),
//     B0 (cols 0-127), B1 (128-255).  Wave (wr = w>>2, wc = w&3) owns rows
//     {h*128 + wr*64 + [0,64)} x cols {g*128 + wc*32 + [0,32)}, h, g in {0, 1}, so its
//     quadrant (h, g) reads exactly half-tiles A_h and B_g.
//   * phase p of K-step t computes quadrant (0,0), (0,1), (1,1), (1,0) (16 MFMAs each)
//     and issues ONE half-tile of step t+1 (2 LDS-DMA per thread) in the order A0, B0, B1,
//     A1; a counted `s_waitcnt vmcnt(4)` keeps two half-tiles in flight across every
//     barrier and retires exactly what the next phase reads.
//   * waves 4-7 run one barrier behind waves 0-3 (stagger), so the two waves sharing a
//     SIMD alternate: one issues its fragment reads and DMA while the other runs MFMAs.
// Reads of a half-tile happen one barrier after the wait that retires it for every wave
// (two barriers for the lagging group); its slot is re-filled >= 4 phases after its last
// read.  Fragments: A 32 VGPR (one half), B 2 x 16 VGPR (both halves), acc 128 VGPR.
// ------------------------------------------------------------------------------------
template <bool FAST>
__global__ __launch_bounds__(512) void conv3x3_fwd_pp_kernel(FwdArgs a) {
  constexpr int CSTR = 256 + 4;
  constexpr int SMEM = 128 * CSTR * 4;  // epilogue half tile; >= 2 x 64 KB stages
  static_assert(SMEM >= 2 * BIG_STAGE, "LDS too small");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 2, wc = w & 3;
  const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (int)(tile / a.tiles_n) * 256;
  const int n0 = (int)(tile % a.tiles_n) * 256;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr_ = make_rsrc(a.w, a.w_bytes);

  // DMA rows of this lane inside a half-tile: w*16 + j*8 + (lane>>3), j = 0, 1.
  // Index k = h*2 + j (A: tile row h*128 + ...; B: output channel n0 + g*128 + ...).
  // FAST (every 64-deep K-step inside one tap and one shuffle slot, or a 1x1 conv): the A source offset is
  // a per-lane pixel base + a wave-uniform (tap, channel) offset computed on the scalar
  // unit, and the zero padding a per-lane 9-bit mask of valid taps -- the fragment-read /
  // DMA segment of a phase then carries ~3 VALU per DMA instead of the full gather math.
  const int c = (lane & 7) ^ (lane >> 3);  // logical chunk loaded by this lane (row & 7 == lane >> 3)
  const int rps = a.in_ps > 0 ? a.in_ps : 1;
  int ay[4], ax[4], anh[4];
  uint32_t abase[4], amask[4];
  uint32_t boff[4];
  bool bval[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = (k >> 1) * 128 + w * 16 + (k & 1) * 8 + (lane >> 3);
    const int m = m0 + r;
    amask[k] = 0;
    abase[k] = 0;
    if (m < a.M) {
      uint32_t q = fdiv((uint32_t)m, a.fd_W);
      ax[k] = m - (int)q * a.W;
      uint32_t n = fdiv(q, a.fd_H);
      ay[k] = (int)q - (int)n * a.H;
      anh[k] = (int)n * a.H;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = ay[k] + t / 3 - 1, xx = ax[k] + t % 3 - 1;
        if ((unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) amask[k] |= 1u << t;
      }
      abase[k] = (uint32_t)(((anh[k] + ay[k]) * rps * (a.W * rps) + ax[k] * rps) * a.ldx) * 2u + (uint32_t)c * 16u;
    } else {
      ax[k] = 0; ay[k] = -100000; anh[k] = 0;
    }
    const int n = n0 + r;
    bval[k] = n < a.Cout;
    boff[k] = (uint32_t)(n * a.ldw) * 2u + (uint32_t)c * 16u;
  }

  f32x4 acc[2][2][4][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[h][g][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (a.nkc + 7) >> 3;
  constexpr uint32_t SLOT_A0 = 0, SLOT_A1 = 16384, SLOT_B0 = 32768, SLOT_B1 = 49152;

  // FAST: wave-uniform state of the K-step whose A half-tiles are issued next (tap,
  // channel offset inside the tap, shuffle slot), advanced once per step on the scalar unit.
  int k_tap = a.tap0, k_chu = 0, k_uoff = 0;
  auto k_eval = [&]() {
    const int dy = k_tap / 3 - 1, dx = k_tap - (k_tap / 3) * 3 - 1;
    if (a.in_ps == 0) {
      k_uoff = ((dy * a.W + dx) * a.ldx + a.xcoff + k_chu) * 2;
    } else {
      const int r = a.in_ps;
      const int sl = (int)fdiv((uint32_t)k_chu, a.fd_cps);
      const int cch = k_chu - sl * a.fd_cps.d;
      const int si = (int)fdiv((uint32_t)sl, a.fd_r), sj = sl - si * r;
      k_uoff = (((dy * r + si) * (a.W * r) + dx * r + sj) * a.ldx + a.xcoff + cch) * 2;
    }
    k_uoff = __builtin_amdgcn_readfirstlane(k_uoff);
  };
  auto k_advance = [&]() {
    k_chu += 64;
    if (k_chu == a.Cin) { k_chu = 0; ++k_tap; }
    k_eval();
  };

  // one A half-tile (h) of K-step ks: 2 DMA per thread (FAST: ks is the step k_* describes)
  auto issue_a = [&](int ks, int h) {
    char* dst = smem + (ks & 1) * BIG_STAGE + (h ? SLOT_A1 : SLOT_A0) + w * 2048;
    if constexpr (FAST) {
      const bool kv = c * 8 < a.Cin - k_chu;  // 1x1 convs: Cin need not fill the last step
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k = h * 2 + j;
        glds16(xr, dst + j * 1024, (kv && ((amask[k] >> k_tap) & 1u)) ? abase[k] + (uint32_t)k_uoff : SR_OOB);
      }
    } else {
      const int q = ks * 8 + c;
      const int tap_i = (int)fdiv((uint32_t)q, a.fd_cpt);
      const int cc = q - tap_i * a.cpt;
      const int tap = tap_i + a.tap0;
      const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
      const bool kval = q < a.nkc;
      const int ch = cc * 8;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k = h * 2 + j;
        const int yy = ay[k] + dy, xx = ax[k] + dx;
        const bool v = kval && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
        uint32_t off;
        if (a.in_ps == 0) {
          off = (uint32_t)((((anh[k] + yy) * a.W + xx) * a.ldx + a.xcoff + ch) * 2);
        } else {
          const int r = a.in_ps;
          const int sl = (int)fdiv((uint32_t)ch, a.fd_cps);
          const int cch = ch - sl * a.fd_cps.d;
          const int si = sl / r, sj = sl - (sl / r) * r;
          off = (uint32_t)((((anh[k] + yy) * r + si) * (a.W * r) + xx * r + sj) * a.ldx + a.xcoff + cch) * 2;
        }
        glds16(xr, dst + j * 1024, v ? off : SR_OOB);
      }
    }
  };
  auto issue_b = [&](int ks, int g) {
    const bool kval = ks * 8 + c < a.nkc;
    char* dst = smem + (ks & 1) * BIG_STAGE + (g ? SLOT_B1 : SLOT_B0) + w * 2048;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = g * 2 + j;
      glds16(wr_, dst + j * 1024, (kval && bval[k]) ? boff[k] + (uint32_t)ks * 128u : SR_OOB);
    }
  };

  u32x4 fa[2][4], fb[2][2][2];  // fa[kk][i] (current A half), fb[g][kk][j]
  auto read_a = [&](int buf, int h) {
    const char* As = smem + buf * BIG_STAGE + (h ? SLOT_A1 : SLOT_A0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        fa[kk][i] = *(const u32x4*)(As + swz128(wr * 64 + i * 16 + (lane & 15), kk * 4 + (lane >> 4)));
  };
  auto read_b = [&](int buf, int g) {
    const char* Bs = smem + buf * BIG_STAGE + (g ? SLOT_B1 : SLOT_B0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[g][kk][j] = *(const u32x4*)(Bs + swz128(wc * 32 + j * 16 + (lane & 15), kk * 4 + (lane >> 4)));
  };
  auto mma = [&](int h, int g) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mfma_chunk<bf16_t>(fa[kk][i], fb[g][kk][j], acc[h][g][i][j]);
    __builtin_amdgcn_s_setprio(0);
  };

  // prologue: K-step 0 fully issued; A0, B0 retired for every wave before the first read
  if constexpr (FAST) k_eval();
  issue_a(0, 0);
  issue_b(0, 0);
  issue_b(0, 1);
  issue_a(0, 1);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  pp_barrier();
  if (wr) pp_barrier();  // stagger: waves 4-7 run one barrier behind

  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < nk;
    // phase 1: quadrant (0,0); issue A0(t+1); retire B1(t)
    read_a(buf, 0);
    read_b(buf, 0);
    if (more) {
      if constexpr (FAST) k_advance();
      issue_a(t + 1, 0);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    }
    pp_barrier();
    mma(0, 0);
    pp_barrier();
    // phase 2: quadrant (0,1); issue B0(t+1); retire A1(t)
    read_b(buf, 1);
    if (more) {
      issue_b(t + 1, 0);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    pp_barrier();
    mma(0, 1);
    pp_barrier();
    // phase 3: quadrant (1,1); issue B1(t+1)
    read_a(buf, 1);
    if (more) issue_b(t + 1, 1);
    pp_barrier();
    mma(1, 1);
    pp_barrier();
    // phase 4: quadrant (1,0); issue A1(t+1); retire A0(t+1), B0(t+1)
    if (more) {
      issue_a(t + 1, 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    }
    pp_barrier();
    mma(1, 0);
    pp_barrier();
  }
  if (!wr) pp_barrier();  // balance the stagger

  float* Cs = (float*)smem;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(wr * 64 + i * 16 + (lane >> 4) * 4 + r) * CSTR + g * 128 + wc * 32 + j * 16 + (lane & 15)] =
                acc[h][g][i][j][r];
    __syncthreads();
    epilogue_tile<bf16_t, 128, 256, 512>(a, Cs, CSTR, m0 + h * 128, n0, tid);
  }
}

// ------------------------------------------------------------------------------------
// conv3x3_fwd_pph_kernel<R>: the phase-interleaved 256x256 schedule of conv3x3_fwd_pp_kernel
// with the A operand formed from input HALO rows instead of one DMA'd half-tile per tap.
// A 256-pixel tile is R whole image rows of W = 256 / R pixels (R = 4: W 64, R = 2: W 128).
// Per 64-channel chunk the R + 2 rows y0-1 .. y0+R (W + 2 px x 128 B, XOR-swizzled, the
// two border columns zero) are staged in LDS once and all 9 taps read their A fragments
// from them.  The K loop is chunk-major (chunk, tap): per K-step only the two B half-tiles
// (2 x 16 KB) and ONE halo piece per wave are issued, vs. 4 half-tiles in the pp kernel.
// Row slots form a ring: load k = (R+2)*chunk + row goes to slot k mod S, issued once the
// slot's previous row is dead (its last tap row done) and >= 2 K-steps before its first use:
//   R = 4 (S 11, rows of 1 piece per wave): at tap j < 6 of chunk c, row j of chunk c+1;
//   R = 2 (S 5, rows of 2 pieces): taps 0-1 row 3 of chunk c, 2-3 / 4-5 / 6-7 rows 0 / 1 / 2
//   of chunk c+1, tap 8 a dummy.
// Per K-step issue order: B0(t+1) [ph1], B1(t+1) [ph2], halo/dummy piece [ph3]; counted
// waits vmcnt(3) at ph1 (retires B1(t)) and ph4 (retires B0(t+1) and the older halo piece).
// ------------------------------------------------------------------------------------
constexpr int PPH_SLOT0 = 2 * 32768;
template <int R>
struct PphGeom {
  static constexpr int W = 256 / R;
  static constexpr int ROWB = (W + 2) * 128;  // px -1 .. W
  static constexpr int NSLOT = R == 4 ? 11 : 5;
  static constexpr int PIECES = W / 64;  // 1-KB pieces per wave per row
  static constexpr int ZERO = PPH_SLOT0 + NSLOT * ROWB;
  static constexpr int LDS = ZERO + 1024;
  static_assert(LDS <= 160 * 1024, "pph LDS");
};

// P2: the two-interval schedule -- per K-step each wave group runs TWO MFMA intervals of two
// quadrants each (32 MFMAs: (0,0)+(0,1), then (1,1)+(1,0)) instead of four of one, so a K-step
// costs 4 barriers instead of 8.  Reads per group: R1 = A half 0 + both B halves, R2 = A half 1;
// DMA issue: B(t+1) (both halves) in R1 -- its buffer was last read at R1 of step t-1 by both
// groups -- and the halo piece in R2, then a counted vmcnt(1) retires B(t+1) and leaves only this
// step's halo piece in flight (halo pieces retire one step after issue, as before).  Where: the
// leading group (waves 0-3) waits after issuing its second MFMA interval, the lagging group at
// the end of its R2 -- both before the barrier that precedes the leading group's next R1, so
// every wave's pieces have landed when any wave reads them, and the leading group's DMA gets one
// more interval in flight.  Each accumulator's K order is unchanged: bitwise equal to the 4-phase
// form.
// P2 == 2 additionally prefetches the B half-tiles two K-steps ahead: B(t+2) is issued in R2 of
// step t into the buffer step t just read in R1 (both groups' R1 reads complete before the barrier
// that ends R1: lgkmcnt(0)), so a weight tile has ~5 intervals in flight instead of ~3.  Per step
// the issue order is [B(t+2) 4 ops][halo(t) 1 op]; the retire point (as above) waits vmcnt(6),
// which retires B(t+2)'s predecessor B(t+1) and every older halo piece (a halo piece issued at step
// t is then visible from step t+3 on; the ring schedule's first uses are >= 4 steps after issue).
// STRIP (R 4, P2 2): images wider than 64 px (W 256 / 512: EDSR at LR 256) as 64-px column strips,
// tiles ordered (image, strip, 4-row block); each halo row also DMAs its two border columns from the
// neighbouring strips (waves 0 / 1: slot pixels 0..7 and 58..65, the overlap rewriting bytes the row's
// own pieces hold; zeros at the image edges; the other waves a zero dummy, so every halo issue is two
// ops per wave and the retire point counts 8 instead of 6), and the epilogue maps tile rows to pixels
// (FwdArgs.strip64)
// PERS (R 4, P2 2, no strips; tiles_n 1, plain NHWC in / out, at most one gate-or-residual operand): the
// persistent multi-tile form.  The grid is min(tiles, G) blocks and block b owns a contiguous run of
// tiles (vertical neighbours in an image, so two of the next tile's six halo rows are L2 hits); ONE K
// loop runs across the run: the ring's chunk counter and the B double buffer's parity carry on over the
// tile boundary, so the next tile's chunk 0 is streamed as "chunk nchunk" of this one (its own image / row)
// and its B(0) / B(1) as B(nk) / B(nk+1); the per-step issue counts and the counted waits are unchanged.
// Only the first tile of a block pays the cold prologue (and the dispatch, LDS zeroing, address setup).
// At loop end the LDS holds the next tile's six rows and two B tiles; the five slots after them are free
// and four of them stage the accumulators in eight passes of 32 tile rows -- 16 of each wave row, so all
// eight waves write -- (a slot is exactly 8 rows of CSTR floats; the run of slots may wrap; their zero
// border columns are rewritten afterwards).  The tile's gate / residual operand (16 x 16 B per thread) and bias are loaded in two batches of 8, the
// first issued before the K loop's last barrier, the second during pass 1 (in flight under passes 2-3),
// instead of four serialized batches each waited for at once.  Per element the arithmetic and its order are
// epilogue_tile's, so the outputs are bitwise those of the one-tile form.  Nothing depends on dispatch
// order or residency: no inter-block communication.
template <int R, int P2 = 0, bool STRIP = false, bool PERS = false>
__global__ __launch_bounds__(512) void conv3x3_fwd_pph_kernel(FwdArgs a) {
  static_assert(!STRIP || (R == 4 && P2 == 2), "pph strips: the R 4 two-interval form");
  static_assert(!PERS || (R == 4 && P2 == 2 && !STRIP), "pph persistent: the R 4 two-interval form");
#ifdef SR_BAND_STAMPS
  // wave 0's phase clocks (tools/pph_stamps.py): [0] entry, [1] tiles, then per tile (the first three)
  // K loop start, K loop end, end of the first / second half of the epilogue; [14] cycles waiting for the
  // epilogue operand (PERS).  One lane stores each value as it is taken (plain vector stores).
  const unsigned long long st_entry = __builtin_readcyclecounter();
  // (the buffer holds 4096 blocks x 16 values)
  unsigned long long* const st_p =
      a.stamps && threadIdx.x == 0 && blockIdx.x < 4096 ? a.stamps + (size_t)blockIdx.x * 16 : nullptr;
  auto stamp = [&](int ti, int k) {
    if (st_p && ti < 3) st_p[2 + 4 * ti + k] = __builtin_readcyclecounter();
  };
#endif
  using G = PphGeom<R>;
  constexpr int W = G::W, RH = R + 2;
  constexpr int CSTR = 256 + 4;
  constexpr int SMEM = G::LDS > 128 * CSTR * 4 ? G::LDS : 128 * CSTR * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 2, wc = w & 3;
  const uint32_t tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (int)(tile / a.tiles_n) * 256;
  const int n0 = (int)(tile % a.tiles_n) * 256;
  int img, y0, sx0 = 0;  // image, first row, first column of the tile (sx0: STRIP)
  if constexpr (STRIP) {
    const int tm = m0 >> 8, tps = a.H >> 2, ns = a.W >> 6;
    img = tm / (tps * ns);
    const int rem = tm - img * tps * ns, j = rem / tps;
    y0 = (rem - j * tps) * 4;
    sx0 = j * 64;
  } else {
    const int HW = a.H * W;
    img = m0 / HW;
    y0 = (m0 - img * HW) / W;
  }
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr_ = make_rsrc(a.w, a.w_bytes);

  const int c = (lane & 7) ^ (lane >> 3);  // logical 16-B chunk of a B row this lane moves
  const int ch_h = (lane & 7) ^ (((lane >> 3) + 1) & 7);  // halo: slot px index = px + 1
  uint32_t boff[4];
  bool bval[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int n = n0 + (k >> 1) * 128 + w * 16 + (k & 1) * 8 + (lane >> 3);
    bval[k] = n < a.Cout;
    boff[k] = (uint32_t)(n * a.ldw) * 2u + (uint32_t)c * 16u;
  }
  // halo piece p of wave w: pixels 64p + 8w .. +7 of a row.  With in_ps = r (pixel-shuffled
  // input, the upsample convs' dgrads) LR pixel (y, x) of LR channel sl * C' + cch is HR pixel
  // (y r + si, x r + sj) (sl = si r + sj) channel cch: rows r HR rows apart, pixels r apart, and a
  // per-chunk (si, sj, cch) offset instead of cc * 128
  const int rps = a.in_ps > 0 ? a.in_ps : 1;
  const uint32_t hlane = (uint32_t)((sx0 + 8 * w + (lane >> 3)) * rps * a.ldx + a.xcoff) * 2u + (uint32_t)ch_h * 16u;
  const uint32_t rowb = (uint32_t)((STRIP ? a.W : W) * rps * rps * a.ldx) * 2u;
  const uint32_t pieceb = (uint32_t)(64 * rps * a.ldx) * 2u;
  auto chunk_off = [&](int cc) -> uint32_t {
    if (a.in_ps == 0) return (uint32_t)cc * 128u;
    const int c0 = cc * 64;
    const int sl = (int)fdiv((uint32_t)c0, a.fd_cps), cch = c0 - sl * a.fd_cps.d;
    const int si = sl / rps, sj = sl - si * rps;
    return (uint32_t)((si * W * rps + sj) * a.ldx + cch) * 2u;
  };

  if (tid < 64) *(u32x4*)(smem + G::ZERO + tid * 16) = u32x4{0u, 0u, 0u, 0u};
  if (!STRIP && tid < G::NSLOT * 16) {  // border columns (slot px index 0 and W + 1) of every slot
    const int sl = tid >> 4, e = tid & 15;
    *(u32x4*)(smem + PPH_SLOT0 + sl * G::ROWB + (e < 8 ? 0 : (W + 1) * 128) + (e & 7) * 16) =
        u32x4{0u, 0u, 0u, 0u};
  }

  f32x4 acc[2][2][4][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[h][g][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunk = a.Cin >> 6;
  const int nk = nchunk * 9;
  auto issue_dummy = [&]() { glds16(xr, smem + G::ZERO, SR_OOB); };
  auto issue_row = [&](int cc, int rr, int p) {  // piece p of row rr of chunk cc into its slot
    const int y = y0 - 1 + rr;
    const int slot = (RH * cc + rr) % G::NSLOT;
    glds16(xr, smem + PPH_SLOT0 + slot * G::ROWB + 128 + p * 8192 + w * 1024,
           (unsigned)y < (unsigned)a.H
               ? (uint32_t)(img * a.H + y) * rowb + (uint32_t)p * pieceb + hlane + chunk_off(cc)
               : SR_OOB);
    if constexpr (STRIP) {  // the strip's border columns (see the kernel comment)
      if (w < 2) {
        const int q = (w == 0 ? 0 : W - 6) + (lane >> 3);  // slot px index
        const int sx = sx0 + q - 1;
        const int lcb = (lane & 7) ^ (q & 7);
        const bool v = (unsigned)y < (unsigned)a.H && (unsigned)sx < (unsigned)a.W;
        glds16(xr, smem + PPH_SLOT0 + slot * G::ROWB + (w == 0 ? 0 : (W - 6) * 128),
               v ? (uint32_t)(((img * a.H + y) * a.W + sx) * a.ldx + a.xcoff) * 2u + (uint32_t)lcb * 16u + chunk_off(cc)
                 : SR_OOB);
      } else {
        issue_dummy();
      }
    }
  };
  auto issue_halo_dummy = [&]() {  // a halo issue's op count without a row
    issue_dummy();
    if constexpr (STRIP) issue_dummy();
  };
  // the halo piece issued at tap j of chunk cc (ring schedule above)
  auto issue_halo = [&](int cc, int j) {
    if constexpr (R == 4) {
      if (j < 6 && cc + 1 < nchunk) issue_row(cc + 1, j, 0); else issue_halo_dummy();
    } else {
      if (j < 2) issue_row(cc, 3, j);
      else if (j < 8 && cc + 1 < nchunk) issue_row(cc + 1, (j - 2) >> 1, j & 1);
      else issue_halo_dummy();
    }
  };
  // B half g of K-step (chunk kc, tap kt): weight columns kt*Cin + kc*64
  auto issue_b = [&](int buf, int kc, int kt, int g) {
    char* dst = smem + buf * 32768 + g * 16384 + w * 2048;
    const uint32_t kofs = (uint32_t)(kt * a.Cin + kc * 64) * 2u;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = g * 2 + j;
      glds16(wr_, dst + j * 1024, bval[k] ? boff[k] + kofs : SR_OOB);
    }
  };
  auto issue_b_dummy = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) issue_dummy();
  };

  u32x4 fa[2][4], fb[2][2][2];
  // A half h of step (cc, ty, tx): the wave's 64 output pixels are row r, columns x0 .. x0+63
  // (R = 4: r = 2h + wr, x0 = 0; R = 2: r = h, x0 = 64 wr); they read halo row r + ty at slot px
  // index x + tx (= px + 1).  Per lane and tx the swizzled offset inside a 16-px group is
  // fixed (16 is a multiple of the 8-row swizzle period): q<tx><kk>, + i * 2048 per group.
  // (named registers, not an array: a runtime-indexed array would live in scratch, and its
  // scratch loads would make the compiler drain vmcnt -- the DMA pipeline -- at every read)
  auto qoff = [&](int tx, int kk) -> uint32_t {
    const uint32_t pxi = (uint32_t)((lane & 15) + tx);
    return pxi * 128u + ((((uint32_t)(kk * 4 + (lane >> 4))) ^ (pxi & 7u)) << 4);
  };
  const uint32_t q00 = qoff(0, 0), q01 = qoff(0, 1), q10 = qoff(1, 0), q11 = qoff(1, 1), q20 = qoff(2, 0),
                 q21 = qoff(2, 1);
  const int xoff = R == 4 ? 0 : wr * 64 * 128;
  auto read_a = [&](int slot, int tx) {
    const char* Rs = smem + PPH_SLOT0 + slot * G::ROWB + xoff;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const uint32_t qa = kk ? q01 : q00, qb = kk ? q11 : q10, qc = kk ? q21 : q20;
      const uint32_t qq = tx == 0 ? qa : (tx == 1 ? qb : qc);
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[kk][i] = *(const u32x4*)(Rs + qq + i * 2048);
    }
  };
  auto read_b = [&](int buf, int g) {
    const char* Bs = smem + buf * 32768 + g * 16384;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        fb[g][kk][j] = *(const u32x4*)(Bs + swz128(wc * 32 + j * 16 + (lane & 15), kk * 4 + (lane >> 4)));
  };
  auto mma = [&](int h, int g) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mfma_chunk<bf16_t>(fa[kk][i], fb[g][kk][j], acc[h][g][i][j]);
    __builtin_amdgcn_s_setprio(0);
  };

  if constexpr (PERS) {
    constexpr int NS = G::NSLOT;
    const int nb = (int)gridDim.x, run = (int)tile;  // the run index (XCD-remapped block)
    const int tq = a.tiles / nb, trem = a.tiles - tq * nb;
    int tl = run * tq + (run < trem ? run : trem);  // the first trem runs own one tile more
    const int tend = tl + tq + (run < trem ? 1 : 0);
    const int HW = a.H * W;
    auto tile_pos = [&](int t_, int& im, int& yy) {
      const int m = t_ * 256;
      im = m / HW;
      yy = (m - im * HW) / W;
    };
    int timg, ty0;
    tile_pos(tl, timg, ty0);
    auto issue_row_p = [&](int slot, int lc, int rr, int im, int yy0) {  // row rr of chunk lc of a tile
      const int y = yy0 - 1 + rr;
      glds16(xr, smem + PPH_SLOT0 + slot * G::ROWB + 128 + w * 1024,
             (unsigned)y < (unsigned)a.H ? (uint32_t)(im * a.H + y) * rowb + hlane + (uint32_t)lc * 128u : SR_OOB);
    };
    auto lds_sync = [&]() {  // LDS writes / reads of this wave done, then the block barrier
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      pp_barrier();
    };
    // the epilogue operand: the ReLU / GELU' gate or the residual (the dispatch admits one of them)
    const bool useg = a.gate != nullptr;
    const __amdgpu_buffer_rsrc_t orr = useg ? make_rsrc(a.gate, a.g_bytes) : make_rsrc(a.res, a.r_bytes);
    // this thread's 8 channels; its 16 groups, in the order the passes consume them: group q is tile row
    // e_r0 + e_row(q)
    const int e_cg = tid & 31, e_n = e_cg * 8, e_r0 = tid >> 5;
    auto e_row = [](int q) { return (q >> 3) * 128 + (q & 1) * 64 + ((q >> 1) & 3) * 16; };
    // (Cout is 256: every channel group of the tile is stored.)  Without an operand the loads read nothing
    const bool e_oval = useg || (a.res && e_n < a.rcols);
    const uint32_t e_ostep = (uint32_t)(useg ? a.ldg : a.ldr) * 2u;  // bytes per operand row

    // cold prologue (first tile only): the six rows of chunk 0, B(0), B(1)
#pragma unroll 1
    for (int rr = 0; rr < 6; ++rr) issue_row_p(rr, 0, rr, timg, ty0);
    issue_b(0, 0, 0, 0);
    issue_b(0, 0, 0, 1);
    issue_b(1, 0, 1, 0);
    issue_b(1, 0, 1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pp_barrier();
    if (wr) pp_barrier();  // stagger: waves 4-7 run one barrier behind

    int s0 = 0;   // slot of row 0 of the current chunk: (6 * chunks so far) mod NS
    int par = 0;  // B buffer of the current step: (steps so far) & 1
    int m0t = tl * 256;
#ifdef SR_BAND_STAMPS
    int sti = 0;
    if (st_p) { st_p[0] = st_entry; st_p[1] = (unsigned long long)(tend - tl); }
#endif
#pragma unroll 1
    for (; tl < tend; ++tl) {
      const bool has_next = tl + 1 < tend;
      int nimg = timg, ny0 = ty0;
      if (has_next) tile_pos(tl + 1, nimg, ny0);
#ifdef SR_BAND_STAMPS
      stamp(sti, 0);
#endif
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[h][g][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      int cc = 0, tap = 0;      // this step
      int n2cc = 0, n2tap = 2;  // the step after the next; past this tile's nk steps, the next tile's first two
#pragma unroll 1
      for (int t = 0; t < nk; ++t) {
        const int buf = par;
        par ^= 1;
        const int ty = tap / 3, tx = tap - ty * 3;
        int sa = s0 + ty + wr;
        if (sa >= NS) sa -= NS;
        int sb = sa + 2;
        if (sb >= NS) sb -= NS;
        // R1
        read_a(sa, tx);
        read_b(buf, 0);
        read_b(buf, 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        pp_barrier();
        mma(0, 0);
        mma(0, 1);
        pp_barrier();
        // R2: B(t+2) -- of the next tile in the last two steps --, then the halo piece: row `tap` of the
        // next chunk, which after the last chunk is chunk 0 of the next tile
        read_a(sb, tx);
        if (t + 2 < nk || has_next) { issue_b(buf, n2cc, n2tap, 0); issue_b(buf, n2cc, n2tap, 1); }
        else { issue_b_dummy(); issue_b_dummy(); }
        {
          const bool lastc = cc + 1 == nchunk;
          if (tap < 6 && (!lastc || has_next)) {
            int sl = s0 + 6 + tap;
            if (sl >= NS) sl -= NS;
            issue_row_p(sl, lastc ? 0 : cc + 1, tap, lastc ? nimg : timg, lastc ? ny0 : ty0);
          } else {
            issue_dummy();
          }
        }
        if (wr) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        pp_barrier();
        mma(1, 1);
        mma(1, 0);
        if (!wr) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        pp_barrier();
        if (++tap == 9) {
          tap = 0;
          ++cc;
          s0 += 6;
          if (s0 >= NS) s0 -= NS;
        }
        if (++n2tap == 9) {
          n2tap = 0;
          if (++n2cc == nchunk) n2cc = 0;
        }
      }
      // the tile's operand and bias in flight while the accumulators are staged: the first half's 8
      // groups now, the second half's after pass 1 (into the registers of the accumulators staged by then)
      u32x4 ova[8], ovb[8];
      const uint32_t ob =
          (uint32_t)(((size_t)(m0t + e_r0) * (useg ? a.ldg : a.ldr) + (useg ? a.gcoff : a.rcoff) + e_n) * 2);
#pragma unroll
      for (int q = 0; q < 8; ++q) ova[q] = buf_load16(orr, e_oval ? ob + (uint32_t)e_row(q) * e_ostep : SR_OOB);
      f32x4 bias0 = f32x4{0.f, 0.f, 0.f, 0.f}, bias1 = bias0;
      if (a.bias) {
        bias0 = *(const f32x4*)(a.bias + e_n);
        bias1 = *(const f32x4*)(a.bias + e_n + 4);
      }
      if (!wr) pp_barrier();  // balance the stagger: every wave is past its last MFMA and LDS read
#ifdef SR_BAND_STAMPS
      stamp(sti, 1);
#endif
      // s0 is now the slot of row 0 of the NEXT chunk: rows s0 .. s0+5 (mod NS) are the next tile's, slots
      // s0+6 .. s0+9 stage 8 tile rows each.  Pass p = (h, i) stages accumulator row group i of half h of
      // every wave: 16 tile rows of each wave row wr (staging rows 16 wr .. 16 wr + 15), so all 8 waves write
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int h = p >> 2, i = p & 3;  // tile rows 128 h + 64 wr + 16 i .. + 15
        if (p) lds_sync();
        {
          int sl = s0 + 6 + wr * 2 + (lane >> 5);
          if (sl >= NS) sl -= NS;
          float* Cw = (float*)(smem + PPH_SLOT0 + sl * G::ROWB) + (((lane >> 4) & 1) * 4) * CSTR + wc * 32 + (lane & 15);
#pragma unroll
          for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int r = 0; r < 4; ++r) Cw[r * CSTR + g * 128 + j * 16] = acc[h][g][i][j][r];
        }
        lds_sync();
        if (p == 0) {
#ifdef SR_BAND_STAMPS
          const unsigned long long tw0 = __builtin_readcyclecounter();
#endif
          // the operand batch, and with it every older DMA of this wave (the next tile's rows and B
          // tiles: the barrier of pass 1 makes them visible to the block)
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef SR_BAND_STAMPS
          if (st_p && sti < 3) st_p[14] += __builtin_readcyclecounter() - tw0;
#endif
        }
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) {
          const int q = p * 2 + k2;
          int sl = s0 + 6 + k2 * 2 + (tid >> 8);
          if (sl >= NS) sl -= NS;
          const float* Cr = (const float*)(smem + PPH_SLOT0 + sl * G::ROWB) + (e_r0 & 7) * CSTR + e_cg * 8;
          {
            const int m = m0t + e_r0 + e_row(q);
            float v[8];
            const f32x4 c0 = *(const f32x4*)Cr;
            const f32x4 c1 = *(const f32x4*)(Cr + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) { v[j] = c0[j]; v[4 + j] = c1[j]; }
            if (a.bias) {
#pragma unroll
              for (int j = 0; j < 4; ++j) { v[j] += bias0[j]; v[4 + j] += bias1[j]; }
            }
            act_apply_n(v, a.act, a.slope);
            // the operand group is consumed HERE on every path (also when no operand is applied), so the
            // compiler's own wait for it is placed here and no load is left pending into the next tile
            // (a pending one makes it drain vmcnt -- the output stores -- where its register is reused)
            u32x4 ovq = q < 8 ? ova[q & 7] : ovb[q & 7];
            asm volatile("" : "+v"(ovq));
            float o8[8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const uint32_t oq = ovq[j];
              o8[2 * j] = bf16_to_f32(oq & 0xffff);
              o8[2 * j + 1] = bf16_to_f32(oq >> 16);
            }
            if (useg) {
              if (a.gate_mode == 1) {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] *= o8[j];
              } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] *= (o8[j] > 0.f ? 1.f : a.gate_slope);
              }
            }
            {
              const float al = a.alpha;
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] *= al;
            }
            if (!useg && a.res && e_n < a.rcols) {
#pragma unroll
              for (int j = 0; j < 8; ++j) v[j] = a.beta * o8[j] + v[j];
            }
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
            *(u32x4*)((bf16_t*)a.y + ((size_t)m * a.ldy + a.ycoff + e_n)) = o;
          }
        }
        if (p == 1) {
#pragma unroll
          for (int q = 0; q < 8; ++q) ovb[q] = buf_load16(orr, e_oval ? ob + (uint32_t)e_row(8 + q) * e_ostep : SR_OOB);
        }
#ifdef SR_BAND_STAMPS
        if (p == 3) stamp(sti, 2);
        if (p == 7) stamp(sti, 3);
#endif
      }
#ifdef SR_BAND_STAMPS
      ++sti;
#endif
      if (has_next) {
        lds_sync();  // the last pass's reads are done: rewrite the staging slots' zero border columns
        if (tid < 64) {
          int sl = s0 + 6 + (tid >> 4);
          if (sl >= NS) sl -= NS;
          const int e = tid & 15;
          *(u32x4*)(smem + PPH_SLOT0 + sl * G::ROWB + (e < 8 ? 0 : (W + 1) * 128) + (e & 7) * 16) = u32x4{0u, 0u, 0u, 0u};
        }
        m0t += 256;
        timg = nimg;
        ty0 = ny0;
        pp_barrier();
        if (wr) pp_barrier();  // stagger again
      }
    }
    return;
  }

  // prologue: the rows chunk 0 needs first (R = 4: all six; R = 2: rows 0-2, row 3 follows
  // at taps 0-1) and both B halves of step 0, all landed
#pragma unroll 1
  for (int rr = 0; rr < (R == 4 ? 6 : 3); ++rr)
#pragma unroll
    for (int p = 0; p < G::PIECES; ++p) issue_row(0, rr, p);
  issue_b(0, 0, 0, 0);
  issue_b(0, 0, 0, 1);
  if constexpr (P2 == 2) {  // B(1) too: the loop issues B(t+2) from step 0 on
    if (nk > 1) { issue_b(1, 0, 1, 0); issue_b(1, 0, 1, 1); }  // step 1 = (chunk 0, tap 1)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  pp_barrier();
#ifdef SR_BAND_STAMPS
  if (st_p) { st_p[0] = st_entry; st_p[1] = 1; }
  stamp(0, 0);
#endif
  if (wr) pp_barrier();  // stagger: waves 4-7 run one barrier behind

  int cc = 0, tap = 0;   // this step
  int ncc = 0, ntap = 1;  // the next step
  int n2cc = 0, n2tap = 2;  // the step after (P2 == 2)
  if (n2tap == 9) { n2tap = 0; ++n2cc; }
#pragma unroll 1
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < nk;
    const int ty = tap / 3, tx = tap - ty * 3;
    int sa, sb;  // slots of this wave's rows in halves 0 / 1
    if constexpr (R == 4) {
      sa = (RH * cc + ty + wr) % G::NSLOT;
      sb = sa + 2;
    } else {
      sa = (RH * cc + ty) % G::NSLOT;
      sb = sa + 1;
    }
    if (sb >= G::NSLOT) sb -= G::NSLOT;
    if constexpr (P2 == 2) {
      // R1: A half 0, B halves 0 and 1 of this step (their reads complete before the barrier: R2
      // re-fills this buffer with B(t+2))
      read_a(sa, tx);
      read_b(buf, 0);
      read_b(buf, 1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      pp_barrier();
      mma(0, 0);
      mma(0, 1);
      pp_barrier();
      // R2: A half 1; issue B(t+2) into this step's buffer, then this step's halo piece; retire B(t+1)
      read_a(sb, tx);
      if (t + 2 < nk) { issue_b(buf, n2cc, n2tap, 0); issue_b(buf, n2cc, n2tap, 1); }
      else { issue_b_dummy(); issue_b_dummy(); }
      issue_halo(cc, tap);
      if constexpr (STRIP) {  // the halo issues are two ops: [halo(t-1) 2][B(t+2) 4][halo(t) 2]
        if (wr) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else {
        if (wr) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      }
      pp_barrier();
      mma(1, 1);
      mma(1, 0);
      if constexpr (STRIP) {
        if (!wr) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else {
        if (!wr) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
      }
      pp_barrier();
      cc = ncc;
      tap = ntap;
      if (++ntap == 9) { ntap = 0; ++ncc; }
      if (++n2tap == 9) { n2tap = 0; ++n2cc; }
      continue;
    }
    if constexpr (P2 == 1) {
      // R1: A half 0, B halves 0 and 1 of this step; issue B(t+1) (both halves)
      read_a(sa, tx);
      read_b(buf, 0);
      read_b(buf, 1);
      if (more) { issue_b(buf ^ 1, ncc, ntap, 0); issue_b(buf ^ 1, ncc, ntap, 1); }
      else { issue_b_dummy(); issue_b_dummy(); }
      pp_barrier();
      mma(0, 0);
      mma(0, 1);
      pp_barrier();
      // R2: A half 1; issue this step's halo piece; retire B(t+1)
      read_a(sb, tx);
      issue_halo(cc, tap);
      if (wr) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      pp_barrier();
      mma(1, 1);
      mma(1, 0);
      if (!wr) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      pp_barrier();
      cc = ncc;
      tap = ntap;
      if (++ntap == 9) { ntap = 0; ++ncc; }
      continue;
    }
    // phase 1: quadrant (0,0); issue B0(t+1); retire B1(t)
    read_a(sa, tx);
    read_b(buf, 0);
    if (more) issue_b(buf ^ 1, ncc, ntap, 0); else issue_b_dummy();
    asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    pp_barrier();
    mma(0, 0);
    pp_barrier();
    // phase 2: quadrant (0,1); issue B1(t+1)
    read_b(buf, 1);
    if (more) issue_b(buf ^ 1, ncc, ntap, 1); else issue_b_dummy();
    pp_barrier();
    mma(0, 1);
    pp_barrier();
    // phase 3: quadrant (1,1); issue this step's halo piece
    read_a(sb, tx);
    issue_halo(cc, tap);
    pp_barrier();
    mma(1, 1);
    pp_barrier();
    // phase 4: quadrant (1,0); retire B0(t+1) (and the older halo piece)
    asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    pp_barrier();
    mma(1, 0);
    pp_barrier();
    cc = ncc;
    tap = ntap;
    if (++ntap == 9) { ntap = 0; ++ncc; }
  }
  if (!wr) pp_barrier();  // balance the stagger
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#ifdef SR_BAND_STAMPS
  stamp(0, 1);
#endif

  float* Cs = (float*)smem;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            Cs[(wr * 64 + i * 16 + (lane >> 4) * 4 + r) * CSTR + g * 128 + wc * 32 + j * 16 + (lane & 15)] =
                acc[h][g][i][j][r];
    __syncthreads();
    epilogue_tile<bf16_t, 128, 256, 512>(a, Cs, CSTR, m0 + h * 128, n0, tid);
#ifdef SR_BAND_STAMPS
    stamp(0, 2 + h);
#endif
  }
}

// The pph form of a call fwd_use_pph takes: 2 rows per tile at W 128, 4 at W 64; the two-interval schedule with the B
// prefetch (P2 2; W 64: persistent blocks where pph_pers_grid says so), without it (SR_VARIANT_PPH_P2_1) or the
// 4-phase schedule (SR_VARIANT_FOUR_PHASE).
void launch_pph(const FwdArgs& a, hipStream_t s) {
  const dim3 grid(a.tiles), blk(512);
  const bool w128 = a.W == 128;
  if (variant_is(SR_VARIANT_FOUR_PHASE)) {
    if (w128) hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<2, 0>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<4, 0>), grid, blk, 0, s, a);
  } else if (variant_is(SR_VARIANT_PPH_P2_1)) {
    if (w128) hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<2, 1>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<4, 1>), grid, blk, 0, s, a);
  } else if (w128) {
    hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<2, 2>), grid, blk, 0, s, a);
  } else if (const int gp = pph_pers_grid(a)) {
    hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<4, 2, false, true>), dim3(gp), blk, 0, s, a);
  } else {
    hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<4, 2>), grid, blk, 0, s, a);
  }
}

}  // namespace

namespace sr_conv {

hipError_t launch_fwd_big(const FwdArgs& a0, hipStream_t s) {
  FwdArgs a = a0;
  const int tm = (a.M + 255) / 256;
  a.tiles_n = (a.Cout + 255) / 256;
  a.tiles = tm * a.tiles_n;
  a.stamps = g_sr_stamps;
  if (variant_is(SR_VARIANT_TWO_BARRIER)) {
    hipLaunchKernelGGL(conv3x3_fwd_big_kernel, dim3(a.tiles), dim3(512), 0, s, a);
  } else if (fwd_use_pph_strip(a)) {
    a.strip64 = 1;
    hipLaunchKernelGGL((conv3x3_fwd_pph_kernel<4, 2, true>), dim3(a.tiles), dim3(512), 0, s, a);
  } else if (fwd_use_pph(a)) {
    launch_pph(a, s);
  } else if ((a.Cin % 64 == 0 || a.tap0 == 4) && (a.in_ps == 0 || a.fd_cps.d % 64 == 0)) {
    hipLaunchKernelGGL(conv3x3_fwd_pp_kernel<true>, dim3(a.tiles), dim3(512), 0, s, a);
  } else {
    hipLaunchKernelGGL(conv3x3_fwd_pp_kernel<false>, dim3(a.tiles), dim3(512), 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace sr_conv
