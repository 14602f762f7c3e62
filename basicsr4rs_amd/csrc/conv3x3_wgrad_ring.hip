// conv3x3 weight / bias gradient, the row-streaming kernels: conv3x3_wgrad_ring_kernel (narrow convs and
// 64-channel output tiles of wider ones, all nine taps per block) and conv3x3_wgrad_row3_kernel (256 x 128
// tiles, one kernel row of taps per block, one or two problems per grid), with their launches.
#include <utility>
#include <type_traits>
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

// ------------------------------------------------------------------------------------
// Weight gradient for narrow convs (Cout <= 64: RCAN / RRDB / SRResNet bodies; or 64-channel output
// tiles of a wider conv, wg_ring_wide), all nine taps in one block, whole image rows per split
// (W % 64 == 0).  The block walks each 64-px column segment of its rows top to bottom, so a K-step
// loads ONE new x halo row (66 px of a 16-ci tile per wave) into a ring and dy[64 px][Cout] once;
// rows above / below an image read a zero slot (x read ~once per pass instead of ~3x).  Every tap's
// GEMM is formed from LDS.  Wave w owns ci tile w (16 channels) x all co tiles x 9 taps (36 * CO_T
// accumulator tiles, pinned to AGPRs); operands by ds_read_b64_tr_b16.  LDS images are
// [tile][row][32 B] with row r stored at r ^ ((r >> 3) & 1) << 2: the rows a 32-lane half reads
// ({b..b+3} u {b+8..b+11}, any base b) hit distinct 32-B bank slots.  Both images are filled by
// LDS-DMA, two steps in flight.  Nearest-neighbour input upsampling (in_up 2, RRDBNet conv_up*) is
// folded into the halo gather; pixel-shuffled dy (the wide form) into the dy gather.  The first
// step of a segment loads its three rows itself, after the previous segment's last step (its slots
// may still be read), so a block has nseg - 1 one-step bubbles.
// (Round 4's variants -- two row groups or two co groups per 8-wave block, co split over blocks,
// early DMA issue, deeper pipelines -- all measured slower and were removed in round 5.)
//
// Output: the block's [tap][ci][co] partial sums (co fastest: a lane's 4 accumulator rows are 4
// consecutive co, one 16-B store per (tap, co tile)) into slab row `split` of [S][9][Cin][Cout].
// (Round 5 tried an in-kernel reduce: write-through slab rows, a ticket per group of G splits, the
// last arriver summing the group's rows in split order into a level-2 slab for the standalone reduce.
// Measured in the step it lost badly -- RCAN 38.1 -> 51.0 / 60.6 ms at G 2 / 4, RRDB 67.3 -> 77.6 /
// 80.7 ms: each group's tail reads (G - 1) x 147 KB at a few GB/s per block while the chip-wide reduce
// it replaces reads the whole slab in ~11 us -- and it was removed)
// ------------------------------------------------------------------------------------
SR_DEV int hrow(int r) { return r ^ (((r >> 3) & 1) << 2); }

template <int CO_T>
__global__ __launch_bounds__(256, 1) void conv3x3_wgrad_ring_kernel(WgArgs a) {
  constexpr int D = 2;              // steps in flight
  constexpr int LA = 3;             // fragment reads ahead of the MFMA group that needs them
  constexpr int RS = 3 * 1024;      // one halo row of one 16-ci tile: 96 rows x 32 B (66 used)
  constexpr int RSL = D + 2;        // ring slots: rows q-1 .. q+1 read, D - 1 in flight (+1 being issued)
  constexpr int RING = (RSL + 1) * RS;  // + the zero slot, per ci tile
  constexpr int DYB = CO_T * 2048;  // dy image: CO_T tiles x 64 rows x 32 B
  constexpr int DYS = DYB + 1024;   // + 1 KB target for padding DMAs
  constexpr int DYI = (CO_T * 2 + 3) / 4;  // dy DMAs per wave
  __shared__ __attribute__((aligned(16))) char smem[4 * RING + D * DYS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
  // block = (split, co tile, ci chunk), ci fastest: the tiles of one split (the same x / dy rows)
  // are consecutive, so xcd_remap keeps them on one XCD's L2
  const int per_split = a.tiles_ci * a.tiles_co;
  const int split = (int)b / per_split;
  const int rem_ = (int)b - split * per_split;
  const int cot = rem_ / a.tiles_ci;
  const int chunk = rem_ - cot * a.tiles_ci;
  const int ci0 = chunk * 64;
  const int co0 = cot * (CO_T * 16);
  // out_ps: the co tile lies in one shuffle slot (C' a multiple of the tile width, checked on the host)
  const int ps_sl = a.out_ps > 0 ? (int)fdiv((uint32_t)co0, a.fd_cps) : 0;
  const int ps_si = a.out_ps > 0 ? ps_sl / a.out_ps : 0, ps_sj = a.out_ps > 0 ? ps_sl - ps_si * a.out_ps : 0;
  const int rows_total = a.N * a.H;
  const int rps = a.kper / a.W;  // image rows per split
  const int r0 = split * rps, r1 = min(rows_total, r0 + rps);
  const int nrows = r1 - r0, nseg = a.W >> 6, nk = nrows * nseg;
  const __amdgpu_buffer_rsrc_t dyr = make_rsrc(a.dy, a.dy_bytes);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const int sh = a.in_up > 1 ? 1 : 0;  // in_up is 1 or 2 here
  const int Hs = a.H >> sh, Ws = a.W >> sh;
  char* ring = smem + w * RING;
  char* dys = smem + 4 * RING;
  auto slot = [](int q) { return (q + RSL) % RSL; };  // q >= -1

  // this lane's halo pixels of its 3 DMAs per row: physical row 32i + (lane >> 1) holds pixel
  // hrow(.) (x0 - 1 + that), channel half lane & 1
  int hpx[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int hr = hrow(32 * i + (lane >> 1));
    hpx[i] = hr < 66 ? hr : -100000;
  }
  const int cil = ci0 + w * 16 + (lane & 1) * 8;
  const bool civ = cil < a.Cin;
  for (int i = lane; i < RS / 16; i += 64) *(u32x4*)(ring + RSL * RS + i * 16) = u32x4{0u, 0u, 0u, 0u};

  f32x4 acc[9][CO_T], accb[CO_T];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int c = 0; c < CO_T; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < CO_T; ++c) accb[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = a.wsb != nullptr && chunk == 0 && w == 0;

  // x halo row q (global image row; outside [0, rows_total) -> zeros), column segment seg
  auto issue_row = [&](int q, int seg) {
    const bool qv = q >= 0 && q < rows_total;
    const int n = qv ? (int)fdiv((uint32_t)q, a.fd_H) : 0;
    const int yy = q - n * a.H;
    char* dst = ring + slot(q) * RS;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int xx = seg * 64 - 1 + hpx[i];
      const bool v = qv && civ && (unsigned)xx < (unsigned)a.W;
      const uint32_t off = (uint32_t)((((n * Hs + (yy >> sh)) * Ws + (xx >> sh)) * a.ldx + a.xcoff + cil) * 2);
      glds16(xr, dst + i * 1024, v ? off : SR_OOB);
    }
  };
  // step j = (segment j / nrows, row r0 + j % nrows); the first step of a segment loads its
  // three rows and is issued after the previous segment's last step (whose slots it reuses)
  auto first = [&](int j) { return j % nrows == 0; };
  auto nops = [&](int j) { return DYI + (first(j) ? 9 : 3); };
  auto issue_iter = [&](int j) { const int f = j - j % nrows - 1, e = j - D; return f > e ? f : e; };
  auto issue = [&](int j) {
    const int seg = j / nrows, q = r0 + (j - seg * nrows);
    if (first(j)) {
      issue_row(q - 1, seg);
      issue_row(q, seg);
    }
    issue_row(q + 1, seg);
    const int p0s = q * a.W + seg * 64;
    char* st = dys + (j % D) * DYS;
#pragma unroll
    for (int i = 0; i < DYI; ++i) {
      const int k = w + 4 * i;  // dy DMA index: co tile k >> 1, rows 32 (k & 1) ..
      char* dst = st + DYB;
      uint32_t off = SR_OOB;
      if (k < CO_T * 2) {
        const int pr = hrow((k & 1) * 32 + (lane >> 1));
        const int co = co0 + (k >> 1) * 16 + (lane & 1) * 8;
        dst = st + k * 1024;
        if (co < a.Cout) {
          if (a.out_ps == 0) {
            off = (uint32_t)(((p0s + pr) * a.ldy + a.ycoff + co) * 2);
          } else {  // pixel-shuffled dy: GEMM column sl * C' + c of LR pixel (q, x) = HR pixel (q r + si, x r + sj), channel c
            const int r = a.out_ps;
            const int hp = (q * r + ps_si) * (a.W * r) + (seg * 64 + pr) * r + ps_sj;
            off = (uint32_t)((hp * a.ldy + a.ycoff + co - ps_sl * a.fd_cps.d) * 2);
          }
        }
      }
      glds16(dyr, dst, off);
    }
  };

  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  auto tr2 = [&](const char* img, int r0_) -> s16x8 {  // rows r0 + tq (K 0..3), r0 + 4 + tq (K 4..7)
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + hrow(r0_ + tq) * 32 + tp * 8));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + hrow(r0_ + 4 + tq) * 32 + tp * 8));
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  auto compute = [&](int j) {
    const int q = r0 + j % nrows;
    const int y = q - (int)fdiv((uint32_t)q, a.fd_H) * a.H;
    const char* rows3[3] = {ring + (y == 0 ? RSL : slot(q - 1)) * RS, ring + slot(q) * RS,
                            ring + (y == a.H - 1 ? RSL : slot(q + 1)) * RS};
    const char* ds = dys + (j % D) * DYS;
    // Fragment reads (per K half: this wave's dy tiles, then the 9 taps' x tiles) run LA reads
    // ahead of the MFMA group (one tap x CO_T co tiles) that needs them, in program order fixed by
    // scheduling barriers (the compiler otherwise sinks each read to just before its MFMAs); at
    // most ~2 (LA + 1) reads are in flight, within what lgkmcnt counts, so its waits stay exact.
    constexpr int NR = CO_T + 9;
    s16x8 fr[2 * NR];
    auto rd = [&](int r) {
      const int kk = r / NR, i = r - kk * NR;
      fr[r] = i < CO_T ? tr2(ds + i * 2048, kk * 32 + 8 * g) : tr2(rows3[(i - CO_T) / 3], ((i - CO_T) % 3) + kk * 32 + 8 * g);
    };
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int need = kk * NR + CO_T + t;
        // reads not yet issued up to need + LA (the previous group issued up to its need + LA)
        const int lo = (kk == 0 && t == 0) ? 0 : (t > 0 ? need + LA : NR + LA);
#pragma unroll
        for (int r = 0; r < 2 * NR; ++r)
          if (r >= lo && r <= need + LA) rd(r);
        // accumulators pinned to AGPRs (inline asm): with this many of them the compiler
        // otherwise moves every one between AGPRs and VGPRs once per step
#pragma unroll
        for (int c = 0; c < CO_T; ++c)
          asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[t][c]) : "v"(fr[kk * NR + c]), "v"(fr[need]));
        __builtin_amdgcn_sched_barrier(0);
      }
      if (do_bias) {  // builtin: the compiler pads the VALU write of `ones` before its read
#pragma unroll
        for (int c = 0; c < CO_T; ++c) accb[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[kk * NR + c], ones, accb[c], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  __syncthreads();  // zero slots written
  int next = 0;  // steps issued so far, in step order (issue_iter is non-decreasing)
  while (next < nk && issue_iter(next) < 0) issue(next++);
  for (int ks = 0; ks < nk; ++ks) {
    // step ks's DMAs landed; the steps issued after it may stay in flight
    if (next == ks + D && (ks + 1) % nrows != 0 && (ks + 1) / nrows == (next - 1) / nrows) {
      // steady state: the D - 1 steps after ks, none of them a segment's first
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * (DYI + 3)) : "memory");
    } else {
      int younger = 0;
      for (int j = ks + 1; j < next; ++j) younger += nops(j);
      vm_wait_dyn(younger);
    }
    __builtin_amdgcn_s_barrier();
    compute(ks);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    while (next < nk && issue_iter(next) <= ks) issue(next++);
  }

  // the last MFMAs' results are read below (inline-asm MFMAs: the hazard wait is ours)
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  const int c16 = lane & 15;
  const int ci = ci0 + w * 16 + c16;
  // slab row `split`; the standalone reduce sums the S rows
  if (ci < a.Cin) {
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float* ws = a.ws + (((size_t)split * 9 + t) * a.Cin + ci) * a.Cout;
#pragma unroll
      for (int c = 0; c < CO_T; ++c) {
        const int co = co0 + c * 16 + g * 4;
        if (co < a.Cout) *(f32x4*)(ws + co) = acc[t][c];
      }
    }
  }
  if (do_bias && c16 == 0) {
#pragma unroll
    for (int c = 0; c < CO_T; ++c)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + c * 16 + g * 4 + r;
        if (co < a.Cout) a.wsb[(size_t)split * a.Cout + co] = accb[c][r];
      }
  }
}

// ------------------------------------------------------------------------------------
// Weight gradient over one kernel ROW of taps (round 6): bf16 3x3, Cout % 256 == 0, Cin % 128 == 0,
// W % 64 == 0, no upsample; pixel-shuffled dy with C' % 256 == 0 (the EDSR-L body and upsample convs).  A pp-kernel block is one tap of
// a 256 x 256 (co x ci) tile: each K-step DMAs the dy tile AND a tap-shifted x tile (64 KB per 4.2 M
// MACs) and its 8 waves of 128 x 64 read 192 KB of fragments.  Here a block owns the three taps
// (ky, 0..2) of a 256 x 128 tile: a K-step (64 pixels of one image row) DMAs the dy tile (32 KB) and
// ONE x halo row of 66 pixels (16.5 KB), and the three taps' B operands are that row read at row
// offsets 0 / 1 / 2: 48.5 KB per 6.3 M MACs.  4 waves, one per SIMD; wave (wr, wc) = 128 co x 64 ci x
// 3 taps, 384 accumulator registers (taps 0 / 1 pinned to AGPRs, tap 2 in VGPRs); an A fragment feeds
// 12 MFMAs and a B fragment 8 (40 KB of fragment reads per wave and step for 1.6 M MACs).  Three LDS
// stages; one barrier per step, placed before the step's last MFMA group, after which the next step's
// first fragment reads run under that group.  Operand images as the ring kernel's: [16-channel tile]
// [row][32 B] with rows permuted by hrow (conflict-free tr reads at any row offset); the halo row's 66
// rows arrive as three 32-row pieces, the third (rows 34..65) rewriting 30 rows of the second with the
// same bytes.  Image edges and rows outside the image read zeros (out-of-range buffer offsets).  Bias:
// bias-role blocks after the tile blocks, each summing dy over bias_group splits.  Output: the pp
// kernel's [S][9][Cout][Cin] slab (same reduce), staged through LDS for 16-B row stores.  One grid can
// hold two problems of one geometry (WgArgs.pair_nt, sr_conv3x3_wgrad_pair: both convs of a residual block
// at half the splits each; DESIGN note 40).
// ------------------------------------------------------------------------------------
// Compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N - 1 (fully unrolled by construction;
// a #pragma unroll loop this large exceeds the unroller's threshold and its arrays go to scratch).
template <typename F, int... I>
SR_DEV void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
SR_DEV void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}
constexpr int row3_need(int gi) { return (gi / 12) * 20 + 8 + gi % 12; }  // last fragment read group gi uses

__global__ __launch_bounds__(256, 1) void conv3x3_wgrad_row3_kernel(WgArgs a) {
  constexpr int LA = 1;  // fragment reads one MFMA group ahead (two: the same time, 4 more VGPRs)
  constexpr int DYT = 2048;      // one 16-co tile of dy: 64 rows x 32 B
  constexpr int XT = 66 * 32;    // one 16-ci tile of the halo row: 66 rows x 32 B
  constexpr int DYB = 16 * DYT;  // 256 co
  constexpr int STG = DYB + 8 * XT;
  constexpr int NOPS = 14;       // LDS-DMAs per wave and K-step: 8 dy + 6 x
  __shared__ __attribute__((aligned(16))) char smem[3 * STG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 1, wc = w & 1;
  uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
  if (a.pair_nt > 0) {
    // two problems of one geometry in one grid, [tiles 0][tiles 1][bias 0][bias 1]: pick this block's
    // problem (block-uniform) and rebase b to its index in that problem's own single-launch grid
    const uint32_t nt = (uint32_t)a.pair_nt, nbias = (gridDim.x - 2 * nt) >> 1;
    bool second;
    if (b < 2 * nt) {
      second = b >= nt;
      b -= second ? nt : 0;
    } else {
      const uint32_t bb = b - 2 * nt;
      second = bb >= nbias;
      b = nt + bb - (second ? nbias : 0);
    }
    if (second) {
      a.dy = a.dy1; a.x = a.x1; a.ws = a.ws1; a.wsb = a.wsb1;
      a.dy_bytes = a.dy1_bytes; a.x_bytes = a.x1_bytes;
    }
  }
  const int ntile = 3 * a.tiles_co * a.tiles_ci;
  const __amdgpu_buffer_rsrc_t dyr = make_rsrc(a.dy, a.dy_bytes);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const int g = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;

  // pixel-shuffled dy (out_ps r, the upsample convs): a 256-co tile lies in ONE shuffle slot sl
  // (C' % 256 == 0, checked on the host), so GEMM column co0 + c of LR pixel (q, x) is channel
  // co0 - sl C' + c of HR pixel (q r + sl / r, x r + sl % r): LR pixels r HR pixels apart
  const int rps = a.out_ps > 0 ? a.out_ps : 1;
  auto dy_base = [&](int p0s, int co0) -> int {  // byte offset of (first pixel of the K-step, co0)
    if (a.out_ps == 0) return (p0s * a.ldy + a.ycoff + co0) * 2;
    const int q = (int)fdiv((uint32_t)p0s, a.fd_W), x0 = p0s - q * a.W;
    const int sl = (int)fdiv((uint32_t)co0, a.fd_cps), si = sl / rps, sj = sl - si * rps;
    return (((q * rps + si) * (a.W * rps) + x0 * rps + sj) * a.ldy + a.ycoff + co0 - sl * (int)a.fd_cps.d) * 2;
  };
  // dy pieces of this wave: k = w + 4 i -> co tile k >> 1, physical rows 32 (k & 1) + (lane >> 1)
  uint32_t dyl[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = w + 4 * i;
    const int pr = hrow((k & 1) * 32 + (lane >> 1));
    dyl[i] = (uint32_t)((pr * rps * a.ldy + (k >> 1) * 16 + (lane & 1) * 8) * 2);
  }
  auto issue_dy = [&](char* st, int s_dyb) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = w + 4 * i;
      glds16(dyr, st + (k >> 1) * DYT + (k & 1) * 1024, (uint32_t)s_dyb + dyl[i]);
    }
  };
  auto tr2 = [&](const char* img, int r0_) -> s16x8 {  // rows r0 + tq (K 0..3), r0 + 4 + tq (K 4..7)
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + hrow(r0_ + tq) * 32 + tp * 8));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(img + hrow(r0_ + 4 + tq) * 32 + tp * 8));
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };

  if ((int)b >= a.splits * ntile) {
    // bias role: dy column sums of one 256-co tile over bias_group splits (dy images only, two stages)
    const int bb = (int)b - a.splits * ntile;
    const int grp = bb / a.tiles_co, co0 = (bb - grp * a.tiles_co) * 256;
    const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
    const int s1 = min(a.splits, (grp + 1) * a.bias_group);
    for (int sp = grp * a.bias_group; sp < s1; ++sp) {
      const int p_begin = sp * a.kper, p_end = min(a.M, p_begin + a.kper);
      const int nk = (p_end - p_begin) >> 6;
      auto base = [&](int ks) { return __builtin_amdgcn_readfirstlane(dy_base(p_begin + ks * 64, co0)); };
      f32x4 accb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      __syncthreads();  // the previous split's stage reads are done
      if (nk > 0) issue_dy(smem, base(0));
      if (nk > 1) issue_dy(smem + STG, base(1));
      for (int ks = 0; ks < nk; ++ks) {
        if (ks + 1 < nk)
          asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const char* st = smem + (ks & 1) * STG;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr2(st + (w * 4 + i) * DYT, kk * 32 + 8 * g), ones, accb[i], 0, 0, 0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (ks + 2 < nk) issue_dy(smem + (ks & 1) * STG, base(ks + 2));
      }
      if ((lane & 15) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int co = co0 + (w * 4 + i) * 16 + g * 4 + r;
            if (co < a.Cout) a.wsb[(size_t)sp * a.Cout + co] = accb[i][r];
          }
      }
    }
    return;
  }

  const int split = (int)b / ntile;
  int rem = (int)b - split * ntile;
  const int ky = rem / (a.tiles_co * a.tiles_ci);
  rem -= ky * a.tiles_co * a.tiles_ci;
  const int co0 = (rem / a.tiles_ci) * 256;
  const int ci0 = (rem % a.tiles_ci) * 128;
  const int dy_ = ky - 1;
  const int p_begin = split * a.kper;
  const int p_end = min(a.M, p_begin + a.kper);
  const int nk = (p_end - p_begin) >> 6;  // >= 1: whole 64-pixel steps (M, kper multiples of 64)

  // x pieces of this wave: k = w + 4 i (i < 6) -> ci tile k / 3, piece k % 3 at physical row 0 / 32 / 34;
  // lane: physical row base + (lane >> 1) = logical halo row (pixel x0 - 1 + row) hrow(.), channel half lane & 1
  uint32_t xl[6];
  int xlr[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const int k = w + 4 * i, t = k / 3, pc = k - 3 * t;
    const int lr = hrow((pc == 0 ? 0 : (pc == 1 ? 32 : 34)) + (lane >> 1));
    xlr[i] = lr;
    xl[i] = (uint32_t)((lr * a.ldx + t * 16 + (lane & 1) * 8) * 2);
  }
  // scalar state of a K-step's DMAs (k_eval), then its 14 pieces (piece < 8: dy, else x)
  int s_dyb = 0, s_xb = 0, s_xm1 = 0, s_yv = 0;
  auto k_eval = [&](int ks) {
    const int p0s = p_begin + ks * 64;
    const int q = (int)fdiv((uint32_t)p0s, a.fd_W);
    const int x0 = p0s - q * a.W;
    const int n = (int)fdiv((uint32_t)q, a.fd_H);
    const int y = q - n * a.H;
    s_dyb = __builtin_amdgcn_readfirstlane(dy_base(p0s, co0));
    s_xb = __builtin_amdgcn_readfirstlane((((q + dy_) * a.W + x0 - 1) * a.ldx + a.xcoff + ci0) * 2);
    s_xm1 = __builtin_amdgcn_readfirstlane(x0 - 1);
    s_yv = __builtin_amdgcn_readfirstlane((unsigned)(y + dy_) < (unsigned)a.H ? 1 : 0);
  };
  auto piece = [&](char* st, int pi) {  // pi: compile-time after unrolling
    if (pi < 8) {
      const int k = w + 4 * pi;
      glds16(dyr, st + (k >> 1) * DYT + (k & 1) * 1024, (uint32_t)s_dyb + dyl[pi]);
    } else {
      const int i = pi - 8, k = w + 4 * i, t = k / 3, pc = k - 3 * t;
      const bool v = s_yv && (unsigned)(s_xm1 + xlr[i]) < (unsigned)a.W;
      glds16(xr, st + DYB + t * XT + (pc == 0 ? 0 : (pc == 1 ? 32 : 34)) * 32, v ? (uint32_t)(s_xb + (int)xl[i]) : SR_OOB);
    }
  };
  auto issue = [&](int ks, char* st) {
    k_eval(ks);
#pragma unroll
    for (int pi = 0; pi < NOPS; ++pi) piece(st, pi);
  };

  f32x4 acc0[8][4], acc1[8][4], acc2[8][4];  // taps kx 0 / 1 (AGPRs), 2 (VGPRs); [co tile][ci tile]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc0[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  // a step's fragment reads: r = 20 kk + i, i < 8: A (dy) co tile wr * 8 + i; 8 <= i < 20: B, tap
  // kx = (i - 8) >> 2, ci tile wc * 4 + ((i - 8) & 3) (the halo row at row offset kx)
  s16x8 fa[2][8], fb[2][12];
  auto rd = [&](const char* st, auto R) {
    constexpr int r = R, kk = r / 20, i = r - kk * 20;
    if constexpr (i < 8) {
      fa[kk][i] = tr2(st + (wr * 8 + i) * DYT, kk * 32 + 8 * g);
    } else {
      constexpr int c = i - 8;
      fb[kk][c] = tr2(st + DYB + (wc * 4 + (c & 3)) * XT, kk * 32 + 8 * g + (c >> 2));
    }
  };
  // MFMA group gi (24 per step): kk = gi / 12, B fragment c = gi % 12 against the 8 A fragments
  auto group = [&acc0, &acc1, &acc2, &fa, &fb](auto GI) {  // (explicit: if constexpr branches)
    constexpr int gi = GI, kk = gi / 12, c = gi % 12, kx = c >> 2, j = c & 3;
    (void)acc0, (void)acc1, (void)acc2;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if constexpr (kx == 0)
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc0[i][j]) : "v"(fa[kk][i]), "v"(fb[kk][c]));
      else if constexpr (kx == 1)
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc1[i][j]) : "v"(fa[kk][i]), "v"(fb[kk][c]));
      else
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc2[i][j]) : "v"(fa[kk][i]), "v"(fb[kk][c]));
    }
  };
  // read stream position x (group x's last read): x < 24 this step, x >= 24 the next step's
  constexpr auto rpos = [](int x) { return x < 24 ? row3_need(x) : 40 + row3_need(x - 24); };
  constexpr int GB = 24 - LA;  // the group before which the barrier runs (its reads reach the next step)

  issue(0, smem);
  if (nk > 1) issue(1, smem + STG);
  if (nk > 2) issue(2, smem + 2 * STG);
  vm_wait_dyn(NOPS * (min(nk, 3) - 1));
  __builtin_amdgcn_s_barrier();
  static_for<rpos(LA - 1) + 1>([&](auto R) { rd(smem, R); });
  int stc = 0;  // stage of step t
  for (int t = 0; t < nk; ++t) {
    const int stn = stc == 2 ? 0 : stc + 1;
    const char* cur = smem + stc * STG;
    const char* nxt = smem + stn * STG;
    const bool more = t + 1 < nk;
    static_for<24>([&](auto GI) {
      constexpr int gi = GI;
      // this step's reads up to group gi + LA's
      static_for<40>([&](auto R) {
        if constexpr (R > rpos(gi + LA - 1) && R <= rpos(gi + LA) && R < 40) rd(cur, R);
      });
      if constexpr (gi == GB) {
        if (more) {
          // every read of step t is issued: once they completed and step t + 1 landed (in every wave),
          // step t's stage takes step t + 3's DMAs and step t + 1's first reads run under these groups
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (t + 2 < nk)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NOPS) : "memory");
          else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
          if (t + 3 < nk) issue(t + 3, smem + stc * STG);
        }
      }
      if constexpr (gi >= GB) {
        if (more) {
          static_for<40>([&](auto R) {
            if constexpr (R + 40 > rpos(gi + LA - 1) && R + 40 <= rpos(gi + LA)) rd(nxt, R);
          });
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      group(GI);
      __builtin_amdgcn_sched_barrier(0);
    });
    stc = stn;
  }

  // the last MFMAs' results are read below (inline-asm MFMAs: the hazard wait is ours)
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  // slab: 4-B stores straight from the accumulators (16 lanes: 64 contiguous bytes).  (Staged through
  // LDS for 16-B row stores, as the pp kernel does, it measured slower: 165-173 vs 163-170 us.)
#pragma unroll
  for (int kx = 0; kx < 3; ++kx) {
    float* ws = a.ws + ((size_t)split * 9 + ky * 3 + kx) * a.Cout * a.Cin;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = kx == 0 ? acc0[i][j] : (kx == 1 ? acc1[i][j] : acc2[i][j]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          ws[(size_t)(co0 + wr * 128 + i * 16 + g * 4 + r) * a.Cin + ci0 + wc * 64 + j * 16 + (lane & 15)] = v[r];
      }
  }
}

}  // namespace

namespace sr_conv {

hipError_t launch_wg_ring(WgArgs a, const sr_conv3x3_wgrad_desc* d, hipStream_t s) {
  const int S = a.splits;
  a.tiles_co = ring_tiles_co(d);
  a.tiles_ci = (a.Cin + 63) / 64;
  const int ct = ring_ct(d);
  const dim3 grid(S * a.tiles_ci * a.tiles_co);
  if (ct == 1) hipLaunchKernelGGL(conv3x3_wgrad_ring_kernel<1>, grid, dim3(256), 0, s, a);
  else if (ct == 2) hipLaunchKernelGGL(conv3x3_wgrad_ring_kernel<2>, grid, dim3(256), 0, s, a);
  else if (ct == 3) hipLaunchKernelGGL(conv3x3_wgrad_ring_kernel<3>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(conv3x3_wgrad_ring_kernel<4>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_wg_row3(WgArgs a, hipStream_t s) {
  const int S = a.splits;
  a.tiles_co = a.Cout / 256;
  a.tiles_ci = a.Cin / 128;
  a.bias_group = wg_row3_bg();
  const int nb = S * 3 * a.tiles_co * a.tiles_ci + (a.wsb ? (S + a.bias_group - 1) / a.bias_group * a.tiles_co : 0);
  hipLaunchKernelGGL(conv3x3_wgrad_row3_kernel, dim3(nb), dim3(256), 0, s, a);
  return hipGetLastError();
}

// Two problems of one geometry (a: problem 0 and the dy1 / x1 / ws1 / wsb1 set, both wsb or neither) in one grid:
// each problem's tile blocks contiguous and split-major as in its own launch, then the bias-role blocks of both.
hipError_t launch_wg_row3_pair(WgArgs a, int bias_group, hipStream_t s) {
  const int S = a.splits;
  a.tiles_co = a.Cout / 256;
  a.tiles_ci = a.Cin / 128;
  a.bias_group = bias_group;
  a.pair_nt = S * 3 * a.tiles_co * a.tiles_ci;
  const int nb = 2 * a.pair_nt + (a.wsb ? 2 * ((S + bias_group - 1) / bias_group) * a.tiles_co : 0);
  hipLaunchKernelGGL(conv3x3_wgrad_row3_kernel, dim3(nb), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sr_conv
