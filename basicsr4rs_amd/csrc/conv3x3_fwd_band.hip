// conv3x3 forward / dgrad for narrow convs, row-streaming persistent form: conv3x3_fwd_band_kernel and its
// launches (whole rows, 128-px column strips).  "The tile kernel above" of the comment below is
// conv3x3_fwd_halo_kernel (conv3x3_fwd_tile.hip).
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

// ------------------------------------------------------------------------------------
// Narrow-conv forward / dgrad, row-streaming persistent form (bf16 3x3, Cin 32 or 64,
// Cout 32 or 64, W 64 or 128: RCAN / SRResNet bodies, RRDB conv1 and dgrads into 64 ch).
//
// The tile kernel above loads a halo, computes and stores in one pass per block, so with one
// wave of blocks the chip runs the three phases one after the other (RCAN conv at B 32:
// 24 us, of which 8 us store tail and ~5 us load burst; the MFMA work is ~4.6 us per SIMD).
// Here a block owns a band of consecutive output rows (one row = W pixels of one image; the
// NHWC rows of all images are one contiguous sequence) and streams it: input rows live in an
// (LA + 2)-slot LDS ring (slot = global row % S, W + 2 swizzled 128-B pixel rows, zero border
// columns written once); row s + LA is DMA'd while row s is computed, the residual / gate
// operands of row s are DMA'd into per-wave staging before its MFMAs (each lane reads back its
// own 16 B), and its stores drain while later rows compute.  Rows outside an image (the 3x3
// zero padding in y) are never read: the taps that would read them are skipped (wave-uniform
// test per row).  Each wave keeps ALL its weights (32 output channels x 9 taps x Cin) in
// registers for the whole band, loaded once.
// MFMA as the DIRECT halo epilogue: C = W x X^T with row-permuted weight tiles, so each lane
// ends with 8 consecutive channels of one pixel and stores 16 B; colsum (RCAN avg-pool)
// partial rows per (image row, pixel wave).
// vmcnt bookkeeping per wave: per row [NG staging pieces] [PPW row pieces] .. MFMAs ..
// vmcnt(PPW) (staging landed) [PT stores] [NC colsum stores]; before row s the count of vector
// memory ops younger than row s + 1's pieces is known in closed form (prologue rows, then the
// steady state (PT + NC) + (LA - 2) * ops-per-row) and waited with a run-time vmcnt.
// ------------------------------------------------------------------------------------
// E (the epilogue, fixed at compile time: at one wave per SIMD every run-time branch of a
// per-row epilogue is exposed): bits 0-1 act, 2-3 gate (0 none, 1 pre-residual (g > 0 ? 1 :
// gate_slope), 2 pre-residual GELU'(g), 3 post-residual (g > 0 ? 1 : gate_slope) on output
// channels gcol0..gcol1), 4 res, 5 res2, 6 aux, 7 colsum, 8 row_scale, 9 dot (with 7: the partial
// sums are of y * dot, the dot operand staged like the residuals).
// blocks per CU the band kernel is built for: two for the W 64 forms whose ring + staging fit
// 80 KB of LDS and 256 registers (no second staging operand), one otherwise.  And (round 6) the RCAB
// conv1 dgrad with the dot epilogue (656: residual + dot staging, 82 KB): not for a second band block
// but so that it shares a CU with a side-stream ring wgrad block (78 KB) as the plain residual form
// does -- at one block per CU (the weight image beside the ring, 154 KB) it held whole CUs against the
// side stream and RCAN ran 35.6 vs 33.6 ms
constexpr int band_occ(int W, int E) {
  return W == 64 && (E == 0 || E == 1 || E == 2 || E == 4 || E == 16 || E == 128 || E == 656) ? 2 : 1;
}
// NWV: waves per block, 4 (one per SIMD) or 8 (two per SIMD, each with half the row's pixel
// tiles, so one wave's epilogue and LDS waits overlap the other's MFMAs; the ring and the weight
// image shared).  8 at W 128: RRDB 63.8 -> 61.0 ms; at W 64 (one pixel tile per wave) RCAN
// 33.8 -> 37.0 ms, so 4 there.
template <int CO, int W, int LA, int KH, int E, int NWV = 4>
__global__ __launch_bounds__(NWV * 64, NWV == 8 ? 2 : band_occ(W, E)) void conv3x3_fwd_band_kernel(FwdArgs a) {
  constexpr int ACT = E & EPI_ACT, GATE = (E >> EPI_GATE_SHIFT) & EPI_GATE;
  constexpr bool RES = (E & EPI_RES) != 0, RES2 = (E & EPI_RES2) != 0, AUX = (E & EPI_AUX) != 0, CS = (E & BAND_CS) != 0,
                 RSC = (E & BAND_RSC) != 0, DOT = (E & BAND_DOT) != 0, STRIP = (E & BAND_STRIP) != 0;
  static_assert(!DOT || CS, "band: dot partials need colsum");
  static_assert(!STRIP || (!CS && !RSC), "band: column strips carry no per-image epilogue");
  constexpr int IR = GATE ? 1 : 0, IR2 = IR + (RES ? 1 : 0), ID = IR2 + (RES2 ? 1 : 0), NSTG = ID + (DOT ? 1 : 0);
  static_assert(NWV == 4 || (NWV == 8 && W / 16 / (8 / (CO / 32)) >= 1), "band: a pixel tile per wave");
  constexpr int WC = CO / 32;       // waves along output channels (32 each = 2 co tiles)
  constexpr int WP = NWV / WC;      // waves along the row's pixels
  constexpr int PT = W / 16 / WP;   // 16-pixel tiles per wave
  constexpr int WPAD = W + 2;
  constexpr int SLOT = WPAD * 128;
  constexpr int S = LA + 2;         // ring slots: rows s-1 .. s+1 read, s+2 .. s+LA in flight
  constexpr int PPW = W / 8 / NWV;  // 1-KB DMA pieces per wave per row
  constexpr int NG = NSTG * PT;     // staging pieces per wave per row (gate / res / res2)
  constexpr int NC = (CS ? 2 : 0) + (AUX ? PT : 0);  // stores after the PT output stores
  constexpr int PPWX = PPW + (STRIP ? 1 : 0);  // + the strip's border piece (or a dummy) per wave
  constexpr int KROW = NG + PPWX + PT + NC;           // vector memory ops per wave per row
  // per-wave staging (none for the wide strip forms without epilogue operands, CO > 64: their LDS is
  // the weight image's)
  constexpr int EPI = (NSTG ? NSTG : (CO > 64 ? 0 : 1)) * PT * 1024;
  constexpr int CIN = 32 * KH;
  constexpr int WROW = 9 * CIN * 2;  // bytes of one output channel's weights [tap][ci]
  constexpr int WBYTES = CO * WROW;
  constexpr int RING = (S + 1) * SLOT + NWV * EPI;
  // ring + one all-zero slot (the rows above / below an image read it, so the MFMA sequence has
  // no branches) + staging; the weight image after them where both fit (WSEP: the ring prologue
  // is issued before the weights are waited for; only forms built for one block per CU: the extra
  // LDS would cost the W 64 forms their second block and RCAN 2.7 ms), else in the same space
  // before the ring starts
  constexpr bool WSEP = band_occ(W, E) == 1 && RING + WBYTES <= 160 * 1024;
  __shared__ __attribute__((aligned(16))) char smem[WSEP ? RING + WBYTES : (RING > WBYTES ? RING : WBYTES)];
  char* const wimg = smem + (WSEP ? RING : 0);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wc = w % WC, wp = w / WC;
  const int g = lane >> 4, c16 = lane & 15;
  const int H = a.H;
  // STRIP (E bit 10): the image is a.W = strips x W pixels wide and each band row is one W-px column
  // strip of an image row, strip rows ordered (image, strip, y) so a band streams down a strip; the
  // strip's two border columns are real pixels of its neighbours (one extra 1-KB piece per row from
  // waves 0 / 1, a zero dummy from the others), and with in_up = 2 the pieces gather the nearest
  // upsample of a half-size input
  const int strips = STRIP ? a.W / W : 1;
  const int HS = H * strips;
  const int T = a.N * HS;  // output rows (strip rows)
  struct RowG { size_t base; int y, irow, x0; };  // first pixel, y, image row n*H + y, strip x origin
  auto row_geom = [&](int q) -> RowG {
    if constexpr (!STRIP) {
      return RowG{(size_t)q * W, q % H, q, 0};
    } else {
      const int nq = q / HS, rem = q - nq * HS, j = rem / H, y = rem - j * H;
      return RowG{(size_t)(nq * H + y) * a.W + j * W, y, nq * H + y, j * W};
    }
  };
  const int upsh = STRIP && a.in_up == 2 ? 1 : 0;
  // input offset (bytes, chunk lc) of pixel sx of image row irow (STRIP)
  auto src_off = [&](int irow, int sx, int lc) -> uint32_t {
    const size_t px = (size_t)(irow >> upsh) * (a.W >> upsh) + (sx >> upsh);
    return (uint32_t)((px * a.ldx + a.xcoff + lc * 8) * 2);
  };
#ifdef SR_BAND_STAMPS
  const unsigned long long t_start = __builtin_readcyclecounter();
  unsigned long long ph[4] = {0ull, 0ull, 0ull, 0ull};  // row wait / barrier / MFMA / epilogue
#endif
  const int G = gridDim.x;
  const int bb = blockIdx.x;
  const int s0 = (int)((int64_t)bb * T / G), s1 = (int)((int64_t)(bb + 1) * T / G);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const __amdgpu_buffer_rsrc_t wr = make_rsrc(a.w, a.w_bytes);
  const __amdgpu_buffer_rsrc_t gr = make_rsrc(a.gate, a.g_bytes);
  const __amdgpu_buffer_rsrc_t rr = make_rsrc(a.res, a.r_bytes);
  const __amdgpu_buffer_rsrc_t rr2 = make_rsrc(a.res2, a.r2_bytes);
  const __amdgpu_buffer_rsrc_t dr = make_rsrc(a.dot, a.d_bytes);

  // weights: one coalesced LDS-DMA image [co][tap][ci] (1 KB contiguous per wave instruction),
  // then each wave reads its MFMA fragments from it: co = wc*32 + 8*(c16>>2) + 4*c + (c16&3)
  // (DIRECT row permutation), K chunk kk*32 + 8*g of every tap
  for (int p = w; p < WBYTES / 1024; p += NWV) {
    const int e = p * 1024 + lane * 16;
    const int co = e / WROW, off = e - co * WROW;
    if constexpr (STRIP) {  // Cin may be 8 / 16 / 24 below CIN (the RRDBNet conv_last dgrad): zero-padded per tap
      const int tap = off / (CIN * 2), cib = off - tap * (CIN * 2);
      glds16(wr, wimg + p * 1024, cib < a.Cin * 2 ? (uint32_t)(co * a.ldw * 2 + tap * a.Cin * 2 + cib) : SR_OOB);
    } else {
      glds16(wr, wimg + p * 1024, (uint32_t)(co * a.ldw * 2 + off));
    }
  }
  const int nn = wc * 32 + 8 * g;  // this lane's 8 output channels
  float bv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bv[j] = 0.f;
  if (a.bias) {
    const f32x4 b0 = *(const f32x4*)(a.bias + nn), b1 = *(const f32x4*)(a.bias + nn + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) { bv[j] = b0[j]; bv[4 + j] = b1[j]; }
  }
  float rsv = a.alpha;  // RSC: alpha * row_scale of image s0 / H + lane (a band spans < 64 images)
  if constexpr (RSC) {
    const int ni = s0 / H + lane;
    rsv = ni < a.N ? a.alpha * a.row_scale[ni] : 0.f;
  }
  u32x4 bw[9][2][2];
  auto read_weights = [&]() {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int co = wc * 32 + 8 * (c16 >> 2) + 4 * c + (c16 & 3);
          bw[tap][kk][c] = kk < KH ? *(const u32x4*)(wimg + co * WROW + (tap * CIN + kk * 32 + 8 * g) * 2)
                                   : u32x4{0u, 0u, 0u, 0u};
        }
    // every fragment in registers (and the compiler knows it) before the ring overwrites the image
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int c = 0; c < 2; ++c) asm volatile("" ::"v"(bw[tap][kk][c]));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };
  auto zero_borders = [&]() {  // pixel rows 0 and W + 1 of every slot (STRIP: DMA'd per row), and the zero slot S
    for (int i = tid; i < (STRIP ? 0 : S * 2 * 8); i += NWV * 64) {
      const int sl = i >> 4, side = (i >> 3) & 1, ch = i & 7;
      *(u32x4*)(smem + sl * SLOT + (side ? (W + 1) * 128 : 0) + ch * 16) = u32x4{0u, 0u, 0u, 0u};
    }
    for (int i = tid; i < SLOT / 16; i += NWV * 64) *(u32x4*)(smem + S * SLOT + i * 16) = u32x4{0u, 0u, 0u, 0u};
  };
  if constexpr (!WSEP) {
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(bv[j]));
    asm volatile("" ::"v"(rsv));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    read_weights();
    __syncthreads();
    zero_borders();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
  } else {
    zero_borders();  // disjoint from the weight image and from the pixel rows the prologue DMAs
  }
#ifdef SR_BAND_STAMPS
  const unsigned long long t_loaded = __builtin_readcyclecounter();
#endif

  // DMA of global row q (pixels 1..W of slot q % S); rows outside [0, T) read zeros
  const int lc_lane = lane & 7;
  auto issue_row = [&](int q) {
    char* slot = smem + (q % S) * SLOT;
    const bool qv = q >= 0 && q < T;
    RowG rg{};
    if constexpr (STRIP) rg = row_geom(q);
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int k = w * PPW + j;            // piece: pixel rows 1 + 8k .. 8 + 8k
      const int px = 1 + 8 * k + (lane >> 3);
      const int lc = lc_lane ^ (px & 7);    // logical 16-B chunk landing in physical slot lane & 7
      const bool v = qv && lc * 8 < a.Cin;
      uint32_t off;
      if constexpr (STRIP) off = src_off(rg.irow, rg.x0 + px - 1, lc);
      else off = (uint32_t)((((size_t)q * W + (px - 1)) * a.ldx + a.xcoff + lc * 8) * 2);
      glds16(xr, slot + (1 + 8 * k) * 128, v ? off : SR_OOB);
    }
    if constexpr (STRIP) {
      // wave 0: slot pixels 0..7 (the left border, 1..7 again as piece 0 has them), wave 1: W-6..W+1
      // (W+1 the right border): a rewrite of the same bytes is harmless.  The image's outer columns
      // load as zeros (OOB).  Other waves: one zero dummy into the zero slot (uniform vmcnt counts).
      if (w < 2) {
        const int pb = w == 0 ? 0 : W - 6;
        const int px = pb + (lane >> 3);
        const int lc = lc_lane ^ (px & 7);
        const int sx = rg.x0 + px - 1;
        const bool v = qv && (unsigned)sx < (unsigned)a.W && lc * 8 < a.Cin;
        glds16(xr, slot + pb * 128, v ? src_off(rg.irow, sx, lc) : SR_OOB);
      } else {
        glds16(xr, smem + S * SLOT, SR_OOB);
      }
    }
  };
  const bool gok = GATE != 3 || (nn >= a.gcol0 && nn < a.gcol1);
  const bool rok = nn < a.rcols;
  auto unpack8 = [](const u32x4& q, float* o) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[2 * j] = bf16_to_f32(q[j] & 0xffff);
      o[2 * j + 1] = bf16_to_f32(q[j] >> 16);
    }
  };
  char* epi = smem + (S + 1) * SLOT + w * EPI;
  // gate / res / res2 of this wave's pixels of output row q into its staging buffer (NG ops)
  auto issue_staging = [&](int q) {
    const bool qv = q < T;
    const size_t mb = row_geom(q).base;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const size_t m = mb + wp * PT * 16 + i * 16 + c16;
      if constexpr (GATE != 0)
        glds16(gr, epi + i * 1024, qv && gok ? (uint32_t)((m * a.ldg + a.gcoff + nn) * 2) : SR_OOB);
      if constexpr (RES)
        glds16(rr, epi + (IR * PT + i) * 1024, qv && rok ? (uint32_t)((m * a.ldr + a.rcoff + nn) * 2) : SR_OOB);
      if constexpr (RES2)
        glds16(rr2, epi + (IR2 * PT + i) * 1024, qv && rok ? (uint32_t)((m * a.ldr2 + a.r2coff + nn) * 2) : SR_OOB);
      if constexpr (DOT)
        glds16(dr, epi + (ID * PT + i) * 1024, qv ? (uint32_t)((m * a.ldd + a.dcoff + nn) * 2) : SR_OOB);
    }
  };
  // prologue: rows s0 - 1 .. s0 + LA - 1 (s0 - 1 first: the oldest), then row s0's staging
  if (s0 < s1) {
    for (int q = s0 - 1; q < s0 + LA; ++q) issue_row(q);
    issue_staging(s0);
  }
  if constexpr (WSEP) {
    // this wave's weight pieces landed (older than the (LA + 1) * PPW + NG prologue ops just
    // issued), then every wave's; the zeros visible to every wave
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(bv[j]));
    asm volatile("" ::"v"(rsv));
    vm_wait_dyn(s0 < s1 ? (LA + 1) * PPWX + NG : 0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    read_weights();
  }
  const int n0 = s0 / H;
  float cst[8];  // band-reduced channel sums (a.cs_band)
#pragma unroll
  for (int j = 0; j < 8; ++j) cst[j] = 0.f;

  // Per row, in issue order: [MFMAs] [epilogue] [staging of row s + 1: NG] [pieces of row
  // s + LA: PPW] [stores: PT + NC].  Vector memory ops complete in issue order, so a wait for
  // one op is a wait for every older one: the row pieces and the staging are issued after the
  // epilogue, so neither wait below ever covers the stores or the DMA of the row just issued.
#pragma unroll 1
  for (int s = s0; s < s1; ++s) {
#ifdef SR_BAND_STAMPS
    const unsigned long long t0 = __builtin_readcyclecounter();
#endif
    // rows <= s + 1 landed: the ops issued after row s + 1's pieces may stay in flight
    if (s + 1 >= s0 + LA) {
      constexpr int STEADY = (PT + NC) + (LA - 2) * KROW;
      static_assert(STEADY <= 63, "band: too many vector memory ops in flight for vmcnt");
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(STEADY) : "memory");
    } else {
      vm_wait_dyn((s0 + LA - 2 - s) * PPWX + NG + (s - s0) * KROW);
    }
#ifdef SR_BAND_STAMPS
    const unsigned long long t1 = __builtin_readcyclecounter();
#endif
    // every wave's pieces of row s + 1 are in LDS, and every wave is done with row s - 2,
    // whose slot row s + LA reuses (S = LA + 2)
    pp_barrier();
#ifdef SR_BAND_STAMPS
    const unsigned long long t2 = __builtin_readcyclecounter();
#endif
    const RowG rgs = row_geom(s);
    const int n_img = STRIP ? 0 : s / H, y = rgs.y;

    f32x4 acc[PT][2];
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
      for (int c = 0; c < 2; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int sl1 = s % S;
    const int sl0 = y == 0 ? S : (sl1 == 0 ? S - 1 : sl1 - 1);      // zero slot above an image
    const int sl2 = y == H - 1 ? S : (sl1 == S - 1 ? 0 : sl1 + 1);  // ... and below it
    const char* srows[3] = {smem + sl0 * SLOT, smem + sl1 * SLOT, smem + sl2 * SLOT};
    // K steps (tap, K half) in order.  Fragment reads run FD - 1 K steps ahead of the MFMAs.  They
    // are inline-asm ds_reads with hand-counted lgkmcnt waits that pass the fragments through (so
    // no MFMA can be scheduled before its wait): the compiler otherwise sinks every read to just
    // before its use and exposes the full LDS latency per 2 MFMAs (one wave per SIMD has nothing
    // else to run).
    constexpr int NK = 9 * KH;
    constexpr int FD = PT >= 8 ? 2 : 5;  // 8 pixel tiles (CO 256 over 8 waves): 2 K steps of fragments
    u32x4 fa[FD][PT];
    uint32_t rbase[3];
#pragma unroll
    for (int ty = 0; ty < 3; ++ty)
      rbase[ty] = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)srows[ty];
    auto read_k = [&](int k, u32x4 (&dst)[PT]) {
      const int tap = k / KH, kk = k % KH, ty = tap / 3, tx = tap % 3;
#pragma unroll
      for (int i = 0; i < PT; ++i) {
        const uint32_t ad = rbase[ty] + swz128(wp * PT * 16 + i * 16 + c16 + tx, kk * 4 + g);
        asm volatile("ds_read_b128 %0, %1" : "=v"(dst[i]) : "v"(ad));
      }
    };
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < FD - 1; ++k) read_k(k, fa[k]);
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if (k + FD - 1 < NK) read_k(k + FD - 1, fa[(k + FD - 1) % FD]);
      const int ahead = (NK - 1 - k < FD - 1 ? NK - 1 - k : FD - 1) * PT;  // reads issued after step k's
      u32x4* f = fa[k % FD];
      if constexpr (PT == 1) {
        switch (ahead) {
          case 0: asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0])); break;
          case 1: asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(f[0])); break;
          case 2: asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f[0])); break;
          case 3: asm volatile("s_waitcnt lgkmcnt(3)" : "+v"(f[0])); break;
          default: asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f[0])); break;
        }
      } else if constexpr (PT == 2) {
        switch (ahead) {
          case 0: asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1])); break;
          case 2: asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(f[0]), "+v"(f[1])); break;
          case 4: asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f[0]), "+v"(f[1])); break;
          case 6: asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(f[0]), "+v"(f[1])); break;
          default: asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f[0]), "+v"(f[1])); break;
        }
      } else if constexpr (PT == 8) {
        if (ahead == 0)
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]),
                       "+v"(f[6]), "+v"(f[7]));
        else
          asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]),
                       "+v"(f[6]), "+v"(f[7]));
      } else {
        switch (ahead) {
          case 0: asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3])); break;
          case 4: asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3])); break;
          case 8: asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3])); break;
          case 12: asm volatile("s_waitcnt lgkmcnt(12)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3])); break;
          default: asm volatile("s_waitcnt lgkmcnt(15)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3])); break;
        }
      }
      const int tap = k / KH, kk = k % KH;
#pragma unroll
      for (int i = 0; i < PT; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) mfma_chunk<bf16_t>(bw[tap][kk][c], f[i], acc[i][c]);
    }
    // The compiler interleaves the epilogue's accumulator reads with the last MFMAs and, on a
    // branchy path, once left too few wait states between the final MFMA and the read of its
    // result (acc[PT-1][1][3] came out stale).  Fence the MFMA block and pad it.
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 3" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#ifdef SR_BAND_STAMPS
    const unsigned long long t3 = __builtin_readcyclecounter();
#endif

    // this row's staging landed (issued before row s + LA - 1's pieces and row s - 1's stores)
    if constexpr (NG > 0) {
      if (s == s0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPWX + PT + NC) : "memory");
    }
    float rs = a.alpha;
    if constexpr (RSC) rs = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, rsv), n_img - n0));
    float cs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cs[j] = 0.f;
    u32x4 ov[PT], avx[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) { v[r] = acc[i][0][r] + bv[r]; v[4 + r] = acc[i][1][r] + bv[4 + r]; }
      if constexpr (AUX) {  // activation side output (act_aux_n: GELU' for GELU)
        float ax[8];
        act_aux_n(v, ax, ACT, a.slope);
#pragma unroll
        for (int j = 0; j < 4; ++j) avx[i][j] = pack_bf16x2(ax[2 * j], ax[2 * j + 1]);
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
      if constexpr (GATE != 0) unpack8(*(const u32x4*)(epi + i * 1024 + lane * 16), gf);
      if constexpr (GATE == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= gf[j] > 0.f ? 1.f : a.gate_slope;
      } else if constexpr (GATE == 2) {  // the stored GELU'
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= gf[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= rs;
      if constexpr (RES) {
        float rf[8];
        unpack8(*(const u32x4*)(epi + (IR * PT + i) * 1024 + lane * 16), rf);
        if (rok) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = a.beta * rf[j] + v[j];
        }
      }
      if constexpr (RES2) {
        float rf[8];
        unpack8(*(const u32x4*)(epi + (IR2 * PT + i) * 1024 + lane * 16), rf);
        if (rok) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = a.beta2 * rf[j] + v[j];
        }
      }
      if constexpr (GATE == 3) {
        if (gok) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= gf[j] > 0.f ? 1.f : a.gate_slope;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) ov[i][j] = pack_bf16x2(v[2 * j], v[2 * j + 1]);
      if constexpr (CS && DOT) {  // y as stored times the dot operand
        float df[8];
        unpack8(*(const u32x4*)(epi + (ID * PT + i) * 1024 + lane * 16), df);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          cs[2 * j] += bf16_to_f32(ov[i][j] & 0xffff) * df[2 * j];
          cs[2 * j + 1] += bf16_to_f32(ov[i][j] >> 16) * df[2 * j + 1];
        }
      } else if constexpr (CS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          cs[2 * j] += bf16_to_f32(ov[i][j] & 0xffff);
          cs[2 * j + 1] += bf16_to_f32(ov[i][j] >> 16);
        }
      }
    }
    if constexpr (NG > 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging read before refill
    issue_staging(s + 1);
    issue_row(s + LA);
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const size_t m = rgs.base + wp * PT * 16 + i * 16 + c16;
      *(u32x4*)((bf16_t*)a.y + m * a.ldy + a.ycoff + nn) = ov[i];
    }
    if constexpr (AUX) {
#pragma unroll
      for (int i = 0; i < PT; ++i) {
        const size_t m = rgs.base + wp * PT * 16 + i * 16 + c16;
        *(u32x4*)((bf16_t*)a.aux + m * a.ldy + a.ycoff + nn) = avx[i];
      }
    }
    if constexpr (CS) {
      // the 16 lanes of a g group hold the same 8 channels: fixed-order butterfly, then lane
      // c16 == 0 writes partial row s * WP + wp (P = H * WP rows per image) -- or, band-reduced
      // (a.cs_band: every band is a.cs_band rows of one image), the running sum over the band's rows
      // so far to partial row bb * WP + wp, so the last row's store leaves the band's sum
      // (P = H / cs_band * WP rows per image; same-address stores of one wave land in order)
      // Band-reduced: each lane keeps its own sums over the band's rows and the butterfly runs once, at
      // the band's last row (it costs ~1300 cycles per row at one wave per SIMD: 32 cross-lane moves in
      // 4 dependent rounds); the rows before store the lane's unreduced running sum to the same
      // address, which the last row's store overwrites (the two stores per row keep the vmcnt counts)
      if (a.cs_band) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { cst[j] += cs[j]; cs[j] = cst[j]; }
        if (s + 1 == s1) {
#pragma unroll
          for (int off = 1; off < 16; off <<= 1)
#pragma unroll
            for (int j = 0; j < 8; ++j) cs[j] += __shfl_xor(cs[j], off, 64);
        }
      } else {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1)
#pragma unroll
          for (int j = 0; j < 8; ++j) cs[j] += __shfl_xor(cs[j], off, 64);
      }
      float* dstp = a.colsum + ((size_t)(a.cs_band ? bb : s) * WP + wp) * a.Cout + nn;
      // exactly two vector store instructions per wave (lanes masked): counted in NC
      if (c16 == 0) *(f32x4*)dstp = f32x4{cs[0], cs[1], cs[2], cs[3]};
      if (c16 == 0) *(f32x4*)(dstp + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
    }
#ifdef SR_BAND_STAMPS
    const unsigned long long t4 = __builtin_readcyclecounter();
    ph[0] += t1 - t0; ph[1] += t2 - t1; ph[2] += t3 - t2; ph[3] += t4 - t3;
#endif
  }
#ifdef SR_BAND_STAMPS
  if (a.stamps && tid == 0) {
    unsigned long long* st = a.stamps + (size_t)blockIdx.x * 16;
    st[0] = t_start; st[1] = t_loaded; st[2] = __builtin_readcyclecounter(); st[3] = s1 - s0;
    st[4] = ph[0]; st[5] = ph[1]; st[6] = ph[2]; st[7] = ph[3];
  }
#endif
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing row pieces (zeros past T) land before exit
}

// the whole-row forms on NWV waves per block (band_nwv)
template <int NWV>
hipError_t launch_band_rows(const FwdArgs& a, hipStream_t s) {
  FwdArgs ab = a;
  ab.stamps = g_sr_stamps;
  ab.cs_band = a.colsum ? band_cs_rows(a) : 0;
  const dim3 grid(band_grid(a.N * a.H)), blk(NWV * 64);
  const int e = band_epi(a, grid.x);
  if (e == 656) {  // instantiated for the RCAN shapes only
    if (a.W == 64) hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 64, 5, 2, 656>), grid, dim3(256), 0, s, ab);
    else hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 128, 3, 2, 656, NWV>), grid, blk, 0, s, ab);
    return hipGetLastError();
  }
#define SR_BAND_E(CO_, W_, LA_, KH_, E_) \
  case E_: hipLaunchKernelGGL((conv3x3_fwd_band_kernel<CO_, W_, LA_, KH_, E_, NWV>), grid, blk, 0, s, ab); break;
#define SR_BAND(CO_, W_, LA_, KH_) \
  if (a.Cout == CO_ && a.W == W_ && a.Cin == 32 * KH_) { \
switch (e) { \
  SR_BAND_E(CO_, W_, LA_, KH_, 0) SR_BAND_E(CO_, W_, LA_, KH_, 1) SR_BAND_E(CO_, W_, LA_, KH_, 2) \
  SR_BAND_E(CO_, W_, LA_, KH_, 4) SR_BAND_E(CO_, W_, LA_, KH_, 16) SR_BAND_E(CO_, W_, LA_, KH_, 20) \
  SR_BAND_E(CO_, W_, LA_, KH_, 28) \
  SR_BAND_E(CO_, W_, LA_, KH_, 48) SR_BAND_E(CO_, W_, LA_, KH_, 72) SR_BAND_E(CO_, W_, LA_, KH_, 128) \
  SR_BAND_E(CO_, W_, LA_, KH_, 304) \
  default: return hipErrorInvalidValue; \
} \
return hipGetLastError(); \
  }
  if constexpr (NWV == 4) {  // W 64: one pixel tile per wave
    SR_BAND(64, 64, 5, 2) SR_BAND(64, 64, 5, 1) SR_BAND(32, 64, 5, 2) SR_BAND(32, 64, 5, 1)
  }
  SR_BAND(64, 128, 3, 2) SR_BAND(64, 128, 3, 1) SR_BAND(32, 128, 4, 2) SR_BAND(32, 128, 4, 1)
#undef SR_BAND
#undef SR_BAND_E
  return hipErrorInvalidValue;
}
hipError_t launch_band_strip(const FwdArgs& a, hipStream_t s) {
  const int rows = a.N * a.H * (a.W / 128);
  FwdArgs ab = a;
  ab.stamps = g_sr_stamps;
  const dim3 grid(band_grid(rows));
  if (a.Cin <= 32 && a.Cout > 64) {  // plain epilogue only (fwd_use_band_strip)
    if (a.Cout == 256) hipLaunchKernelGGL((conv3x3_fwd_band_kernel<256, 128, 3, 1, 1024, 8>), grid, dim3(512), 0, s, ab);
    else hipLaunchKernelGGL((conv3x3_fwd_band_kernel<128, 128, 3, 1, 1024, 8>), grid, dim3(512), 0, s, ab);
    return hipGetLastError();
  }
  if (a.Cin <= 32) {
    switch (band_epi(a, grid.x)) {
      case 0: hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 128, 3, 1, 1024, 8>), grid, dim3(512), 0, s, ab); break;
      case 4: hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 128, 3, 1, 1028, 8>), grid, dim3(512), 0, s, ab); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  switch (band_epi(a, grid.x)) {
    case 0: hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 128, 3, 2, 1024, 8>), grid, dim3(512), 0, s, ab); break;
    case 1: hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 128, 3, 2, 1025, 8>), grid, dim3(512), 0, s, ab); break;
    case 2: hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 128, 3, 2, 1026, 8>), grid, dim3(512), 0, s, ab); break;
    case 4: hipLaunchKernelGGL((conv3x3_fwd_band_kernel<64, 128, 3, 2, 1028, 8>), grid, dim3(512), 0, s, ab); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

namespace sr_conv {

hipError_t launch_band(const FwdArgs& a, hipStream_t s) {
  if (a.W > 128 || a.in_up != 1) return launch_band_strip(a, s);
  return band_nwv(a) == 8 ? launch_band_rows<8>(a, s) : launch_band_rows<4>(a, s);
}

}  // namespace sr_conv
