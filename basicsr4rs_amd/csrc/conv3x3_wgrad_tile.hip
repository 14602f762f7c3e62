// conv3x3 weight / bias gradient on GEMM tiles, split-K into an fp32 slab (WgArgs in conv3x3_args.h has the
// GEMM view): the generic conv3x3_wgrad_kernel (bf16 and exact f32, 16..128-wide tiles) and the 256 x 256
// conv3x3_wgrad_big_kernel / conv3x3_wgrad_pp_kernel, with their launches.
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

// 32-byte-block XOR swizzle for the [K rows][256 B] tr-read image (tools/lds_banks.py):
// the 8 rows a 32-lane half reads ({0..3, 8..11} + base) land on 8 distinct blocks.
SR_DEV uint32_t swz_tr(uint32_t row, uint32_t byte_in_row, uint32_t row_bytes) {
  const uint32_t f = (row & 3u) | (((row >> 3) & 1u) << 2);
  const uint32_t blk = (byte_in_row >> 5) ^ (f & ((row_bytes >> 5) - 1));
  return row * row_bytes + (blk << 5) + (byte_in_row & 31u);
}

template <typename T, int BMW, int BNW, int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_kernel(WgArgs a) {
  constexpr int PER = Elt<T>::PER16;
  constexpr int SZ = Elt<T>::SIZE;
  constexpr bool BF = (SZ == 2);
  constexpr int KSTEP = BF ? 64 : 32;  // pixels per K-step
  constexpr int MI = BMW / WM / 16;
  constexpr int NI = BNW / WN / 16;
  constexpr int ARB = BMW * SZ;  // bytes per A row (one pixel's co tile)
  constexpr int BRB = BNW * SZ;
  constexpr int ACPR = ARB / 16, BCPR = BRB / 16;  // chunks per row
  constexpr int ACH = KSTEP * ACPR, BCH = KSTEP * BCPR;  // chunks per tile
  constexpr int A_PT = (ACH + 255) / 256, B_PT = (BCH + 255) / 256;
  constexpr int STAGE = KSTEP * (ARB + BRB);
  constexpr int SMEM = 2 * STAGE > 256 * 8 * 4 ? 2 * STAGE : 256 * 8 * 4;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  // block -> (split, tap, co tile, ci tile); splits outermost so concurrent blocks share
  // the same pixel range (dy / x rows re-read from L2).
  const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
  const int per_split = a.taps * a.tiles_co * a.tiles_ci;
  const int split = (int)b / per_split;
  int rem = (int)b - split * per_split;
  const int tap = rem / (a.tiles_co * a.tiles_ci);
  rem -= tap * a.tiles_co * a.tiles_ci;
  const int co0 = (rem / a.tiles_ci) * BMW;
  const int ci0 = (rem % a.tiles_ci) * BNW;
  const int etap = tap + a.tap0;
  const int dy_ = etap / 3 - 1, dx_ = etap % 3 - 1;
  const int p_begin = split * a.kper;
  const int p_end = min(a.M, p_begin + a.kper);
  const bool do_bias = (etap == 4) && (ci0 == 0) && a.wsb != nullptr;

  const __amdgpu_buffer_rsrc_t dyr = make_rsrc(a.dy, a.dy_bytes);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);

  u32x4 ra[A_PT], rb[B_PT];
  float bacc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto pix_decomp = [&](int p, int& nh, int& y, int& x) {
    uint32_t q = fdiv((uint32_t)p, a.fd_W);
    x = p - (int)q * a.W;
    uint32_t n = fdiv(q, a.fd_H);
    y = (int)q - (int)n * a.H;
    nh = (int)n * a.H;
  };

  auto load = [&](int p0) {
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int c = tid + 256 * i;
      const int row = c / ACPR, cc = c % ACPR;
      const int p = p0 + row;
      const int co = co0 + cc * PER;
      bool v = (c < ACH) && p < p_end && co < a.Cout;
      uint32_t off = SR_OOB;
      if (v) {
        if (a.out_ps == 0) {
          off = (uint32_t)(((size_t)p * a.ldy + a.ycoff + co) * SZ);
        } else {
          int nh, y, x;
          pix_decomp(p, nh, y, x);
          const int r = a.out_ps;
          const int s = (int)fdiv((uint32_t)co, a.fd_cps);
          const int cch = co - s * a.fd_cps.d;
          const int si = s / r, sj = s - (s / r) * r;
          off = (uint32_t)((((size_t)((nh + y) * r + si) * (a.W * r) + x * r + sj) * a.ldy + a.ycoff + cch) * SZ);
        }
      }
      ra[i] = buf_load16(dyr, off);
    }
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int c = tid + 256 * i;
      const int row = c / BCPR, cc = c % BCPR;
      const int p = p0 + row;
      const int ci = ci0 + cc * PER;
      bool v = (c < BCH) && p < p_end && ci < a.Cin;
      uint32_t off = SR_OOB;
      if (v) {
        int nh, y, x;
        pix_decomp(p, nh, y, x);
        const int yy = y + dy_, xx = x + dx_;
        if ((unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W) {
          const int u = a.in_up;
          off = (uint32_t)(((size_t)((nh / u + yy / u) * (a.W / u) + xx / u) * a.ldx + a.xcoff + ci) * SZ);
        }
      }
      rb[i] = buf_load16(xr, off);
    }
  };
  auto bias_accum = [&]() {
    // every A chunk a thread loads covers the same 8 (or 4) channels across K-steps
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      if (BF) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bacc[2 * j] += bf16_to_f32(ra[i][j] & 0xffff);
          bacc[2 * j + 1] += bf16_to_f32(ra[i][j] >> 16);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) bacc[j] += __uint_as_float(ra[i][j]);
      }
    }
  };
  auto store = [&](int buf) {
    char* As = smem + buf * STAGE;
    char* Bs = As + KSTEP * ARB;
#pragma unroll
    for (int i = 0; i < A_PT; ++i) {
      const int c = tid + 256 * i;
      if (c < ACH) {
        const int row = c / ACPR, cc = c % ACPR;
        const uint32_t o = BF ? swz_tr(row, cc * 16, ARB) : (uint32_t)(row * ARB + cc * 16);
        *(u32x4*)(As + o) = ra[i];
      }
    }
#pragma unroll
    for (int i = 0; i < B_PT; ++i) {
      const int c = tid + 256 * i;
      if (c < BCH) {
        const int row = c / BCPR, cc = c % BCPR;
        const uint32_t o = BF ? swz_tr(row, cc * 16, BRB) : (uint32_t)(row * BRB + cc * 16);
        *(u32x4*)(Bs + o) = rb[i];
      }
    }
  };
  auto compute = [&](int buf) {
    const char* As = smem + buf * STAGE;
    const char* Bs = As + KSTEP * ARB;
    if constexpr (BF) {
      const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        s16x8 fa[MI], fb[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
          const int col = wm * (BMW / WM) + i * 16 + 4 * p;  // co column of this lane's address
          const int r0 = kk * 32 + 8 * g + q;
          s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(As + swz_tr(r0, col * 2, ARB)));
          s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(As + swz_tr(r0 + 4, col * 2, ARB)));
          fa[i] = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          const int col = wn * (BNW / WN) + j * 16 + 4 * p;
          const int r0 = kk * 32 + 8 * g + q;
          s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(Bs + swz_tr(r0, col * 2, BRB)));
          s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(Bs + swz_tr(r0 + 4, col * 2, BRB)));
          fb[j] = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    } else {
      const int k = lane >> 4, c16 = lane & 15;
#pragma unroll 4
      for (int ks = 0; ks < KSTEP; ks += 4) {
        float fa[MI], fb[NI];
#pragma unroll
        for (int i = 0; i < MI; ++i)
          fa[i] = *(const float*)(As + (ks + k) * ARB + (wm * (BMW / WM) + i * 16 + c16) * 4);
#pragma unroll
        for (int j = 0; j < NI; ++j)
          fb[j] = *(const float*)(Bs + (ks + k) * BRB + (wn * (BNW / WN) + j * 16 + c16) * 4);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
          for (int j = 0; j < NI; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    }
  };

  const int nk = (p_end - p_begin + KSTEP - 1) / KSTEP;
  if (nk > 0) {
    load(p_begin);
    if (do_bias) bias_accum();
    store(0);
  }
  __syncthreads();
  for (int ks = 0; ks < nk; ++ks) {
    const bool more = ks + 1 < nk;
    if (more) load(p_begin + (ks + 1) * KSTEP);
    compute(ks & 1);
    if (more) {
      if (do_bias) bias_accum();
      store((ks + 1) & 1);
    }
    __syncthreads();
  }

  // partial tile -> slab ws[split][tap][co][ci]; C/D layout: row = co, col = ci
  float* ws = a.ws + ((size_t)split * a.taps + tap) * a.Cout * a.Cin;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wm * (BMW / WM) + i * 16 + (lane >> 4) * 4 + r;
        const int ci = ci0 + wn * (BNW / WN) + j * 16 + (lane & 15);
        if (co < a.Cout && ci < a.Cin) ws[(size_t)co * a.Cin + ci] = acc[i][j][r];
      }

  if (do_bias) {
    float* red = (float*)smem;  // [256][8]
#pragma unroll
    for (int j = 0; j < 8; ++j) red[tid * 8 + j] = bacc[j];
    __syncthreads();
    if (tid < BMW) {
      const int cc = tid / PER, j = tid % PER;
      float s = 0.f;
      // threads whose A chunks are chunk cc of a row: tid' with (tid' + 256 i) % ACPR == cc
      for (int t2 = 0; t2 < 256; ++t2)
        if ((t2 % ACPR) == cc && t2 < ACH) s += red[t2 * 8 + j];
      if (co0 + tid < a.Cout) a.wsb[(size_t)split * a.Cout + co0 + tid] = s;
    }
  }
}

// ------------------------------------------------------------------------------------
// 256 (co) x 256 (ci) weight-gradient tile per tap for bf16, Cout >= 256 and Cin >= 256.
// Same LDS-DMA pipeline as conv3x3_fwd_big_kernel: the [64 pixels][256 ch] images of dy and
// of the tap-shifted x arrive by buffer_load ... lds (two 64 KB stages, counted vmcnt, raw
// barriers); MFMA operands need 8 consecutive pixels per lane and are read transposed
// with ds_read_b64_tr_b16 from 32-byte-block XOR-swizzled 512-byte rows (the swizzle is
// applied to the per-lane DMA source chunk).  The bias gradient of the centre-tap blocks
// is one extra MFMA per A fragment against an all-ones B operand (dy^T . 1).
// ------------------------------------------------------------------------------------
SR_DEV uint32_t swz512(uint32_t row, uint32_t byte_in_row) {
  const uint32_t f = (row & 3u) | (((row >> 3) & 1u) << 2);
  return row * 512u + ((((byte_in_row >> 5) ^ f)) << 5) + (byte_in_row & 31u);
}

// Bias-gradient role of the wgrad launch: the [64 pixels][256 co] dy image of each K-step
// (same LDS-DMA pipeline, A operand only) times an all-ones B operand on MFMA.
SR_DEV void wgrad_bias_role(const WgArgs& a, char* smem, int split, int co0) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p_begin = split * a.kper;
  const int p_end = min(a.M, p_begin + a.kper);
  const __amdgpu_buffer_rsrc_t dyr = make_rsrc(a.dy, a.dy_bytes);
  constexpr int STAGE = 2 * 64 * 512;
  int lc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int R = 8 * w + 2 * j + (lane >> 5);
    const int f = (R & 3) | (((R >> 3) & 1) << 2);
    lc[j] = ((((lane & 31) >> 1) ^ f) << 1) | (lane & 1);
  }
  auto issue = [&](int p0, int buf) {
    char* As = smem + buf * STAGE + w * 4096;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int R = 8 * w + 2 * j + (lane >> 5);
      const int p = p0 + R;
      const bool pv = p < p_end;
      const int pc = pv ? p : 0;
      const int co = co0 + lc[j] * 8;
      uint32_t off;
      if (a.out_ps == 0) {
        off = (uint32_t)((pc * a.ldy + a.ycoff + co) * 2);
      } else {
        uint32_t q = fdiv((uint32_t)pc, a.fd_W);
        const int x = pc - (int)q * a.W;
        const int r = a.out_ps;
        const int s = (int)fdiv((uint32_t)co, a.fd_cps);
        const int cch = co - s * a.fd_cps.d;
        const int si = s / r, sj = s - (s / r) * r;
        off = (uint32_t)((((int)q * r + si) * (a.W * r) + x * r + sj) * a.ldy + a.ycoff + cch) * 2;
      }
      glds16(dyr, As + j * 1024, (pv && co < a.Cout) ? off : SR_OOB);
    }
  };
  const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const int nk = (p_end - p_begin + 63) / 64;
  if (nk > 0) issue(p_begin, 0);
  if (nk > 1) issue(p_begin + 64, 1);
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk)
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const char* As = smem + (ks & 1) * STAGE;
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int r0 = kk * 32 + 8 * g + q;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int col = w * 32 + i * 16 + 4 * pp;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(As + swz512(r0, col * 2)));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(As + swz512(r0 + 4, col * 2)));
        const s16x8 fa = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, ones, accb[i], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (ks + 2 < nk) issue(p_begin + (ks + 2) * 64, ks & 1);
  }
  if ((lane & 15) == 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + w * 32 + i * 16 + (lane >> 4) * 4 + r;
        if (co < a.Cout) a.wsb[(size_t)split * a.Cout + co] = accb[i][r];
      }
  }
}

__global__ __launch_bounds__(512) void conv3x3_wgrad_big_kernel(WgArgs a) {
  constexpr int MI = 8, NI = 4;
  constexpr int STAGE = 2 * 64 * 512;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;
  // block -> (split, role): roles 0 .. 9*tco*tci-1 are (tap, co tile, ci tile) GEMM tiles,
  // the last tco roles (present only when db is wanted) are bias-gradient blocks.
  const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
  const int ntile = a.taps * a.tiles_co * a.tiles_ci;
  const int per_split = ntile + (a.wsb ? a.tiles_co : 0);
  const int split = (int)b / per_split;
  int rem = (int)b - split * per_split;
  if (rem >= ntile) {
    wgrad_bias_role(a, smem, split, (rem - ntile) * 256);
    return;
  }
  const int tap = rem / (a.tiles_co * a.tiles_ci);
  rem -= tap * a.tiles_co * a.tiles_ci;
  const int co0 = (rem / a.tiles_ci) * 256;
  const int ci0 = (rem % a.tiles_ci) * 256;
  const int etap = tap + a.tap0;
  const int dy_ = etap / 3 - 1, dx_ = etap % 3 - 1;
  const int p_begin = split * a.kper;
  const int p_end = min(a.M, p_begin + a.kper);
  const __amdgpu_buffer_rsrc_t dyr = make_rsrc(a.dy, a.dy_bytes);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);

  // DMA rows of this lane: R_j = 8w + 2j + (lane >> 5); logical 16-B chunk lc_j (source swizzle)
  int lc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int R = 8 * w + 2 * j + (lane >> 5);
    const int f = (R & 3) | (((R >> 3) & 1) << 2);
    lc[j] = ((((lane & 31) >> 1) ^ f) << 1) | (lane & 1);
  }

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto issue = [&](int p0, int buf) {
    char* As = smem + buf * STAGE + w * 4096;
    char* Bs = As + 32768;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int R = 8 * w + 2 * j + (lane >> 5);
      const int p = p0 + R;
      const bool pv = p < p_end;
      const int pc = pv ? p : 0;
      uint32_t q = fdiv((uint32_t)pc, a.fd_W);
      const int x = pc - (int)q * a.W;
      uint32_t n = fdiv(q, a.fd_H);
      const int y = (int)q - (int)n * a.H;
      const int co = co0 + lc[j] * 8;
      uint32_t offa;
      if (a.out_ps == 0) {
        offa = (uint32_t)((pc * a.ldy + a.ycoff + co) * 2);
      } else {
        const int r = a.out_ps;
        const int s = (int)fdiv((uint32_t)co, a.fd_cps);
        const int cch = co - s * a.fd_cps.d;
        const int si = s / r, sj = s - (s / r) * r;
        offa = (uint32_t)((((int)q * r + si) * (a.W * r) + x * r + sj) * a.ldy + a.ycoff + cch) * 2;
      }
      glds16(dyr, As + j * 1024, (pv && co < a.Cout) ? offa : SR_OOB);
      const int yy = y + dy_, xx = x + dx_;
      const int ci = ci0 + lc[j] * 8;
      const bool bv = pv && ci < a.Cin && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
      const uint32_t offb = (uint32_t)((((int)q + dy_) * a.W + xx) * a.ldx + a.xcoff + ci) * 2;
      glds16(xr, Bs + j * 1024, bv ? offb : SR_OOB);
    }
  };

  auto compute = [&](int buf) {
    const char* As = smem + buf * STAGE;
    const char* Bs = As + 32768;
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int r0 = kk * 32 + 8 * g + q;
      s16x8 fa[MI], fb[NI];
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int col = wn * 64 + j * 16 + 4 * pp;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(Bs + swz512(r0, col * 2)));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(Bs + swz512(r0 + 4, col * 2)));
        fb[j] = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int col = wm * 128 + i * 16 + 4 * pp;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(As + swz512(r0, col * 2)));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(As + swz512(r0 + 4, col * 2)));
        fa[i] = s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  };

  const int nk = (p_end - p_begin + 63) / 64;
  if (nk > 0) issue(p_begin, 0);
  if (nk > 1) issue(p_begin + 64, 1);
  for (int ks = 0; ks < nk; ++ks) {
    if (ks + 1 < nk)
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    compute(ks & 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (ks + 2 < nk) issue(p_begin + (ks + 2) * 64, ks & 1);
  }

  float* ws = a.ws + ((size_t)split * a.taps + tap) * a.Cout * a.Cin;
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + wm * 128 + i * 16 + (lane >> 4) * 4 + r;
        const int ci = ci0 + wn * 64 + j * 16 + (lane & 15);
        if (co < a.Cout && ci < a.Cin) ws[(size_t)co * a.Cin + ci] = acc[i][j][r];
      }
}

// ------------------------------------------------------------------------------------
// Weight gradient, phase-interleaved 256x256 (co x ci) tile: the schedule of
// conv3x3_fwd_pp_kernel applied to the per-tap GEMM over pixels.  Half-tiles are
// [64 pixels][128 channels] images (256-B rows, 32-B-block swizzle, ds_read_b64_tr_b16
// operand reads): A_h = dy channels co0 + h*128.., B_g = x channels ci0 + g*128.. at the
// tap-shifted pixel.  Needs W % 64 == 0 (a 64-pixel K-step is one image-row segment, so
// the tap's zero padding is a wave-uniform row test plus a per-lane column test and every
// source offset is a scalar per-step base + a per-lane constant) and Cout, Cin (and the
// shuffle slot width) multiples of 128.  Output: fp32 slab tile staged through LDS and
// written with 16-B row-contiguous stores.
// ------------------------------------------------------------------------------------
// P2: the two-interval schedule of conv3x3_fwd_pph_kernel<.., P2> -- R1 reads A half 0 and both B
// halves and issues all four half-tiles of step t+1 (their buffer was last read at R2 of step t-1
// by both groups), two quadrants per MFMA interval, R2 reads A half 1; the leading group retires
// step t+1's DMAs after issuing its second MFMA interval, the lagging group at the end of its R2.
template <bool P2 = false>
__global__ __launch_bounds__(512) void conv3x3_wgrad_pp_kernel(WgArgs a) {
  constexpr int STAGE = 65536;
  constexpr int CSTR = 256 + 4;
  constexpr int SMEM = 128 * CSTR * 4;
  static_assert(SMEM >= 2 * STAGE, "LDS too small");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w >> 2, wc = w & 3;
  const uint32_t b = xcd_remap(blockIdx.x, gridDim.x);
  const int ntile = a.taps * a.tiles_co * a.tiles_ci;
  int split, rem;
  if (a.bias_group > 0) {
    // tile blocks first; the bias-role blocks (light: dy only) each take bias_group splits, so
    // fewer CUs sit on them and the tile blocks get more splits (shorter K ranges)
    if ((int)b >= a.splits * ntile) {
      const int bb = (int)b - a.splits * ntile;
      const int grp = bb / a.tiles_co, co_t = bb - grp * a.tiles_co;
      const int s1 = min(a.splits, (grp + 1) * a.bias_group);
      for (int sp = grp * a.bias_group; sp < s1; ++sp) {
        if (sp > grp * a.bias_group) __syncthreads();  // the previous split's LDS stages are free
        wgrad_bias_role(a, smem, sp, co_t * 256);
      }
      return;
    }
    split = (int)b / ntile;
    rem = (int)b - split * ntile;
  } else {
    const int per_split = ntile + (a.wsb && !a.bias_fused ? a.tiles_co : 0);
    split = (int)b / per_split;
    rem = (int)b - split * per_split;
    if (rem >= ntile) {
      wgrad_bias_role(a, smem, split, (rem - ntile) * 256);
      return;
    }
  }
  const int tap = rem / (a.tiles_co * a.tiles_ci);
  rem -= tap * a.tiles_co * a.tiles_ci;
  const int co0 = (rem / a.tiles_ci) * 256;
  const int ci0 = (rem % a.tiles_ci) * 256;
  const int etap = tap + a.tap0;
  const int dy_ = etap / 3 - 1, dx_ = etap % 3 - 1;
  const int p_begin = split * a.kper;
  const int p_end = min(a.M, p_begin + a.kper);
  const __amdgpu_buffer_rsrc_t dyr = make_rsrc(a.dy, a.dy_bytes);
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(a.x, a.x_bytes);
  const int rps = a.out_ps > 0 ? a.out_ps : 1;

  // DMA rows of this lane: R_j = 8w + 4j + (lane >> 4), 16-B slot lane & 15 holding the
  // logical chunk lc_j of the swizzled 256-B row.
  int Rj[2];
  uint32_t la[2], lb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int R = 8 * w + 4 * j + (lane >> 4);
    const int f = (R & 3) | (((R >> 3) & 1) << 2);
    const int sl = lane & 15;
    const int lc = (((sl >> 1) ^ f) << 1) | (sl & 1);
    Rj[j] = R;
    la[j] = (uint32_t)(R * rps * a.ldy) * 2u + (uint32_t)lc * 16u;
    lb[j] = (uint32_t)(R * a.ldx) * 2u + (uint32_t)lc * 16u;
  }

  // scalar state of the K-step being issued
  int s_ua0 = 0, s_ua1 = 0, s_ub = 0, s_x0 = 0, s_left = 0, s_yv = 0;
  auto k_eval = [&](int ks) {
    const int p0s = p_begin + ks * 64;
    const int q = (int)fdiv((uint32_t)p0s, a.fd_W);
    const int x0 = p0s - q * a.W;
    const int n = (int)fdiv((uint32_t)q, a.fd_H);
    const int y = q - n * a.H;
    int ua[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int cu = co0 + h * 128;
      if (a.out_ps == 0) {
        ua[h] = (p0s * a.ldy + a.ycoff + cu) * 2;
      } else {
        const int r = a.out_ps;
        const int sl = (int)fdiv((uint32_t)cu, a.fd_cps);
        const int cch = cu - sl * a.fd_cps.d;
        const int si = sl / r, sj = sl - si * r;
        ua[h] = (((q * r + si) * (a.W * r) + x0 * r + sj) * a.ldy + a.ycoff + cch) * 2;
      }
    }
    s_ua0 = __builtin_amdgcn_readfirstlane(ua[0]);
    s_ua1 = __builtin_amdgcn_readfirstlane(ua[1]);
    s_ub = __builtin_amdgcn_readfirstlane((((q + dy_) * a.W + x0 + dx_) * a.ldx + a.xcoff + ci0) * 2);
    s_x0 = __builtin_amdgcn_readfirstlane(x0 + dx_);
    s_left = __builtin_amdgcn_readfirstlane(p_end - p0s);
    s_yv = __builtin_amdgcn_readfirstlane((unsigned)(y + dy_) < (unsigned)a.H ? 1 : 0);
  };
  constexpr uint32_t SLOT_A0 = 0, SLOT_A1 = 16384, SLOT_B0 = 32768, SLOT_B1 = 49152;
  auto issue_a = [&](int ks, int h) {
    char* dst = smem + (ks & 1) * STAGE + (h ? SLOT_A1 : SLOT_A0) + w * 2048;
    const uint32_t ua = (uint32_t)(h ? s_ua1 : s_ua0);
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(dyr, dst + j * 1024, Rj[j] < s_left ? ua + la[j] : SR_OOB);
  };
  auto issue_b = [&](int ks, int g) {
    char* dst = smem + (ks & 1) * STAGE + (g ? SLOT_B1 : SLOT_B0) + w * 2048;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool v = s_yv && Rj[j] < s_left && (unsigned)(s_x0 + Rj[j]) < (unsigned)a.W;
      glds16(xr, dst + j * 1024, v ? (uint32_t)s_ub + (uint32_t)g * 256u + lb[j] : SR_OOB);
    }
  };

  const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
  s16x8 fa[2][4], fb[2][2][2];  // fa[kk][i] (current A half), fb[g][kk][j]
  auto tr8 = [&](const char* base, int r0, int col) -> s16x8 {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(base + swz_tr(r0, col * 2, 256)));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)(base + swz_tr(r0 + 4, col * 2, 256)));
    return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  auto read_a = [&](int buf, int h) {
    const char* As = smem + buf * STAGE + (h ? SLOT_A1 : SLOT_A0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[kk][i] = tr8(As, kk * 32 + 8 * tg + tq, wr * 64 + i * 16 + 4 * tp);
  };
  auto read_b = [&](int buf, int g) {
    const char* Bs = smem + buf * STAGE + (g ? SLOT_B1 : SLOT_B0);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[g][kk][j] = tr8(Bs, kk * 32 + 8 * tg + tq, wc * 32 + j * 16 + 4 * tp);
  };
  f32x4 acc[2][2][4][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[h][g][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // fused bias (a.bias_fused): the centre-tap blocks of the first ci tile also sum dy over their
  // pixels -- wave (wr, wc) takes A row block i = wc of each half against a ones operand
  const bool bias_here = a.bias_fused && a.wsb && tap == a.taps / 2 && ci0 == 0;
  const s16x8 ones = {0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
  f32x4 accb[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  auto mma = [&](int h, int g) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[h][g][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][i], fb[g][kk][j], acc[h][g][i][j], 0, 0, 0);
    if (g == 0 && bias_here) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (wc == 0) accb[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][0], ones, accb[h], 0, 0, 0);
        else if (wc == 1) accb[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][1], ones, accb[h], 0, 0, 0);
        else if (wc == 2) accb[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][2], ones, accb[h], 0, 0, 0);
        else accb[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[kk][3], ones, accb[h], 0, 0, 0);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  const int nk = (p_end - p_begin + 63) / 64;  // >= 1 (every split owns >= 1 pixel)
  k_eval(0);
  issue_a(0, 0);
  issue_b(0, 0);
  issue_b(0, 1);
  issue_a(0, 1);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  pp_barrier();
  if (wr) pp_barrier();
  for (int t = 0; t < nk; ++t) {
    const int buf = t & 1;
    const bool more = t + 1 < nk;
    if constexpr (P2) {
      // step 0's four half-tiles were retired by the prologue's vmcnt(4) only partly: drain once
      if (t == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); pp_barrier(); pp_barrier(); }
      read_a(buf, 0);
      read_b(buf, 0);
      read_b(buf, 1);
      if (more) {
        k_eval(t + 1);
        issue_a(t + 1, 0);
        issue_b(t + 1, 0);
        issue_b(t + 1, 1);
        issue_a(t + 1, 1);
      }
      pp_barrier();
      mma(0, 0);
      mma(0, 1);
      pp_barrier();
      read_a(buf, 1);
      // A half 1 is read here and re-filled at the other group's next R1 (one interval later):
      // these reads complete before the barrier
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (wr) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      pp_barrier();
      mma(1, 1);
      mma(1, 0);
      if (!wr) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      pp_barrier();
      continue;
    }
    read_a(buf, 0);
    read_b(buf, 0);
    if (more) {
      k_eval(t + 1);
      issue_a(t + 1, 0);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    }
    pp_barrier();
    mma(0, 0);
    pp_barrier();
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
    read_a(buf, 1);
    if (more) issue_b(t + 1, 1);
    pp_barrier();
    mma(1, 1);
    pp_barrier();
    if (more) {
      issue_a(t + 1, 1);
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    }
    pp_barrier();
    mma(1, 0);
    pp_barrier();
  }
  if (!wr) pp_barrier();

  if (bias_here && (lane & 15) == 0) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + h * 128 + wr * 64 + wc * 16 + (lane >> 4) * 4 + r;
        if (co < a.Cout) a.wsb[(size_t)split * a.Cout + co] = accb[h][r];
      }
  }
  float* ws = a.ws + ((size_t)split * a.taps + tap) * a.Cout * a.Cin;
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
    for (int idx = tid; idx < 128 * 64; idx += 512) {
      const int row = idx >> 6, c4 = (idx & 63) * 4;
      const int co = co0 + h * 128 + row, ci = ci0 + c4;
      if (co < a.Cout && ci < a.Cin)
        *(f32x4*)(ws + (size_t)co * a.Cin + ci) = *(const f32x4*)(Cs + row * CSTR + c4);
    }
  }
}

// Wave grid (WM x WN = 4) for a BMW x BNW wgrad tile: every wave needs >= one 16x16 tile.
constexpr int wg_wm(int bm, int bn) {
  return (bm >= 32 && bn >= 32) ? 2 : (bm >= 64 ? 4 : 1);
}

template <typename T, int BMW, int BNW>
hipError_t launch_wg(WgArgs a, hipStream_t s) {
  constexpr int WM = wg_wm(BMW, BNW);
  constexpr int WN = 4 / WM;
  static_assert(BMW / WM >= 16 && BNW / WN >= 16, "wgrad tile too small for 4 waves");
  a.tiles_co = (a.Cout + BMW - 1) / BMW;
  a.tiles_ci = (a.Cin + BNW - 1) / BNW;
  const int blocks = a.splits * a.taps * a.tiles_co * a.tiles_ci;
  hipLaunchKernelGGL((conv3x3_wgrad_kernel<T, BMW, BNW, WM, WN>), dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <typename T>
hipError_t dispatch_wg(const WgArgs& a, hipStream_t s) {
  int bm, bn;
  wg_tiles(a.Cout, a.Cin, &bm, &bn);
#define SR_WG(X, Y) \
  if (bm == X && bn == Y) return launch_wg<T, X, Y>(a, s);
  SR_WG(128, 128) SR_WG(128, 64) SR_WG(64, 128) SR_WG(64, 64) SR_WG(128, 32) SR_WG(32, 128)
  SR_WG(128, 16) SR_WG(16, 128) SR_WG(64, 32) SR_WG(32, 64) SR_WG(64, 16) SR_WG(16, 64)
  SR_WG(32, 32)
#undef SR_WG
  return hipErrorInvalidValue;
}

}  // namespace

namespace sr_conv {

hipError_t launch_wg_tile(const WgArgs& a, bool bf16, hipStream_t s) {
  return bf16 ? dispatch_wg<bf16_t>(a, s) : dispatch_wg<float>(a, s);
}

// The 256 x 256 kernels (wg_use_big).
hipError_t launch_wg_big(WgArgs a, const sr_conv3x3_wgrad_desc* d, hipStream_t s) {
  const int S = a.splits, taps = a.taps;
  a.tiles_co = (a.Cout + 255) / 256;
  a.tiles_ci = (a.Cin + 255) / 256;
  a.bias_fused = wg_bias_fused(d) ? 1 : 0;
  a.bias_group = a.bias_fused ? 0 : wg_bias_group(d);
  // bias-role blocks per co tile: none (fused into the centre-tap blocks), one per bias_group splits, or one per split
  const int bias_splits = a.bias_fused || !a.wsb ? 0 : a.bias_group > 0 ? (S + a.bias_group - 1) / a.bias_group : S;
  const dim3 grid(S * taps * a.tiles_co * a.tiles_ci + bias_splits * a.tiles_co);
  if (!wg_use_pp(d)) hipLaunchKernelGGL(conv3x3_wgrad_big_kernel, grid, dim3(512), 0, s, a);
  else if (variant_is(SR_VARIANT_FOUR_PHASE)) hipLaunchKernelGGL(conv3x3_wgrad_pp_kernel<false>, grid, dim3(512), 0, s, a);
  else hipLaunchKernelGGL(conv3x3_wgrad_pp_kernel<true>, grid, dim3(512), 0, s, a);
  return hipGetLastError();
}

}  // namespace sr_conv
