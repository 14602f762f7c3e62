// conv3x3 weight gradient, second pass: the deterministic reduce of the split-K slab into dw / db
// (wgrad_reduce_kernel and its narrow, grouped, 4-wide and transposed-slab forms) and the launch that picks
// one for a sr_conv3x3_wgrad call.
#include "conv3x3_args.h"
#include "conv3x3_dev.h"

using namespace sr_conv;

namespace {

// dw[co][ci][ky][kx] = scale * sum_s ws[s][tap][co'][ci], co' = GEMM column of co (out_ps
// permutation); one thread per (co, ci): slab reads coalesced along ci, 9 taps per thread.
__global__ void wgrad_reduce_kernel(const float* ws, const float* wsb, float* dw, float* db, int S,
                                    int Cout, int Cin, int Cout_real, int Cin_real, int out_ps, int taps,
                                    const int* co_map, const int* ci_map, float scale, int accumulate) {
  const int64_t total = (int64_t)Cout_real * Cin_real;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int r2 = out_ps > 0 ? out_ps * out_ps : 1;
  const int cps = Cout_real / r2;  // C' (channels after shuffle)
  if (i < total) {
    const int ci = (int)(i % Cin_real);
    const int co = (int)(i / Cin_real);
    const int cop = co_map ? co_map[co] : (out_ps > 0 ? (co % r2) * cps + co / r2 : co);  // GEMM column
    const int cip = ci_map ? ci_map[ci] : ci;                                                // GEMM k channel
    const size_t stride = (size_t)taps * Cout * Cin;
    float s[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) s[t] = 0.f;
    for (int k = 0; k < S; ++k) {
      const float* src = ws + k * stride + (size_t)cop * Cin + cip;
#pragma unroll
      for (int t = 0; t < 9; ++t)
        if (t < taps) s[t] += src[(size_t)t * Cout * Cin];
    }
    float* d = dw + i * taps;
#pragma unroll
    for (int t = 0; t < 9; ++t)
      if (t < taps) d[t] = s[t] * scale + (accumulate ? d[t] : 0.f);
  }
  if (db && i < Cout_real) {
    const int co = (int)i;
    const int cop = co_map ? co_map[co] : (out_ps > 0 ? (co % r2) * cps + co / r2 : co);
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += wsb[(size_t)k * Cout + cop];
    db[co] = s * scale + (accumulate ? db[co] : 0.f);
  }
}

// Slab reduction for the RGB head conv (Cin_real <= 8, not a multiple of 4): wgrad_reduce_kernel
// gives each (co, ci) pair ONE thread that walks all S slabs (RRDB conv_first: 192 threads x
// S 1024 = 1.28 ms).  Here one block per output channel: 256 threads split the slabs, each
// keeps 9 x Cin_real (+ bias) partial sums, then a fixed-order LDS tree -- deterministic.
__global__ __launch_bounds__(256) void wgrad_reduce_narrow_kernel(const float* ws, const float* wsb, float* dw,
                                                                  float* db, int S, int Cout, int Cin, int Cin_real,
                                                                  int out_ps, int taps, const int* co_map,
                                                                  const int* ci_map, float scale, int accumulate) {
  constexpr int NV = 9 * 8 + 1;
  __shared__ float red[NV][256];
  const int co = blockIdx.x, t = threadIdx.x;
  const int r2 = out_ps > 0 ? out_ps * out_ps : 1;
  const int cps = (int)gridDim.x / r2;
  const int cop = co_map ? co_map[co] : (out_ps > 0 ? (co % r2) * cps + co / r2 : co);
  int cip[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) cip[c] = c < Cin_real ? (ci_map ? ci_map[c] : c) : 0;
  float s[9][8], sb = 0.f;
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int c = 0; c < 8; ++c) s[tp][c] = 0.f;
  const size_t stride = (size_t)taps * Cout * Cin, tstride = (size_t)Cout * Cin;
  for (int k = t; k < S; k += 256) {
    const float* src = ws + k * stride + (size_t)cop * Cin;
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if (tp < taps && c < Cin_real) s[tp][c] += src[tp * tstride + cip[c]];
    if (db) sb += wsb[(size_t)k * Cout + cop];
  }
#pragma unroll
  for (int tp = 0; tp < 9; ++tp)
#pragma unroll
    for (int c = 0; c < 8; ++c) red[tp * 8 + c][t] = s[tp][c];
  red[NV - 1][t] = sb;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w)
      for (int v = 0; v < NV; ++v) red[v][t] += red[v][t + w];
    __syncthreads();
  }
  if (t < 9 * 8) {
    const int tp = t >> 3, c = t & 7;
    if (tp < taps && c < Cin_real) {
      float* d = dw + ((size_t)co * Cin_real + c) * taps + tp;
      *d = red[t][0] * scale + (accumulate ? *d : 0.f);
    }
  } else if (t == NV - 1 && db) {
    db[co] = red[t][0] * scale + (accumulate ? db[co] : 0.f);
  }
}

// Slab reduction, one kernel for both slab layouts (TR false: [S][taps][Cout][Cin], groups (tap,
// co, 4 ci); TR true: the row-streaming wgrad's [S][taps][Cin][Cout], groups (tap, ci, 4 co)), no
// gathered loads (ci_map with TR false / co_map with TR true go to the kernels below).  A block
// of nw waves holds GPW groups x P = nw * 64 / GPW split phases: lane -> (phase, group), one 16-B
// load per split, GPW * 16 B contiguous per phase and wave instruction, phases k = ph (mod P)
// with 4 independent loads in flight, then a fixed-order LDS combine -- deterministic.  The host
// sizes P to ~8 slabs per thread and GPW so that the grid covers the chip (RCAN: S 256 over 9216
// groups = 288 blocks of 32 groups x 32 phases instead of 144 of 64 x 16).
// CIG (TR false with a ci_map, the SwinIR proj / dense linears over padded head channels): groups run
// over the GEMM columns (16-B loads, no gather) and each sum is stored at its parameter column, through
// the GEMM -> parameter inverse of ci_map built in LDS (-1: a padding column, dropped).  (The gathered
// wgrad_reduce4_kernel it replaces read 36 MB in 60 us in the SwinIR step.)
template <int GPW, bool TR, bool CIG = false>
__global__ __launch_bounds__(1024) void wgrad_reduce_g_kernel(const float* ws, const float* wsb, float* dw, float* db,
                                                              int S, int Cout, int Cin, int Cout_real, int Cin_real,
                                                              int out_ps, int taps, const int* co_map,
                                                              const int* ci_map, float scale, int wblocks,
                                                              int accumulate, WgReduce2 p2) {
  extern __shared__ f32x4 red[];  // nw * 64 entries (dynamic: a 4-wave block needs 4 KB, so it can
                                  // share a CU with the 158 KB pph kernel when it runs on a side stream)
  if (blockIdx.y) {  // grid row 1: the second item of a paired reduce (same shape, S and order of the sums)
    ws = p2.ws; wsb = p2.wsb; dw = p2.dw; db = p2.db; scale = p2.scale;
  }
  const int nw = (int)(blockDim.x >> 6);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r2 = out_ps > 0 ? out_ps * out_ps : 1;
  const int cps = Cout_real / r2;
  if ((int)blockIdx.x >= wblocks) {  // bias: 64 co per block, nw phases
    const int c = ((int)blockIdx.x - wblocks) * 64 + lane;
    float sb = 0.f;
    if (c < Cout_real) {
      const int cop = co_map ? co_map[c] : (out_ps > 0 ? (c % r2) * cps + c / r2 : c);
      for (int k = wv; k < S; k += nw) sb += wsb[(size_t)k * Cout + cop];
    }
    red[wv * 64 + lane] = f32x4{sb, 0.f, 0.f, 0.f};
    __syncthreads();
    if (wv == 0 && c < Cout_real) {
      float sm = red[lane][0];
      for (int k = 1; k < nw; ++k) sm += red[k * 64 + lane][0];
      db[c] = sm * scale + (accumulate ? db[c] : 0.f);
    }
    return;
  }
  const int P = nw * (64 / GPW);
  const int ph = wv * (64 / GPW) + lane / GPW, gl = lane % GPW;
  const int64_t i = (int64_t)blockIdx.x * GPW + gl;
  const int c4n = TR ? (Cout_real + 3) >> 2 : (CIG ? Cin >> 2 : Cin_real >> 2);
  [[maybe_unused]] int* inv = nullptr;
  if constexpr (CIG) {
    __shared__ int inv_s[1024];  // GEMM column -> parameter column (Cin <= 1024, checked on the host)
    inv = inv_s;
    for (int k = threadIdx.x; k < Cin; k += blockDim.x) inv_s[k] = -1;
    __syncthreads();
    for (int c = threadIdx.x; c < Cin_real; c += blockDim.x) inv_s[ci_map[c]] = c;
    __syncthreads();
  }
  const int rows = TR ? Cin_real : Cout_real;
  const int64_t total = (int64_t)taps * rows * c4n;
  int q4 = 0, rw = 0, tap = 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (i < total) {
    q4 = (int)(i % c4n);
    const int64_t t2 = i / c4n;
    rw = (int)(t2 % rows);
    tap = (int)(t2 / rows);
    int rp;
    if (TR) rp = ci_map ? ci_map[rw] : rw;
    else rp = co_map ? co_map[rw] : (out_ps > 0 ? (rw % r2) * cps + rw / r2 : rw);
    const size_t stride = (size_t)taps * Cout * Cin;
    const float* src = ws + ((size_t)tap * (TR ? Cin : Cout) + rp) * (TR ? Cout : Cin) + q4 * 4;
    // 8 independent 16-B loads in flight, and the < 8 left over issued together too (clamped to a
    // valid split, zeroed after the load: no branch, so no load waits for the one before it -- the
    // round-5 form ran its remainder one dependent iteration at a time, e.g. 2-3 of the 6-7 loads per
    // lane at the EDSR body wgrad's 26 splits)
    int k = ph;
    for (; k + 7 * P < S; k += 8 * P) {
      f32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *(const f32x4*)(src + (size_t)(k + j * P) * stride);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += v[j];
    }
    if (k < S) {
      f32x4 v[7];
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const int kj = k + j * P < S ? k + j * P : S - 1;
        v[j] = *(const f32x4*)(src + (size_t)kj * stride);
      }
#pragma unroll
      for (int j = 0; j < 7; ++j)
        if (k + j * P < S) acc += v[j];
    }
  }
  red[ph * GPW + gl] = acc;
  __syncthreads();
  if (ph == 0 && i < total) {
    f32x4 sm = red[gl];
    for (int k = 1; k < P; ++k) sm += red[k * GPW + gl];
    if (TR) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = q4 * 4 + e;
        if (co < Cout_real) {
          float* d = dw + ((size_t)co * Cin_real + rw) * taps + tap;
          *d = sm[e] * scale + (accumulate ? *d : 0.f);
        }
      }
    } else if constexpr (CIG) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int pc = inv[q4 * 4 + e];
        if (pc >= 0) {
          float* d = dw + ((size_t)rw * Cin_real + pc) * taps + tap;
          *d = sm[e] * scale + (accumulate ? *d : 0.f);
        }
      }
    } else {
      float* d = dw + ((size_t)rw * Cin_real + q4 * 4) * taps + tap;
#pragma unroll
      for (int e = 0; e < 4; ++e) d[(size_t)e * taps] = sm[e] * scale + (accumulate ? d[(size_t)e * taps] : 0.f);
    }
  }
}

// Slab reduction for Cin_real % 4 == 0 (16-B loads, or gathered through ci_map): 64 (tap, co, 4 ci) groups per
// 1024-thread block; the 16 waves take splits k = wave (mod 16) with independent 16-B loads
// (coalesced along ci), then a fixed-order LDS combine -- deterministic, and S / 16 loads
// per thread instead of S.  The last ceil(Cout_real / 64) blocks sum the bias slab the same
// way (one co per lane).
__global__ __launch_bounds__(1024) void wgrad_reduce4_kernel(const float* ws, const float* wsb, float* dw, float* db,
                                                             int S, int Cout, int Cin, int Cout_real, int Cin_real,
                                                             int out_ps, int taps, const int* co_map,
                                                             const int* ci_map, float scale, int wblocks,
                                                             int accumulate) {
  __shared__ f32x4 red[16][64];
  const int t = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r2 = out_ps > 0 ? out_ps * out_ps : 1;
  const int cps = Cout_real / r2;
  if ((int)blockIdx.x >= wblocks) {  // bias
    const int c = ((int)blockIdx.x - wblocks) * 64 + t;
    float sb = 0.f;
    if (c < Cout_real) {
      const int cop = co_map ? co_map[c] : (out_ps > 0 ? (c % r2) * cps + c / r2 : c);
      for (int k = wv; k < S; k += 16) sb += wsb[(size_t)k * Cout + cop];
    }
    red[wv][t] = f32x4{sb, 0.f, 0.f, 0.f};
    __syncthreads();
    if (wv == 0 && c < Cout_real) {
      float sm = red[0][t][0];
#pragma unroll
      for (int k = 1; k < 16; ++k) sm += red[k][t][0];
      db[c] = sm * scale + (accumulate ? db[c] : 0.f);
    }
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * 64 + t;
  const int c4n = Cin_real >> 2;
  const int64_t total = (int64_t)taps * Cout_real * c4n;
  int co = 0, ci4 = 0, tap = 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (i < total) {
    ci4 = (int)(i % c4n);
    const int64_t t2 = i / c4n;
    co = (int)(t2 % Cout_real);
    tap = (int)(t2 / Cout_real);
    const int cop = co_map ? co_map[co] : (out_ps > 0 ? (co % r2) * cps + co / r2 : co);
    const size_t stride = (size_t)taps * Cout * Cin;
    const float* row = ws + ((size_t)tap * Cout + cop) * Cin;
    if (ci_map) {  // GEMM channels of the 4 parameter channels (padded heads): gathered loads
      int cip[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) cip[e] = ci_map[ci4 * 4 + e];
      for (int k = wv; k < S; k += 16) {
        const float* sk = row + (size_t)k * stride;
        acc += f32x4{sk[cip[0]], sk[cip[1]], sk[cip[2]], sk[cip[3]]};
      }
    } else {
      const float* src = row + ci4 * 4;
      int k = wv;
      for (; k + 48 < S; k += 64) {
        const f32x4 v0 = *(const f32x4*)(src + (size_t)k * stride);
        const f32x4 v1 = *(const f32x4*)(src + (size_t)(k + 16) * stride);
        const f32x4 v2 = *(const f32x4*)(src + (size_t)(k + 32) * stride);
        const f32x4 v3 = *(const f32x4*)(src + (size_t)(k + 48) * stride);
        acc += v0; acc += v1; acc += v2; acc += v3;
      }
      for (; k < S; k += 16) acc += *(const f32x4*)(src + (size_t)k * stride);
    }
  }
  red[wv][t] = acc;
  __syncthreads();
  if (wv == 0 && i < total) {
    f32x4 sm = red[0][t];
#pragma unroll
    for (int k = 1; k < 16; ++k) sm += red[k][t];
    float* d = dw + ((size_t)co * Cin_real + ci4 * 4) * taps + tap;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[(size_t)e * taps] = sm[e] * scale + (accumulate ? d[(size_t)e * taps] : 0.f);
  }
}

// Slab reduction for the row-streaming wgrad's [S][taps][Cin][Cout] slab: 64 (tap, ci, 4 co)
// groups per 1024-thread block, 16-B loads coalesced along co, the 16 waves take splits
// k = wave (mod 16), fixed-order LDS combine (deterministic); bias blocks as wgrad_reduce4_kernel.
__global__ __launch_bounds__(1024) void wgrad_reduce_tr_kernel(const float* ws, const float* wsb, float* dw, float* db,
                                                               int S, int Cout, int Cin, int Cout_real, int Cin_real,
                                                               int taps, const int* co_map, const int* ci_map,
                                                               float scale, int wblocks, int accumulate, int out_ps) {
  __shared__ f32x4 red[16][64];
  const int t = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r2 = out_ps > 0 ? out_ps * out_ps : 1, cps = Cout_real / r2;
  // GEMM column of parameter output channel c (co_map, or the PixelShuffle order: slot c % r^2)
  auto gcol = [&](int c) { return co_map ? co_map[c] : (out_ps > 0 ? (c % r2) * cps + c / r2 : c); };
  if ((int)blockIdx.x >= wblocks) {  // bias
    const int c = ((int)blockIdx.x - wblocks) * 64 + t;
    float sb = 0.f;
    if (c < Cout_real) {
      const int cop = gcol(c);
      for (int k = wv; k < S; k += 16) sb += wsb[(size_t)k * Cout + cop];
    }
    red[wv][t] = f32x4{sb, 0.f, 0.f, 0.f};
    __syncthreads();
    if (wv == 0 && c < Cout_real) {
      float sm = red[0][t][0];
#pragma unroll
      for (int k = 1; k < 16; ++k) sm += red[k][t][0];
      db[c] = sm * scale + (accumulate ? db[c] : 0.f);
    }
    return;
  }
  const int64_t i = (int64_t)blockIdx.x * 64 + t;
  const int c4n = (Cout_real + 3) >> 2;
  const int64_t total = (int64_t)taps * Cin_real * c4n;
  int co4 = 0, ci = 0, tap = 0;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (i < total) {
    co4 = (int)(i % c4n);
    const int64_t t2 = i / c4n;
    ci = (int)(t2 % Cin_real);
    tap = (int)(t2 / Cin_real);
    const int cip = ci_map ? ci_map[ci] : ci;
    const size_t stride = (size_t)taps * Cin * Cout;
    const float* row = ws + ((size_t)tap * Cin + cip) * Cout;
    if (co_map || out_ps > 0) {  // GEMM columns of the 4 parameter channels: gathered loads
      int cop[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) cop[e] = co4 * 4 + e < Cout_real ? gcol(co4 * 4 + e) : 0;
      for (int k = wv; k < S; k += 16) {
        const float* sk = row + (size_t)k * stride;
        acc += f32x4{sk[cop[0]], sk[cop[1]], sk[cop[2]], sk[cop[3]]};
      }
    } else {
      const float* src = row + co4 * 4;
      int k = wv;
      for (; k + 48 < S; k += 64) {
        const f32x4 v0 = *(const f32x4*)(src + (size_t)k * stride);
        const f32x4 v1 = *(const f32x4*)(src + (size_t)(k + 16) * stride);
        const f32x4 v2 = *(const f32x4*)(src + (size_t)(k + 32) * stride);
        const f32x4 v3 = *(const f32x4*)(src + (size_t)(k + 48) * stride);
        acc += v0; acc += v1; acc += v2; acc += v3;
      }
      for (; k < S; k += 16) acc += *(const f32x4*)(src + (size_t)k * stride);
    }
  }
  red[wv][t] = acc;
  __syncthreads();
  if (wv == 0 && i < total) {
    f32x4 sm = red[0][t];
#pragma unroll
    for (int k = 1; k < 16; ++k) sm += red[k][t];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int co = co4 * 4 + e;
      if (co < Cout_real) {
        float* d = dw + ((size_t)co * Cin_real + ci) * taps + tap;
        *d = sm[e] * scale + (accumulate ? *d : 0.f);
      }
    }
  }
}

}  // namespace

namespace sr_conv {

// The slab reduce of a sr_conv3x3_wgrad call (S splits of its plan, slab ws, bias slab wsb)
int wgrad_reduce_launch(const sr_conv3x3_wgrad_desc* d, int S, int taps, const float* ws, const float* wsb, float* dw,
                        float* db, const int* co_map, const int* ci_map, hipStream_t s, const WgReduce2* second) {
  const int acc1 = d->accumulate & 1;
  const WgReduce2 p2 = second ? *second : WgReduce2{};
  const int Cout_real = d->Cout_real > 0 ? d->Cout_real : d->Cout;
  const int Cin_real = d->Cin_real > 0 ? d->Cin_real : d->Cin;
  const int64_t total = (int64_t)Cout_real * Cin_real;
  const int64_t work = total > Cout_real ? total : Cout_real;
  const bool tr = wg_use_halo(d);
  // (the row-streaming slab keeps wgrad_reduce_tr_kernel: 32-group blocks measured slower on RCAN / RRDB)
  const bool cig = !tr && ci_map && d->Cin % 4 == 0 && d->Cin <= 1024;  // ci gather on the output side
  if (!tr && ((Cin_real % 4 == 0 && !ci_map) || cig)) {
    // split phases P ~ S / 8 (pow2 <= 32), group width GPW so that the grid covers the chip
    const int64_t groups = tr ? (int64_t)taps * Cin_real * ((Cout_real + 3) / 4)
                              : (int64_t)taps * Cout_real * ((cig ? d->Cin : Cin_real) / 4);
    int P = 1;
    while (P * 8 < S && P < 32) P <<= 1;
    int gpw = 64;
    while (gpw > 16 && P * gpw / 64 > 16) gpw >>= 1;  // <= 16 waves
    while (gpw > 16 && (groups + gpw - 1) / gpw < 256 && P * gpw / 64 >= 2) gpw >>= 1;
    const int nw = P * gpw / 64 > 0 ? P * gpw / 64 : 1;
    const int wblocks = (int)((groups + gpw - 1) / gpw);
    const int bblocks = db ? (Cout_real + 63) / 64 : 0;
    const dim3 grid((unsigned)(wblocks + bblocks), second ? 2u : 1u), blk((unsigned)(nw * 64));
#define SR_RG(G, T, ...)                                                                                        \
  hipLaunchKernelGGL((wgrad_reduce_g_kernel<G, T, ##__VA_ARGS__>), grid, blk, (size_t)nw * 64 * 16, s, (const float*)ws, (const float*)wsb, dw, db, \
                     S, d->Cout, d->Cin, Cout_real, Cin_real, d->out_ps, taps, co_map, ci_map, d->scale, wblocks,  \
                     acc1, p2)
    // (the tr arm is never taken under the !tr guard above: the row-streaming slab keeps wgrad_reduce_tr_kernel; its
    // three instantiations stay so that the set of kernels in the library is the parent's)
    if (tr) { if (gpw == 64) SR_RG(64, true); else if (gpw == 32) SR_RG(32, true); else SR_RG(16, true); }
    else if (cig) { if (gpw == 64) SR_RG(64, false, true); else if (gpw == 32) SR_RG(32, false, true); else SR_RG(16, false, true); }
    else { if (gpw == 64) SR_RG(64, false); else if (gpw == 32) SR_RG(32, false); else SR_RG(16, false); }
#undef SR_RG
  } else if (second) {
    return sr_fail(SR_EINVAL, "conv3x3_wgrad reduce: a paired reduce needs the grouped slab reduce (Cin_real % 4 == 0, no maps)");
  } else if (tr) {
    const int64_t work4 = (int64_t)taps * Cin_real * ((Cout_real + 3) / 4);
    const int wblocks = (int)((work4 + 63) / 64);
    const int bblocks = db ? (Cout_real + 63) / 64 : 0;
    hipLaunchKernelGGL(wgrad_reduce_tr_kernel, dim3((unsigned)(wblocks + bblocks)), dim3(1024), 0, s,
                       (const float*)ws, (const float*)wsb, dw, db, S, d->Cout, d->Cin, Cout_real, Cin_real, taps,
                       co_map, ci_map, d->scale, wblocks, acc1, d->out_ps);
  } else if (Cin_real % 4 == 0) {
    const int64_t work4 = (int64_t)taps * Cout_real * (Cin_real / 4);
    const int wblocks = (int)((work4 + 63) / 64);
    const int bblocks = db ? (Cout_real + 63) / 64 : 0;
    hipLaunchKernelGGL(wgrad_reduce4_kernel, dim3((unsigned)(wblocks + bblocks)), dim3(1024), 0, s, (const float*)ws,
                       (const float*)wsb, dw, db, S, d->Cout, d->Cin, Cout_real, Cin_real, d->out_ps, taps, co_map,
                       ci_map, d->scale, wblocks, acc1);
  } else if (Cin_real <= 8 && !variant_is(SR_VARIANT_REDUCE_PLAIN)) {
    hipLaunchKernelGGL(wgrad_reduce_narrow_kernel, dim3((unsigned)Cout_real), dim3(256), 0, s, (const float*)ws,
                       (const float*)wsb, dw, db, S, d->Cout, d->Cin, Cin_real, d->out_ps, taps, co_map, ci_map,
                       d->scale, acc1);
  } else {
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s,
                       (const float*)ws, (const float*)wsb, dw, db, S, d->Cout, d->Cin, Cout_real,
                       Cin_real, d->out_ps, taps, co_map, ci_map, d->scale, acc1);
  }
  return sr_check(hipGetLastError(), "conv3x3_wgrad reduce launch");
}

}  // namespace sr_conv
