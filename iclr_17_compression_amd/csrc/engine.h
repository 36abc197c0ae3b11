// The implicit-GEMM convolution engine of the Ballé-2017 codec on gfx950: everything its kernel
// families share (templates and inline code only; the instantiations and entry points live in
// engine_fp32.hip and deconv3_halo.hip).
//
// One engine covers every layer of the hot path:
//   analysis  conv2/conv3 (k5 s2 p2)            — forward conv, 25 taps, base grid = output grid
//   synthesis deconv1/deconv2 (k5 s2 p2 op1)    — stride-phase decomposition: 4 dense sub-convs
//                                                 (3×3 / 3×2 / 2×3 / 2×2 taps), no zero insertion
//   synthesis deconv3 (k9 s4 p4 op3, N→3)       — "all-phase" GEMM: the 16 output phases × 3
//                                                 channels share one 3×3 input neighbourhood, so
//                                                 they form a dense N = 48 GEMM (K = 9·N)
//   analysis  conv1 (3→N, k9 s4)                — own A-loader (NCHW patch staged in LDS, K = 243)
//
// Tile: 64 output pixels (an 8×8 block of the base grid) × BN output channels per 256-thread
// workgroup (4 waves). GEMM mapping: M = pixels, N = output channels, K = (tap, input channel).
// MFMA: v_mfma_f32_16x16x4_f32 (exact f32), or in the x6 flavour six v_mfma_f32_16x16x32_bf16 part
// products per MAC. Both operands are staged in LDS by LDS-DMA (global_load_lds): the A tile
// (input pixels × 32 channels of one tap; out-of-image taps DMA from a zero line) and the B tile
// (packed weights [tap][Cin/4][Cout][4] of the same step), double buffered, one barrier per k-step.
//
// "float4 k-trick": a lane loads 4 consecutive input channels of its pixel with one 16-byte
// read and feeds them to 4 successive MFMAs; MFMA e of a 16-deep k-block therefore covers
// channels {16kb + 4g + e : g = 0..3}. The weight packing [Cin/4][Cout][4] makes the matching B
// fragment a 16-byte read as well.
//
// Epilogues are fused: bias + GDN/IGDN (a second channel-contraction GEMM over an LDS x² tile
// and the packed γ, then x/√n or x·√n), conv3's quantiser + factorised rate (per-tile bit sums),
// and deconv3's bias + clamp (+ per-tile SSE against the input image). Outputs leave through
// LDS as coalesced 16-byte row stores.
#pragma once

#include <string.h>

#include <type_traits>

#include "common.h"

namespace iclr17 {

constexpr int BM = 64;        // output pixels per tile


enum Epi : int {
  EPI_GDN = 0, EPI_IGDN = 1, EPI_QUANT = 2, EPI_OUT3 = 3, EPI_PLAIN = 4,
  EPI_GDN_BWD = 5, EPI_IGDN_BWD = 6, EPI_RATE_BWD = 7
};

struct TapTable {
  int npx;            // phases along x
  int nph;            // total phases
  int begin[17];      // taps of phase p: [begin[p], begin[p+1])
  int dydx[64];       // (dy + 128) | (dx + 128) << 8 — dword entries so the wave-uniform lookup
                      // is a scalar kernarg load (a byte array becomes a VMEM load + vmcnt(0))
};

__host__ __device__ inline int pack_tap(int dy, int dx) { return (dy + 128) | ((dx + 128) << 8); }

struct EngineArgs {
  const float* in;      // NHWC [B][Hin][Win][CI]   (conv1: NCHW image)
  const float* w;       // packed weights
  const float* bias;    // [CO] or nullptr
  const float* gbeta;   // GDN effective beta [CO]
  const float* ggamma;  // GDN effective gamma, packed [CO/4][CO][4]
  float* out;           // NHWC [B][Hout][Wout][CO]   (deconv3: clipped NCHW image)
  float* pre;           // optional pre-activation output (same layout as out)
  int B, Hin, Win, Hout, Wout;
  int gh, gw;           // base grid per phase
  int tiles_x, tiles_y;
  int sin, sout;        // input / output stride applied to base coordinates
  TapTable tt;
  // conv3 quantiser + rate
  int qmode;
  const float* noise;   // NCHW [B][CO][Hout][Wout]
  const float* rate;    // packed [11][CO]
  const float* rtab;    // round mode, nullable: element_bits of the integer latents −32..32 [CO][65]
  float* yhat;          // NHWC
  double* partial;      // per-tile partial sums
  int partials_per_image;
  // deconv3
  const float* xref;    // NCHW input image (SSE) or nullptr
  float* recon;         // unclipped NCHW or nullptr
  int sse_unclipped;    // SSE of (recon − x) instead of (clipped − x) (training MSE, model.py:61)
  // backward epilogues
  const float* saved;   // GDN/IGDN bwd: the layer's saved pre-activation u (NHWC, output grid);
                        // rate bwd: ỹ (NHWC)
  const float* ggammaT; // γ packed transposed: packed[q][j][e] = γ[4q+e][j]
  float* tout;          // GDN bwd: dn = ∂L/∂n (NHWC) for the parameter gradients
  const float* gscale;  // rate bwd: device scalar ∂L/∂bpp (nullptr → no rate term)
  float count;          // rate bwd: B·H·W (bpp denominator, model.py:78)
  float* rpart;         // rate bwd: per-tile parameter partials [tiles][11][CO]
  float* colsum_out;    // GDN bwd: per-tile column sums of ∂u (the conv bias gradient) [tiles][CO]
  float* colsum_t;      // GDN bwd: per-tile column sums of dn (∂β_eff) [tiles][CO]
  // x6 mode: activations as three bf16 planes (hi, mid, lo; x = hi + mid + lo exactly)
  const unsigned short* in_split;   // [3][B][Hin][Win][CI]
  long in_plane;                    // plane stride (elements)
  unsigned short* out_split;        // [3][B][Hout][Wout][CO] or nullptr
  long out_plane;
  // chunk-major split form [3][B][C/32][h][w][32] (deconv2 → deconv3 x6: a 32-channel chunk of a
  // patch row is contiguous, so the halo kernel's chunks do not share cache lines). out_cm: the
  // writer (store_tile_rows_split), in_cm: the reader (deconv3_x6_kernel)
  int out_cm, in_cm;
  const unsigned short* ggamma6;    // x6: γ_eff split, [3][CO/8][CO][8] bf16 (plane CO·CO)
  const unsigned short* ggammaT6;   // x6 backward: the transposed packing of γ_eff, split
  // deconv3 (x6 / bf16): conv3's bit partials [B][fold_T] reduced by workgroup 0 before its tile
  // (fold_bits: reduce_partials_kernel's arithmetic and order), or nullptr
  const double* fold_partial;
  int fold_T;
  double* fold_per_image;   // [B] or nullptr
  // x6 conv3 (W6 instantiation): the weights pre-split into three bf16 planes
  // (iclr17_split_packed(w_packed, 25, CI, CO): [3][25][CI/8][CO][8]) instead of split per k-step
  const unsigned short* w6;
  long w6_plane;
  float* fold_total;        // scale · Σ, 0-dim
  double fold_scale;
  // deconv3 in the h3 form (deconv3_x6_kernel<CI, true>): the input as two fp16 planes
  // (in_split) and the weights pre-split into two fp16 planes whose packing trailer holds
  // 2⁻¹¹/(σ_a·σ_w) at wscale[1]; range: the chain's h3 range flag (read only, the NaN poison)
  const float* wscale;
  int* range;
};

// iclr17_reduce_partials inside the last kernel of the eval chain (deconv3): the per-image sums of
// conv3's T bit partials and scale · their total, by workgroup 0 before its own tile, which saves
// the chain a kernel launch and boundary. Arithmetic and order are reduce_partials_kernel's
// (csrc/aux.hip): per image a lane-strided sum over t ≡ lane (mod 64) in t order, a fixed xor
// butterfly, then the images added in order by thread 0 — so the results are bit-identical.
// The loads of a wave's images go out together (one memory latency for the common T ≤ 64).
// poison: the h3 range flag was set upstream (deconv3_x6_kernel<CI, true>); every total is NaN.
template <int NTHR>
__device__ __forceinline__ void fold_bits(const EngineArgs& a, double* img /* LDS, 64 doubles */,
                                          bool poison = false) {
  constexpr int NW = NTHR / 64, KI = (64 + NW - 1) / NW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = a.fold_T;
  double acc = 0.0;
  for (int b0 = 0; b0 < a.B; b0 += 64) {
    const int nb = a.B - b0 < 64 ? a.B - b0 : 64;
    double v[KI];
#pragma unroll
    for (int k = 0; k < KI; ++k) {
      const int b = wave + k * NW;
      v[k] = b < nb && lane < T ? a.fold_partial[(long)(b0 + b) * T + lane] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < KI; ++k) {
      const int b = wave + k * NW;
      if (b >= nb) continue;
      double s = 0.0 + v[k];
      for (int t = lane + 64; t < T; t += 64) s += a.fold_partial[(long)(b0 + b) * T + t];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (poison) s = __builtin_nan("");
      if (lane == 0) {
        img[b] = s;
        if (a.fold_per_image) a.fold_per_image[b0 + b] = s;
      }
    }
    __syncthreads();
    if (threadIdx.x == 0)
      for (int b = 0; b < nb; ++b) acc += img[b];
    __syncthreads();
  }
  if (threadIdx.x == 0 && a.fold_total) *a.fold_total = (float)(acc * a.fold_scale);
}

struct TileInfo {
  int b, ty, tx, py, px, nb;
  int th;   // tile height in base-grid rows (tile = th × 8 base pixels)
};

template <int TH = 8>
__device__ __forceinline__ TileInfo decode_tile(const EngineArgs& a) {
  TileInfo t;
  t.th = TH;
  int bid = blockIdx.x;
  // stride phases in dispatch order 0..3 (9, 6, 6, 4 taps): longest workgroups first
  const int per_ph = a.tiles_x * a.tiles_y * a.B;
  const int ph = bid / per_ph;
  bid -= ph * per_ph;
  t.tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  t.ty = bid % a.tiles_y;
  bid /= a.tiles_y;
  t.b = bid;
  t.py = ph / a.tt.npx;
  t.px = ph % a.tt.npx;
  t.nb = blockIdx.y;
  return t;
}

// Row m of a tile → output pixel (NHWC row offset in pixels) or -1 when outside the grid.
__device__ __forceinline__ long out_pixel(const EngineArgs& a, const TileInfo& t, int m) {
  const int gy = t.ty * t.th + (m >> 3), gx = t.tx * 8 + (m & 7);
  if (gy >= a.gh || gx >= a.gw) return -1;
  const int oy = gy * a.sout + t.py, ox = gx * a.sout + t.px;
  return ((long)t.b * a.Hout + oy) * a.Wout + ox;
}

// Store an [R][BN] tile held in LDS (row stride ld) to NHWC rows of CO floats at column
// offset col0, 16 bytes per lane, rows outside the grid skipped (T threads).
template <int BN, int R = BM, int T = 256>
__device__ __forceinline__ void store_tile_rows(const EngineArgs& a, const TileInfo& t,
                                                const float* s, int ld, float* dst, int CO,
                                                int col0) {
  constexpr int C4 = BN / 4;
  for (int idx = threadIdx.x; idx < R * C4; idx += T) {
    const int m = idx / C4, c4 = idx % C4;
    const long p = out_pixel(a, t, m);
    if (p < 0) continue;
    const f4 v = *(const f4*)(s + m * ld + c4 * 4);
    *(f4*)(dst + p * CO + col0 + c4 * 4) = v;
  }
}

// Inverse of store_tile_rows: NHWC rows of the tile's pixels → LDS (zeros outside the grid).
template <int BN>
__device__ __forceinline__ void load_tile_rows(const EngineArgs& a, const TileInfo& t,
                                               const float* __restrict__ src, float* s, int ld,
                                               int CO, int col0) {
  constexpr int C4 = BN / 4;
  for (int idx = threadIdx.x; idx < BM * C4; idx += 256) {
    const int m = idx / C4, c4 = idx % C4;
    const long p = out_pixel(a, t, m);
    const f4 v = p < 0 ? f4{0.f, 0.f, 0.f, 0.f} : *(const f4*)(src + p * CO + col0 + c4 * 4);
    *(f4*)(s + m * ld + c4 * 4) = v;
  }
}

// Store a [BM][BN] LDS tile (row stride ld) as the three bf16 planes of the x6 activation
// format (rows of CO channels, columns col0 ..), 8 channels (16 bytes per plane) per lane.
template <int BN, int R = BM, int T = 256>
__device__ __forceinline__ void store_tile_rows_split(const EngineArgs& a, const TileInfo& t,
                                                      const float* s, int ld, int CO, int col0) {
  constexpr int C8 = BN / 8;
  for (int idx = threadIdx.x; idx < R * C8; idx += T) {
    const int m = idx / C8, c8 = idx % C8;
    const long p = out_pixel(a, t, m);
    if (p < 0) continue;
    u4 hi, mi, lo;
    split8(*(const f4*)(s + m * ld + c8 * 8), *(const f4*)(s + m * ld + c8 * 8 + 4), hi, mi, lo);
    unsigned short* d = a.out_split + p * CO + col0 + c8 * 8;
    if (a.out_cm) {   // [B][C/32][h][w][32]: image b, chunk c, pixel q of the image
      const long hw = (long)a.Hout * a.Wout, b = p / hw, q = p - b * hw;
      const int c = col0 + c8 * 8;
      d = a.out_split + ((b * (CO / 32) + (c >> 5)) * hw + q) * 32 + (c & 31);
    }
    *(u4*)d = hi;
    *(u4*)(d + a.out_plane) = mi;
    *(u4*)(d + 2 * a.out_plane) = lo;
  }
}

// Column sums of an LDS tile [BM][ld] over the rows inside the output grid → dst[blockIdx.x][CO],
// fixed row order (deterministic). Feeds bias / β gradients without another pass over HBM.
template <int CO>
__device__ __forceinline__ void tile_colsum(const EngineArgs& a, const TileInfo& t, const float* s,
                                            int ld, float* dst) {
  const int gy0 = t.ty * 8, gx0 = t.tx * 8;
  const int rows = a.gh - gy0 < 8 ? a.gh - gy0 : 8, cols = a.gw - gx0 < 8 ? a.gw - gx0 : 8;
  for (int c = threadIdx.x; c < CO; c += 256) {
    float acc = 0.f;
    for (int my = 0; my < rows; ++my)
      for (int mx = 0; mx < cols; ++mx) acc += s[(my * 8 + mx) * ld + c];
    dst[(long)blockIdx.x * CO + c] = acc;
  }
}

// Load the B fragments of one 32-deep k-step: packed weights [.][CIq][CO][4], quad rows
// q0 .. q0+7, columns ncol0 + nt*16 + (lane & 15).
template <int NT, int CO>
__device__ __forceinline__ void load_bfrag(f4 (&bf)[2][NT], const float* __restrict__ wp, int q0,
                                           int ncol0, int lane) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    const int q = q0 + kk * 4 + (lane >> 4);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = ncol0 + nt * 16 + (lane & 15);
      bf[kk][nt] = *(const f4*)(wp + ((long)q * CO + n) * 4);
    }
  }
}

template <int MT, int NT>
__device__ __forceinline__ void mfma_block(f4 (&acc)[MT][NT], const f4 (&af)[MT], const f4 (&bf)[NT]) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma16(af[mt][e], bf[nt][e], acc[mt][nt]);
}

// Two-level accumulation of the exact-f32 contractions (common.h): a 32-deep
// k-block (two mfma_block calls) is summed from zero into `part`, then added to acc.
template <int MT, int NT>
__device__ __forceinline__ void zero_tile(f4 (&t)[MT][NT]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) t[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
}
template <int MT, int NT>
__device__ __forceinline__ void add_tile(f4 (&acc)[MT][NT], const f4 (&t)[MT][NT]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] += t[mt][nt];
}

// ----------------------------------------------------------------------------- GDN epilogue
// Channel contraction of an LDS tile: out[m][i] = Σ_j sX[m][j] · B[j][i], B packed
// [CO/4][CO][4] (packed[q][i][e] = B[4q+e][i]) and read straight from L2, one k-block ahead.
template <int CO, int MT, int NT, bool SQ = false>
__device__ __forceinline__ void chan_gemm(f4 (&acc)[MT][NT], const float* sX,
                                          const float* __restrict__ bp, int wm, int ncol0,
                                          int lane) {
  constexpr int XS = CO + 8;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
  f4 g[NT], gn[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    g[nt] = *(const f4*)(bp + ((long)(lane >> 4) * CO + ncol0 + nt * 16 + (lane & 15)) * 4);
  constexpr int KB = CO / 16;
#pragma unroll 2
  for (int kb = 0; kb < KB; ++kb) {
    if (kb + 1 < KB) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        gn[nt] = *(const f4*)(bp + ((long)((kb + 1) * 4 + (lane >> 4)) * CO + ncol0 + nt * 16 +
                                    (lane & 15)) * 4);
    }
    f4 af[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      af[mt] = *(const f4*)(sX + (wm * MT * 16 + mt * 16 + (lane & 15)) * XS + kb * 16 +
                            4 * (lane >> 4));
      if (SQ) af[mt] = af[mt] * af[mt];
    }
    mfma_block<MT, NT>(acc, af, g);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) g[nt] = gn[nt];
  }
}

// s_waitcnt vmcnt(N) (exp/lgkm counters untouched) + workgroup barrier; the empty asm statements
// keep the compiler from moving LDS accesses across it.
template <int N>
__device__ __forceinline__ void wait_vmcnt_barrier() {
  static_assert(N >= 0 && N < 64, "vmcnt field");
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// Zero source for glds lanes whose tap falls outside the image (padding). The library is built
// without relocatable device code, so every unit that includes this header carries its own copy
// (its host-side shadow has internal linkage). Not `static`: a static __device__ variable is
// externalised with default visibility and then addressed through the GOT, one more scalar load
// in every kernel that uses it.
__device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};

__device__ __forceinline__ void glds16(const float* src, float* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// The same contraction with γ streamed through LDS by LDS-DMA: 16-row k-blocks ([4][CO][4],
// contiguous in the packed layout), two stages at sG, one barrier per k-block. Entry: the
// caller's sX writes are complete in program order (the first loop barrier publishes them);
// exit: no barrier after the last k-block (callers add one before reusing sX or sG).
constexpr int GSTAGE_FLOATS(int CO) { return 2 * 16 * CO; }

template <int CO, int MT, int NT, bool SQ = false, int NW = 4>
__device__ __forceinline__ void chan_gemm_lds(f4 (&acc)[MT][NT], const float* sX,
                                              const float* __restrict__ bp, float* sG, int wm,
                                              int ncol0, int lane, int wave) {
  constexpr int XS = CO + 8;
  constexpr int GST = 16 * CO;          // floats per stage
  constexpr int NGI = GST * 4 / 1024;   // glds wave-instructions per stage
  constexpr int GI_W = (NGI + NW - 1) / NW;
  constexpr int KB = CO / 16;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
  auto issue = [&](int kb, int buf) {
    const float* src = bp + kb * GST + lane * 4;
#pragma unroll
    for (int j = 0; j < GI_W; ++j) {
      const int i = wave + NW * j;
      if (NGI % NW == 0 || i < NGI) glds16(src + i * 256, sG + buf * GST + i * 256);
    }
  };
  const int goff = ((lane >> 4) * CO + ncol0 + (lane & 15)) * 4;
  const float* xrow = sX + (wm * MT * 16 + (lane & 15)) * XS + 4 * (lane >> 4);
  issue(0, 0);
#pragma unroll 2
  for (int kb = 0; kb < KB; ++kb) {
    dma_barrier();
    if (kb + 1 < KB) issue(kb + 1, (kb + 1) & 1);
    const float* g = sG + (kb & 1) * GST + goff;
    f4 bf[NT], af[MT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bf[nt] = *(const f4*)(g + nt * 64);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      af[mt] = *(const f4*)(xrow + mt * 16 * XS + kb * 16);
      if (SQ) af[mt] = af[mt] * af[mt];
    }
    mfma_block<MT, NT>(acc, af, bf);
  }
}

// x6 channel contraction: acc[m][i] = Σ_j sX[m][j]·Γ[j][i], sX fp32 in LDS (split in VALU, one
// 8-channel fragment per (mt, 32-deep k-block)), Γ pre-split [3][CO/8][CO][8] bf16 — the
// B-fragment layout of v_mfma_f32_16x16x32_bf16 — read from L2 (221 KB at CO = 192; there is
// no LDS left beside the x² tile at two workgroups per CU), one k-block ahead. Entry: the sX
// writes of every wave are published (caller's barrier).
template <int CO, int MT, int NT, bool SQ = false>
__device__ __forceinline__ void chan_gemm_x6(f4 (&acc)[MT][NT], const float* sX,
                                             const unsigned short* __restrict__ g6, int wm,
                                             int ncol0, int lane) {
  constexpr int XS = CO + 8;
  constexpr int KB = CO / 32;
  constexpr long GP = (long)CO * CO;   // plane stride
  static_assert(KB % 2 == 0, "k-blocks in pairs (ping-pong B registers)");
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
  const float* xrow = sX + (wm * MT * 16 + (lane & 15)) * XS + 8 * (lane >> 4);
  const unsigned short* gb = g6 + ((lane >> 4) * CO + ncol0 + (lane & 15)) * 8;
  u4 b0[3][NT], b1[3][NT];
  auto load = [&](int kb, u4 (&b)[3][NT]) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        b[p][nt] = *(const u4*)(gb + p * GP + (long)kb * 4 * CO * 8 + nt * 128);
  };
  auto block = [&](int kb, const u4 (&b)[3][NT]) {
    X6Acc st;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u4 ah, am, al;
      f4 x0 = *(const f4*)(xrow + mt * 16 * XS + kb * 32);
      f4 x1 = *(const f4*)(xrow + mt * 16 * XS + kb * 32 + 4);
      if (SQ) {   // u² rounded to fp32 first, as the fp32 contraction (and conv2d(x², γ)) does
        x0 = x0 * x0;
        x1 = x1 * x1;
      }
      split8(x0, x1, ah, am, al);
      const bf8 Ah = __builtin_bit_cast(bf8, ah), Am = __builtin_bit_cast(bf8, am),
                Al = __builtin_bit_cast(bf8, al);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf8 Bh = __builtin_bit_cast(bf8, b[0][nt]), Bm = __builtin_bit_cast(bf8, b[1][nt]),
                  Bl = __builtin_bit_cast(bf8, b[2][nt]);
        mfma_x6<false>(acc, st, mt, nt, Ah, Am, Al, Bh, Bm, Bl);
      }
    }
    x6_flush<false>(acc, st);
  };
  load(0, b0);
  for (int kb = 0; kb < KB; kb += 2) {
    load(kb + 1, b1);
    block(kb, b0);
    if (kb + 2 < KB) load(kb + 2, b0);
    block(kb + 1, b1);
  }
}

// The same x6 contraction with the A operand already split in LDS: three bf16 planes
// [3][R][CO+8] (u16), written once by the producing waves, so no wave splits rows in VALU (with
// one wave row every wave used to split the whole x² tile for itself).
template <int CO, int MT, int NT, int R>
__device__ __forceinline__ void chan_gemm_x6p(f4 (&acc)[MT][NT], const unsigned short* sP,
                                              const unsigned short* __restrict__ g6, int wm,
                                              int ncol0, int lane) {
  constexpr int PS = CO + 8;
  constexpr int KB = CO / 32;
  constexpr long GP = (long)CO * CO;
  static_assert(KB % 2 == 0, "k-blocks in pairs (ping-pong B registers)");
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
  const unsigned short* arow = sP + (wm * MT * 16 + (lane & 15)) * PS + 8 * (lane >> 4);
  const unsigned short* gb = g6 + ((lane >> 4) * CO + ncol0 + (lane & 15)) * 8;
  u4 b0[3][NT], b1[3][NT];
  auto load = [&](int kb, u4 (&b)[3][NT]) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        b[p][nt] = *(const u4*)(gb + p * GP + (long)kb * 4 * CO * 8 + nt * 128);
  };
  auto block = [&](int kb, const u4 (&b)[3][NT]) {
    X6Acc st;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const unsigned short* a = arow + mt * 16 * PS + kb * 32;
      const bf8 Ah = __builtin_bit_cast(bf8, *(const u4*)(a));
      const bf8 Am = __builtin_bit_cast(bf8, *(const u4*)(a + R * PS));
      const bf8 Al = __builtin_bit_cast(bf8, *(const u4*)(a + 2 * R * PS));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const bf8 Bh = __builtin_bit_cast(bf8, b[0][nt]), Bm = __builtin_bit_cast(bf8, b[1][nt]),
                  Bl = __builtin_bit_cast(bf8, b[2][nt]);
        mfma_x6<false>(acc, st, mt, nt, Ah, Am, Al, Bh, Bm, Bl);
      }
    }
    x6_flush<false>(acc, st);
  };
  load(0, b0);
  for (int kb = 0; kb < KB; kb += 2) {
    load(kb + 1, b1);
    block(kb, b0);
    if (kb + 2 < KB) load(kb + 2, b0);
    block(kb + 1, b1);
  }
}

// LDS floats the GDN core needs for an R-row tile (fp32 x² tile + γ stages, or, for the x6
// contraction, the three split planes of x²).
constexpr int gdn_lds_floats(int R, int CO, bool G6) {
  return G6 ? (3 * R * (CO + 8) + 1) / 2 : R * (CO + 8) + GSTAGE_FLOATS(CO);
}

// x (bias already added) in accumulator layout → GDN(x) (or IGDN) left in LDS sX[BM][CO+4].
// models/GDN.py:83-90: n = conv2d(x², γ, β) = β + Σ_j γ[i][j]·x_j²;  y = x / √n | x·√n.
// The caller guarantees smem is free on entry; on return every wave has passed a barrier after
// the last sX write.
template <int CO, int MT, int NT, bool INVERSE, int R = BM, int T = 256, bool G6 = false>
__device__ __forceinline__ void gdn_core(const f4 (&x)[MT][NT], float* sX,
                                         const float* __restrict__ gbeta,
                                         const float* __restrict__ gp, int wm, int ncol0,
                                         int lane, const unsigned short* g6 = nullptr) {
  constexpr int XS = CO + 8;
  f4 nacc[MT][NT];
  if constexpr (G6) {
    // x² (rounded to fp32, as conv2d(x², γ) sees it) split once into three bf16 planes
    unsigned short* sP = (unsigned short*)sX;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
          const int col = ncol0 + nt * 16 + (lane & 15);
          const float v = x[mt][nt][r] * x[mt][nt][r];
          const unsigned h = __float_as_uint(v) & 0xffff0000u;
          const float rr = v - __uint_as_float(h);
          const unsigned m = __float_as_uint(rr) & 0xffff0000u;
          const unsigned l = __float_as_uint(rr - __uint_as_float(m));
          sP[row * XS + col] = (unsigned short)(h >> 16);
          sP[(R + row) * XS + col] = (unsigned short)(m >> 16);
          sP[(2 * R + row) * XS + col] = (unsigned short)(l >> 16);
        }
    __syncthreads();   // planes of every wave published
    chan_gemm_x6p<CO, MT, NT, R>(nacc, sP, g6, wm, ncol0, lane);
  } else {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
        const int col = ncol0 + nt * 16 + (lane & 15);
        const float v = x[mt][nt][r];
        sX[row * XS + col] = v * v;
      }
    chan_gemm_lds<CO, MT, NT, false, T / 64>(nacc, sX, gp, sX + R * XS, wm, ncol0, lane,
                                             __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
  }
  __syncthreads();  // all reads of x² done
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
        const int col = ncol0 + nt * 16 + (lane & 15);
        const float n = nacc[mt][nt][r] + gbeta[col];
        const float s = sqrtf(n);
        sX[row * XS + col] = INVERSE ? x[mt][nt][r] * s : x[mt][nt][r] / s;
      }
  __syncthreads();
}

// Accumulator-layout values → LDS tile [BM][ld] (caller synchronises).
template <int MT, int NT>
__device__ __forceinline__ void acc_to_lds(const f4 (&v)[MT][NT], float* s, int ld, int wm,
                                           int col0, int lane) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
        s[row * ld + col0 + nt * 16 + (lane & 15)] = v[mt][nt][r];
      }
}

template <int CO, int MT, int NT, bool INVERSE, int R = BM, int T = 256, bool G6 = false>
__device__ __forceinline__ void gdn_epilogue(f4 (&x)[MT][NT], float* smem, const EngineArgs& a,
                                             const TileInfo& t, int wm, int ncol0, int lane) {
  constexpr int XS = CO + 8;
  gdn_core<CO, MT, NT, INVERSE, R, T, G6>(x, smem, a.gbeta, a.ggamma, wm, ncol0, lane,
                                          a.ggamma6);
  if (a.out != nullptr) store_tile_rows<CO, R, T>(a, t, smem, XS, a.out, CO, 0);
  if (a.out_split != nullptr) store_tile_rows_split<CO, R, T>(a, t, smem, XS, CO, 0);
  if (a.pre != nullptr) {
    __syncthreads();
    acc_to_lds<MT, NT>(x, smem, XS, wm, ncol0, lane);
    __syncthreads();
    store_tile_rows<CO, R, T>(a, t, smem, XS, a.pre, CO, 0);
  }
}

// ------------------------------------------------------------------ GDN / IGDN backward epilogue
// g = ∂L/∂(GDN output) in accumulator layout (the dgrad GEMM of the NEXT layer); u = the saved
// GDN input (pre-activation). Mirrors the autograd of models/GDN.py:83-90 op for op:
//   n = β + γ·u², s = √n
//   GDN : ∂u = g/s + 2u·(γᵀ dn),  dn = ((−g·u)/(s·s)) / (2s)      (div, sqrt backward)
//   IGDN: ∂u = g·s + 2u·(γᵀ dn),  dn = (g·u) / (2s)               (mul, sqrt backward)
// Stores ∂u (a.out) and dn (a.tout; dγ = Σ_p dn ⊗ u², dβ = Σ_p dn are reduced later).
template <int CO, int MT, int NT, bool INVERSE>
__device__ __forceinline__ void gdn_bwd_epilogue(f4 (&g)[MT][NT], float* smem, const EngineArgs& a,
                                                 const TileInfo& t, int wm, int ncol0, int lane) {
  constexpr int XS = CO + 8;
  float* sX = smem;
  float* sG = smem + BM * XS;
  const int wave = threadIdx.x >> 6;
  load_tile_rows<CO>(a, t, a.saved, sX, XS, CO, 0);   // u, kept in LDS through GEMM 1
  f4 acc2[MT][NT];
  if (a.ggamma6 != nullptr) {   // x6: γ and γᵀ pre-split, from L2 (no LDS stages)
    __syncthreads();            // u tile published
    chan_gemm_x6<CO, MT, NT, true>(acc2, sX, a.ggamma6, wm, ncol0, lane);
  } else {
    chan_gemm_lds<CO, MT, NT, true>(acc2, sX, a.ggamma, sG, wm, ncol0, lane, wave);  // Σ_j γ[i][j] u_j²
  }
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = ncol0 + nt * 16 + (lane & 15);
        const int idx = (wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r) * XS + col;
        const float uu = sX[idx];  // read, then rewritten by the same lane: no barrier needed
        const float n = acc2[mt][nt][r] + a.gbeta[col];
        const float sq = sqrtf(n);
        const float gg = g[mt][nt][r];
        float dn;
        if (INVERSE) {
          g[mt][nt][r] = gg * sq;
          dn = (gg * uu) / (2.0f * sq);
        } else {
          g[mt][nt][r] = gg / sq;
          dn = ((-gg * uu) / (sq * sq)) / (2.0f * sq);
        }
        sX[idx] = dn;
      }
  if (a.ggammaT6 != nullptr) {
    __syncthreads();            // dn tile published
    chan_gemm_x6<CO, MT, NT>(acc2, sX, a.ggammaT6, wm, ncol0, lane);
  } else {
    chan_gemm_lds<CO, MT, NT>(acc2, sX, a.ggammaT, sG, wm, ncol0, lane, wave);  // w_j = Σ_i γ[i][j] dn_i
  }
  store_tile_rows<CO>(a, t, sX, XS, a.tout, CO, 0);
  if (a.colsum_t != nullptr) tile_colsum<CO>(a, t, sX, XS, a.colsum_t);
  __syncthreads();
  // u again, from HBM/L2 rather than held in 48 VGPRs through both contractions (that kept
  // the kernel at one wave per SIMD)
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
      const long p = out_pixel(a, t, row);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int col = ncol0 + nt * 16 + (lane & 15);
        const float uu = p < 0 ? 0.f : a.saved[p * CO + col];
        sX[row * XS + col] = g[mt][nt][r] + acc2[mt][nt][r] * (2.0f * uu);
      }
    }
  __syncthreads();
  // the fp32 ∂u is optional beside its split form (the x6 backward hands only the split on)
  if (a.out != nullptr) store_tile_rows<CO>(a, t, sX, XS, a.out, CO, 0);
  if (a.out_split != nullptr) store_tile_rows_split<CO>(a, t, sX, XS, CO, 0);   // x6 consumer
  if (a.colsum_out != nullptr) tile_colsum<CO>(a, t, sX, XS, a.colsum_out);
}

// ------------------------------------------------------------------------- rate backward epilogue
// ∂L/∂ỹ = (decoder dgrad in acc) + ∂L/∂bpp / (B·H·W) · ∂bits/∂ỹ, and the per-channel parameter
// gradients of the factorised model, as the autograd of model.py:71-78 / bitEstimator.py:20-25
// evaluates them (per element; summed per tile here, over tiles later).
// (per element: rate_bwd_element, common.h)
template <int CO, int BN, int MT, int NT>
__device__ __forceinline__ void rate_bwd_epilogue(f4 (&acc)[MT][NT], float* smem, const EngineArgs& a,
                                                  const TileInfo& t, int wm, int ncol0, int lane) {
  constexpr int OS = BN + 4;
  float* sO = smem;
  const int cbase = t.nb * BN;
  const bool rate = a.gscale != nullptr;
  if (rate) load_tile_rows<BN>(a, t, a.saved, sO, OS, CO, cbase);
  __syncthreads();
  const float gsc = rate ? a.gscale[0] / a.count : 0.0f;
  float pg[NT][11];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int k = 0; k < 11; ++k) pg[nt][k] = 0.0f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
        const int lcol = ncol0 - cbase + nt * 16 + (lane & 15);
        float v = acc[mt][nt][r];
        if (rate && out_pixel(a, t, row) >= 0)
          v += rate_bwd_element(sO[row * OS + lcol], a.rate, CO, cbase + lcol, gsc, pg[nt]);
        sO[row * OS + lcol] = v;
      }
  __syncthreads();
  store_tile_rows<BN>(a, t, sO, OS, a.out, CO, cbase);
  if (a.out_split != nullptr) store_tile_rows_split<BN>(a, t, sO, OS, CO, cbase);
  if (rate) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        float v = pg[nt][k];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        // row = the tile's linear index
        const long row = ((long)t.b * a.tiles_y + t.ty) * a.tiles_x + t.tx;
        if (lane < 16) a.rpart[(row * 11 + k) * CO + ncol0 + nt * 16 + lane] = v;
      }
  }
}

// ------------------------------------------------------------------- quantiser + rate epilogue
// model.py:48-56 (ŷ = round(y) | y + noise) and model.py:71-73 (bits per element), summed per
// tile; y and ŷ stored NHWC.
template <int CO, int BN, int MT, int NT, int WN>
__device__ __forceinline__ void quant_epilogue(f4 (&acc)[MT][NT], float* smem, const EngineArgs& a,
                                               const TileInfo& t, int wm, int ncol0, int lane,
                                               int wave) {
  constexpr int OS = BN + 4;
  float* sO = smem;
  float bits = 0.f;
  const int cbase = t.nb * BN;
  // Integer latents: the per-channel table of the same element_bits, read for every element
  // (index clamped, loads all in flight); the others (noise mode, |ŷ| > 32, no table) are
  // evaluated in one block after them — a per-element `table ? lookup : element_bits` branch
  // skipped 2 KB of inlined element_bits per element, an instruction-cache miss each time.
  // The bits are added in the same element order either way.
  float yv[MT][NT][4], bv[MT][NT][4];
  bool slow = false;
  const bool table = a.rtab != nullptr && a.qmode == ICLR17_QUANT_ROUND;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
        const int lcol = ncol0 - cbase + nt * 16 + (lane & 15);
        const int col = cbase + lcol;
        const int gy = t.ty * 8 + (row >> 3), gx = t.tx * 8 + (row & 7);
        const bool ok = gy < a.gh && gx < a.gw;
        const float y = acc[mt][nt][r];
        float yh;
        if (a.qmode == ICLR17_QUANT_ROUND) {
          yh = rintf(y);
        } else {
          const float u = ok ? a.noise[(((long)t.b * CO + col) * a.Hout + gy) * a.Wout + gx] : 0.f;
          yh = y + u;
        }
        yv[mt][nt][r] = yh;
        bv[mt][nt][r] = table ? a.rtab[col * 65 + (int)fminf(fmaxf(yh, -32.f), 32.f) + 32] : 0.f;
        slow |= ok && !(table && fabsf(yh) <= 32.f);
        sO[row * OS + lcol] = yh;
      }
  if (slow) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float yh = yv[mt][nt][r];
          if (!(table && fabsf(yh) <= 32.f))
            bv[mt][nt][r] = element_bits(yh, a.rate, CO, ncol0 + nt * 16 + (lane & 15));
        }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
        const int gy = t.ty * 8 + (row >> 3), gx = t.tx * 8 + (row & 7);
        if (gy < a.gh && gx < a.gw) bits += bv[mt][nt][r];
      }
  __syncthreads();
  store_tile_rows<BN>(a, t, sO, OS, a.yhat, CO, cbase);
  if (a.out_split != nullptr) store_tile_rows_split<BN>(a, t, sO, OS, CO, cbase);   // ŷ, x6 form
  if (a.out != nullptr) {
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
          const int lcol = ncol0 - cbase + nt * 16 + (lane & 15);
          sO[row * OS + lcol] = acc[mt][nt][r];
        }
    __syncthreads();
    store_tile_rows<BN>(a, t, sO, OS, a.out, CO, cbase);
  }
  // deterministic tile sum: lanes → wave (xor tree) → waves in order
  bits = wave_sum(bits);
  __syncthreads();
  if (lane == 0) sO[wave] = bits;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < 4; ++w) s += (double)sO[w];
    const int tile = (t.ty * a.tiles_x + t.tx) * gridDim.y + t.nb;
    a.partial[(long)t.b * a.partials_per_image + tile] = s;
  }
}

// --------------------------------------------------------------- deconv3 (all-phase) epilogue
// Column n = co*16 + ry*4 + rx; row m = base pixel q (8×8 block). Output pixel
// (4·qy + ry, 4·qx + rx) of channel co. synthesis_17.py:23 + model.py:59 clamp(0, 1).
template <int MT, int NT>
__device__ __forceinline__ void out3_epilogue(f4 (&acc)[MT][NT], float* smem, const EngineArgs& a,
                                              const TileInfo& t, int wm, int lane, int wave) {
  constexpr int SS = 33;  // padded row of the 32×32 output block
  float* sO = smem;       // [3][32][33]
  const int H = a.Hout, W = a.Wout;  // image dims
  float vals[MT][NT][4];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) vals[mt][nt][r] = acc[mt][nt][r] + a.bias[nt];
  float sse = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && a.recon == nullptr) break;
    float* dst = pass == 0 ? a.out : a.recon;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
          const int ph = lane & 15;
          const int oyl = (m >> 3) * 4 + (ph >> 2), oxl = (m & 7) * 4 + (ph & 3);
          float v = vals[mt][nt][r];
          if (pass == 0) v = fminf(fmaxf(v, 0.0f), 1.0f);
          sO[(nt * 32 + oyl) * SS + oxl] = v;
        }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 3 * 32 * 8; idx += 256) {
      const int c4 = idx & 7, row = (idx >> 3) & 31, co = idx >> 8;
      const int oy = t.ty * 32 + row, ox = t.tx * 32 + c4 * 4;
      if (oy >= H || ox >= W) continue;
      const float* s = sO + (co * 32 + row) * SS + c4 * 4;
      const f4 v = f4{s[0], s[1], s[2], s[3]};
      const long off = (((long)t.b * 3 + co) * H + oy) * W + ox;
      *(f4*)(dst + off) = v;
      if (pass == (a.sse_unclipped ? 1 : 0) && a.xref != nullptr) {
        const f4 xr = *(const f4*)(a.xref + off);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[e] - xr[e];
          sse += d * d;
        }
      }
    }
    __syncthreads();
  }
  if (a.xref != nullptr) {
    sse = wave_sum(sse);
    if (lane == 0) sO[wave] = sse;
    __syncthreads();
    if (threadIdx.x == 0) {
      double s = 0.0;
      for (int w = 0; w < 4; ++w) s += (double)sO[w];
      a.partial[(long)t.b * a.partials_per_image + t.ty * a.tiles_x + t.tx] = s;
    }
  }
}

// ------------------------------------------------------------------------- the engine kernel
// Main loop: both operands reach LDS by LDS-DMA (global_load_lds_dwordx4), so no staging VGPRs
// and no ds_write pass. A step is 32 input channels of one tap:
//   A image [BM][32] floats, 128-byte rows, 16-byte chunk c stored at c ^ (row & 7) — the swizzle
//     lives in the per-lane SOURCE address (glds writes lane-linear), and makes the fragment
//     reads (16 rows × one chunk per lane group) bank-conflict free;
//   B image [8 quads][BN][4] floats: the packed weights of the step, copied linearly.
// Two LDS stages, one barrier per step: the DMA of step s+1 is in flight while step s computes.
//
// X6 (the bf16x6 mode): the A operand arrives as three bf16 planes (hi, mid, lo — the exact split
// written by the producing layer's epilogue), A image [3][BM][32] bf16 with 64-byte rows whose
// 16-byte piece g sits at g ^ ((row >> 1) & 3); B stays fp32 in LDS and each wave splits its own
// columns in VALU. One 32-deep step = per 16×16 tile six v_mfma_f32_16x16x32_bf16:
// lo·hi + hi·lo + mid·mid + mid·hi + hi·mid + hi·hi (the dropped mid·lo, lo·mid, lo·lo terms are
// below 2^-24 of the product), accumulated in fp32.
// W6 (x6 conv3): B arrives pre-split, [3 planes][4 k-groups][BN][8] bf16 per stage (a.w6), and
// the fragments are read as they are: conv3's 2×2 waves split each weight column for only two
// row tiles, so the per-step split was 3.7 VALU instructions per MFMA. Same bf16 operands (the
// split is iclr17_split_packed's, i.e. the same split8 on the same quads): bit-identical output.
// (The h3 form's convolutions run on the h3 engine, csrc/engine_h3.hip.)
template <int CI, int CO, int BN, int WM, int WN, int EPI, bool X6, int BMT = BM, bool W6 = false>
__device__ __forceinline__ void engine_body(const EngineArgs& a) {
  constexpr bool XS = X6;                        // 16-bit split-form A planes
  constexpr int APL = 3;                         // A / pre-split B planes
  constexpr int NWV = WM * WN;                   // waves (4, or 8 for the 128-row tiles)
  constexpr int MT = BMT / WM / 16;
  constexpr int NT = BN / WN / 16;
  constexpr int KCH = 32;                        // input channels per k-step
  constexpr int NCH = CI / KCH;
  static_assert(!W6 || (X6 && EPI == EPI_QUANT), "pre-split weights: x6 conv3");
  constexpr int SA = XS ? APL * BMT * KCH / 2 : BMT * KCH;   // A image floats per stage
  constexpr int SB = W6 ? APL * 4 * BN * 8 / 2   // W6: [3][4][BN][8] bf16
                        : KCH * BN;              // B image floats per stage: [8 quads][BN][4]
  constexpr int STAGE = SA + SB;
  constexpr int NAI = SA * 4 / 1024;             // A glds wave-instructions per step (8 | 12)
  constexpr int NBI = SB * 4 / 1024;             // B glds wave-instructions per step
  constexpr int AI_W = NAI / NWV;                // per wave
  constexpr int BI_W = (NBI + NWV - 1) / NWV;
  constexpr int API = BMT / 16;                  // x6: A wave-instructions per plane (16 rows each)
  // DMA ring depth: conv3 (+ quantiser) has a third of conv2's MFMAs per step, too few to hide
  // an L2-miss DMA issued one step ahead, so it runs NS stages with a counted vmcnt wait.
  // x6 IGDN layers (deconv1 / deconv2): halo-patch A operand (see the main loop)
  constexpr bool HALO = X6 && EPI == EPI_IGDN && BMT == BM;
  // per-tap two-level accumulation for the encoder layers whose latents are rounded (conv2+GDN2,
  // conv3+quantiser): their accuracy decides the ŷ flips against the reference
  constexpr bool TAPSEP = kSepAcc && !HALO && (EPI == EPI_GDN || EPI == EPI_QUANT);
  constexpr int HALO_NI = (3 * 100 * 64 + 1023) / 1024;   // patch DMA wave-instructions (19)
  constexpr int HALO_PF = HALO_NI * 256;                  // patch floats
  constexpr int LDS_A = HALO ? HALO_PF + 2 * SB
                             : 2 * STAGE;   // two-stage ring (3, 4 stages measured slower: DESIGN.md §5)
  constexpr int LDS_XF = BMT * (CO + 8) + GSTAGE_FLOATS(CO);
  constexpr int LDS_XP = gdn_lds_floats(BMT, CO, XS);
  constexpr int LDS_X = (EPI == EPI_GDN || EPI == EPI_IGDN) ? (LDS_XF > LDS_XP ? LDS_XF : LDS_XP)
                        : (EPI == EPI_GDN_BWD || EPI == EPI_IGDN_BWD) ? LDS_XF : 0;
  constexpr int LDS_O = BMT * (BN + 4) + 8;
  constexpr int LDS_3 = 3 * 32 * 33 + 8;
  constexpr int L1 = LDS_A > LDS_X ? LDS_A : LDS_X;
  constexpr int L2 = LDS_O > LDS_3 ? LDS_O : LDS_3;
  constexpr int LDS_FLOATS = L1 > L2 ? L1 : L2;
  static_assert(MT * WM * 16 == BMT && NT * WN * 16 == BN, "tile shape");
  static_assert(BMT == BM || (X6 && (EPI == EPI_GDN || EPI == EPI_IGDN) && NWV == 8),
                "128-row tiles: the x6 GDN / IGDN layers on 8 waves");
  static_assert(NWV == 4 || NWV == 8, "4 or 8 waves");
  static_assert(CI % KCH == 0 && NAI % NWV == 0, "k-step split");
  static_assert(BN == CO || BN % 16 == 0, "B image: quad rows of BN columns");
  static_assert((SB * 4) % 1024 == 0, "B image in whole wave-instructions");
  __shared__ __attribute__((aligned(16))) float smem[LDS_FLOATS];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform (scalar branches)
  const int wm = wave / WN, wn = wave % WN;
  TileInfo t = decode_tile<BMT / 8>(a);
  const int ph = t.py * a.tt.npx + t.px;
  const int ncol0 = t.nb * BN + wn * (BN / WN);

  // A DMA. fp32: wave-instruction i covers rows 8i .. 8i+7; lane → (row, physical chunk
  // lane & 7), fetching logical chunk (lane & 7) ^ (row & 7). X6: instruction i covers plane
  // i >> 2, rows 16(i & 3) .. +15; lane → (row, physical piece lane & 3), fetching logical piece
  // (lane & 3) ^ ((row >> 1) & 3) (8 bf16 channels).
  int iy0[AI_W], ix0[AI_W], pbase[AI_W];
  bool rval[AI_W];
#pragma unroll
  for (int j = 0; j < AI_W; ++j) {
    const int i = wave * AI_W + j;
    const int row = XS ? 16 * (i % API) + (lane >> 2) : i * 8 + (lane >> 3);
    const int c = XS ? (lane & 3) ^ ((row >> 1) & 3) : (lane & 7) ^ (row & 7);
    const int gy = t.ty * (BMT / 8) + (row >> 3), gx = t.tx * 8 + (row & 7);
    rval[j] = gy < a.gh && gx < a.gw;
    iy0[j] = gy * a.sin;
    ix0[j] = gx * a.sin;
    pbase[j] = (iy0[j] * a.Win + ix0[j]) * CI + c * (XS ? 8 : 4);
  }
  const long img = (long)t.b * a.Hin * a.Win * CI;
  const float* __restrict__ inb = a.in + img;
  const unsigned short* __restrict__ inb6 = a.in_split + img;
  // B DMA: wave-instruction i copies 1 KB; source offset (floats) within the step's slice
  int bsrc[BI_W];
#pragma unroll
  for (int j = 0; j < BI_W; ++j) {
    const int i = wave + NWV * j;
    if constexpr (W6) {   // u16 offset in the pre-split planes: (plane, k-group, column) of the slot
      const int o2 = i * 512 + lane * 8;   // u16 offset in the LDS image [3][4][BN][8]
      const int pl = o2 / (32 * BN), r = o2 - pl * 32 * BN;
      const int gg = r / (BN * 8), col = (r - gg * BN * 8) / 8;
      bsrc[j] = (int)(pl * a.w6_plane) + (gg * CO + t.nb * BN + col) * 8;
    } else {
      const int o = i * 256 + lane * 4;   // offset in the LDS image [8 quads][BN][4]
      bsrc[j] = (BN == CO) ? o : ((o / (BN * 4)) * CO + t.nb * BN) * 4 + o % (BN * 4);
    }
  }

  int t0 = 0, ntaps = 1;
  // Step order: tap-major (the 6 channel chunks of a tap in a row). Chunk-major order keeps a
  // workgroup's input footprint to one chunk and cuts the HBM refetch 3-5x, but measured 3-6 %
  // slower on the same box: these layers are bound by MFMA issue, and the
  // Infinity Cache absorbs the L2 misses.
  auto issue = [&](int s, int buf) {
    const int tap = t0 + s / NCH, cc = s - (s / NCH) * NCH;
    const int td = a.tt.dydx[tap];
    const int dy = (td & 0xff) - 128, dx = ((td >> 8) & 0xff) - 128;
    const int so = (dy * a.Win + dx) * CI + cc * KCH;
    float* sa = smem + buf * STAGE;
#pragma unroll
    for (int j = 0; j < AI_W; ++j) {
      const bool ok = rval[j] && (unsigned)(iy0[j] + dy) < (unsigned)a.Hin &&
                      (unsigned)(ix0[j] + dx) < (unsigned)a.Win;
      const int i = wave * AI_W + j;
      if constexpr (XS) {
        const unsigned short* src = inb6 + (i / API) * a.in_plane + pbase[j] + so;
        glds16(ok ? (const float*)src : g_zero16, sa + i * 256);
      } else {
        glds16(ok ? inb + pbase[j] + so : g_zero16, sa + i * 256);
      }
    }
    float* sb = sa + SA;
    if constexpr (W6) {
      const unsigned short* __restrict__ ws6 = a.w6 + ((long)tap * (CI / 8) + cc * 4) * CO * 8;
#pragma unroll
      for (int j = 0; j < BI_W; ++j) {
        const int i = wave + NWV * j;
        if (NBI % NWV == 0 || i < NBI) glds16((const float*)(ws6 + bsrc[j]), sb + i * 256);
      }
    } else {
      const float* __restrict__ ws = a.w + ((long)tap * CI + cc * KCH) * CO;   // uniform base
#pragma unroll
      for (int j = 0; j < BI_W; ++j) {
        const int i = wave + NWV * j;
        if (NBI % NWV == 0 || i < NBI) glds16(ws + bsrc[j], sb + i * 256);
      }
    }
  };

  f4 acc[MT][NT];
  // fragment read offsets (floats) within a stage
  int aoff[2][MT];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int row = wm * MT * 16 + mt * 16 + (lane & 15);
      aoff[kk][mt] = row * KCH + (((kk * 4 + (lane >> 4)) ^ (row & 7)) * 4);
    }
  const int boff0 = ((lane >> 4) * BN + wn * (BN / WN) + (lane & 15)) * 4;

  // X6 fragment offsets: A piece (bf16 elements) per mt; B quads 2g, 2g+1 (floats)
  int aoff6[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int row = wm * MT * 16 + mt * 16 + (lane & 15);
    aoff6[mt] = (row * 4 + ((lane >> 4) ^ ((row >> 1) & 3))) * 8;
  }
  const int boff6 = (2 * (lane >> 4) * BN + wn * (BN / WN) + (lane & 15)) * 4;

  auto compute6 = [&](int buf) {
    X6Acc st;
    const unsigned short* sa = (const unsigned short*)(smem + buf * STAGE);
    const float* sb = smem + buf * STAGE + SA + boff6;
    bf8 Bh[NT], Bm[NT], Bl[NT];
    if constexpr (W6) {   // [3][4][BN][8]: lane (k-group lane >> 4, column) reads 16 bytes per plane
      const unsigned short* sb6 = (const unsigned short*)(smem + buf * STAGE + SA) +
                                  ((lane >> 4) * BN + wn * (BN / WN) + (lane & 15)) * 8;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        Bh[nt] = __builtin_bit_cast(bf8, *(const u4*)(sb6 + nt * 128));
        Bm[nt] = __builtin_bit_cast(bf8, *(const u4*)(sb6 + 32 * BN + nt * 128));
        Bl[nt] = __builtin_bit_cast(bf8, *(const u4*)(sb6 + 64 * BN + nt * 128));
      }
    } else {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      u4 bh, bm, bl;
      split8(*(const f4*)(sb + nt * 64), *(const f4*)(sb + BN * 4 + nt * 64), bh, bm, bl);
      Bh[nt] = __builtin_bit_cast(bf8, bh);
      Bm[nt] = __builtin_bit_cast(bf8, bm);
      Bl[nt] = __builtin_bit_cast(bf8, bl);
    }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const bf8 Ah = __builtin_bit_cast(bf8, *(const u4*)(sa + aoff6[mt]));
      const bf8 Am = __builtin_bit_cast(bf8, *(const u4*)(sa + BMT * KCH + aoff6[mt]));
      const bf8 Al = __builtin_bit_cast(bf8, *(const u4*)(sa + 2 * BMT * KCH + aoff6[mt]));
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        mfma_x6<false>(acc, st, mt, nt, Ah, Am, Al, Bh[nt], Bm[nt], Bl[nt]);
      }
    }
    x6_flush<false>(acc, st);
  };

  auto compute = [&](int buf) {
    if constexpr (X6) {
      compute6(buf);
      return;
    }
    const float* sa = smem + buf * STAGE;
    const float* sb = sa + SA + boff0;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f4 af[MT], bf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bf[nt] = *(const f4*)(sb + kk * 16 * BN + nt * 64);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) af[mt] = *(const f4*)(sa + aoff[kk][mt]);
      mfma_block<MT, NT>(acc, af, bf);
    }
  };

  t0 = a.tt.begin[ph];
  ntaps = a.tt.begin[ph + 1] - t0;
  const int nsteps = ntaps * NCH;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};

  if constexpr (HALO) {
    // x6 deconv (IGDN layers, input stride 1, taps dy, dx ∈ {−1, 0, 1}): chunk-major steps. The
    // 10×10 input patch of the 8×8 base tile (three bf16 planes, 64 bytes per pixel, 19 KB) is
    // staged ONCE per 32-channel chunk and every tap reads its shifted window from it, instead
    // of each (tap, chunk) step DMA-ing its own 64 rows again (100 vs 64·taps staged pixels).
    // The patch is single-buffered (the chunk boundary is a barrier-bounded refill that the
    // co-resident workgroup covers); the weight stages stay double-buffered. 16-byte piece g of
    // patch pixel q sits at g ^ 2·((q / 10) & 1): conflict-free ds_read_b128 lane groups for every
    // tap offset (checked exhaustively).
    unsigned short* const sp = (unsigned short*)smem;
    float* const sbw = smem + HALO_PF;
    const int gy0 = t.ty * 8 - 1, gx0 = t.tx * 8 - 1;   // patch origin (input coordinates)
    auto issue_patch = [&](int cc) {
#pragma unroll
      for (int j = 0; j < (HALO_NI + 3) / 4; ++j) {
        const int i = wave + 4 * j;
        if (i >= HALO_NI) break;   // wave-uniform
        const int qq = 16 * i + (lane >> 2);            // plane · 100 + patch pixel
        const int pl = qq / 100, q = qq - pl * 100;
        const int iy = gy0 + q / 10, ix = gx0 + q % 10;
        const bool ok = pl < 3 && (unsigned)iy < (unsigned)a.Hin && (unsigned)ix < (unsigned)a.Win;
        const int g = (lane & 3) ^ (2 * ((q / 10) & 1));
        const unsigned short* src =
            inb6 + (long)(pl < 3 ? pl : 0) * a.in_plane + ((long)iy * a.Win + ix) * CI + cc * KCH + g * 8;
        glds16(ok ? (const float*)src : g_zero16, (float*)sp + i * 256);
      }
    };
    auto issue_b = [&](int s, int buf) {   // weights of step s = (chunk, tap) into stage buf
      const int cc = s / ntaps, tap = t0 + (s - cc * ntaps);
      float* sb = sbw + buf * SB;
      const float* __restrict__ ws = a.w + ((long)tap * CI + cc * KCH) * CO;
#pragma unroll
      for (int j = 0; j < BI_W; ++j) {
        const int i = wave + NWV * j;
        if (NBI % NWV == 0 || i < NBI) glds16(ws + bsrc[j], sb + i * 256);
      }
    };
    // tile pixel of fragment row mt: (ty, tx) = (r >> 3, r & 7); patch pixel at tap (0, 0)
    int hq[MT], hy[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int r = wm * MT * 16 + mt * 16 + (lane & 15);
      hy[mt] = (r >> 3) + 1;
      hq[mt] = hy[mt] * 10 + (r & 7) + 1;
    }
    auto compute_halo = [&](int buf, int dy, int dx) {
      X6Acc st;
      const float* sb = sbw + buf * SB + boff6;
      bf8 Bh[NT], Bm[NT], Bl[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        u4 bh, bm, bl;
        split8(*(const f4*)(sb + nt * 64), *(const f4*)(sb + BN * 4 + nt * 64), bh, bm, bl);
        Bh[nt] = __builtin_bit_cast(bf8, bh);
        Bm[nt] = __builtin_bit_cast(bf8, bm);
        Bl[nt] = __builtin_bit_cast(bf8, bl);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int q = hq[mt] + dy * 10 + dx;
        const int g = (lane >> 4) ^ (2 * ((hy[mt] + dy) & 1));
        const unsigned short* pa = sp + q * 32 + g * 8;
        const bf8 Ah = __builtin_bit_cast(bf8, *(const u4*)(pa));
        const bf8 Am = __builtin_bit_cast(bf8, *(const u4*)(pa + 100 * 32));
        const bf8 Al = __builtin_bit_cast(bf8, *(const u4*)(pa + 200 * 32));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          mfma_x6<false>(acc, st, mt, nt, Ah, Am, Al, Bh[nt], Bm[nt], Bl[nt]);
        }
      }
      x6_flush<false>(acc, st);
    };
    issue_patch(0);
    issue_b(0, 0);
    for (int cc = 0; cc < NCH; ++cc) {
      for (int k = 0; k < ntaps; ++k) {
        const int s = cc * ntaps + k;
        dma_barrier();   // weights of step s landed (and, at k = 0, chunk cc's patch)
        if (k + 1 < ntaps) issue_b(s + 1, (s + 1) & 1);
        const int td = a.tt.dydx[t0 + k];
        compute_halo(s & 1, (td & 0xff) - 128, ((td >> 8) & 0xff) - 128);
        if (k + 1 == ntaps && cc + 1 < NCH) {
          __syncthreads();   // every wave is done with this chunk's patch
          issue_patch(cc + 1);
          issue_b(s + 1, (s + 1) & 1);
        }
      }
    }
  } else {
    issue(0, 0);
    if constexpr (TAPSEP) {
      // two-level accumulation (common.h): each tap's NCH steps accumulate in
      // place from zero, and the tap sum is added to `total` with one correctly rounded add
      static_assert(NCH % 2 == 0, "stage parity = chunk parity");
      f4 total[MT][NT];
      zero_tile<MT, NT>(total);
      for (int tp = 0; tp < ntaps; ++tp) {
        zero_tile<MT, NT>(acc);
#pragma unroll
        for (int cc = 0; cc < NCH; ++cc) {
          const int s = tp * NCH + cc;
          dma_barrier();   // step s landed for every wave; stage (s+1)&1 is free
          if (s + 1 < nsteps) issue(s + 1, (cc + 1) & 1);
          compute(cc & 1);
        }
        add_tile<MT, NT>(total, acc);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = total[mt][nt];
    } else {
      for (int s = 0; s < nsteps; ++s) {
        dma_barrier();   // step s landed for every wave; stage (s+1)&1 is free
        if (s + 1 < nsteps) issue(s + 1, (s + 1) & 1);
        compute(s & 1);
      }
    }
  }
  __syncthreads();     // last stage reads done before the epilogue reuses LDS

  if constexpr (EPI == EPI_GDN || EPI == EPI_IGDN) {
    static_assert(BN == CO, "GDN fusion needs every channel of a pixel in the workgroup");
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][nt][r] += a.bias[ncol0 + nt * 16 + (lane & 15)];
    gdn_epilogue<CO, MT, NT, EPI == EPI_IGDN, BMT, NWV * 64, XS>(acc, smem, a, t, wm, ncol0,
                                                                lane);
  } else if constexpr (EPI == EPI_QUANT) {
    quant_epilogue<CO, BN, MT, NT, WN>(acc, smem, a, t, wm, ncol0, lane, wave);
  } else if constexpr (EPI == EPI_OUT3) {
    out3_epilogue<MT, NT>(acc, smem, a, t, wm, lane, wave);
  } else if constexpr (EPI == EPI_GDN_BWD || EPI == EPI_IGDN_BWD) {
    static_assert(BN == CO, "GDN backward needs every channel of a pixel in the workgroup");
    gdn_bwd_epilogue<CO, MT, NT, EPI == EPI_IGDN_BWD>(acc, smem, a, t, wm, ncol0, lane);
  } else if constexpr (EPI == EPI_RATE_BWD) {
    rate_bwd_epilogue<CO, BN, MT, NT>(acc, smem, a, t, wm, ncol0, lane);
  } else {
    constexpr int OS = BN + 4;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = wm * MT * 16 + mt * 16 + 4 * (lane >> 4) + r;
          const int lcol = wn * (BN / WN) + nt * 16 + (lane & 15);
          float v = acc[mt][nt][r];
          if (a.bias != nullptr) v += a.bias[t.nb * BN + lcol];
          smem[row * OS + lcol] = v;
        }
    __syncthreads();
    store_tile_rows<BN>(a, t, smem, OS, a.out, CO, t.nb * BN);
  }
}

template <int CI, int CO, int BN, int WM, int WN, int EPI, bool X6 = false, bool W6 = false>
__global__ void __launch_bounds__(256) engine_kernel(const EngineArgs a) {
  engine_body<CI, CO, BN, WM, WN, EPI, X6, BM, W6>(a);
}

// The same kernel held to 256 VGPRs (2 waves per SIMD) where the compiler would otherwise just
// exceed it (the x6 GDN / IGDN backward instances).
template <int CI, int CO, int BN, int WM, int WN, int EPI, bool X6 = false>
__global__ void __launch_bounds__(256, 2) engine_kernel_occ2(const EngineArgs a) {
  engine_body<CI, CO, BN, WM, WN, EPI, X6>(a);
}

// ------------------------------------------------------------------------- host launch helpers
// An entry point validates, fills a zeroed EngineArgs by field name and hands it to a launcher
// (EngineArgs, N, stream), which adds what is derived and picks the instantiation.
inline EngineArgs zero_args() {
  EngineArgs a;
  memset(&a, 0, sizeof(a));
  return a;
}

inline hipStream_t S(void* s) { return (hipStream_t)s; }

// A runtime channel count (validated: 128 or 192) or flag as a compile-time constant:
// with_N(N, [&](auto n) { constexpr int CN = decltype(n)::value; … })
template <class F>
inline int with_N(int N, F&& f) {
  return N == 192 ? f(std::integral_constant<int, 192>{}) : f(std::integral_constant<int, 128>{});
}
template <class F>
inline int with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

}  // namespace iclr17
