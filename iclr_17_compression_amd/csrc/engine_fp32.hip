// The 8×8-tile engine's instantiations and entry points (gfx950), in its two operand flavours:
//   fp32  exact-f32 MFMA (v_mfma_f32_16x16x4_f32), the parity mode
//   x6    activations and weights as three bf16 planes, six v_mfma_f32_16x16x32_bf16 per MAC
// forward (conv2/conv3, deconv1/deconv2, the fp32 deconv3) and the fused backward epilogues
// (engine.h: engine_body), plus the two conv1 kernels with their own A-loaders (conv1_gdn_kernel,
// conv1_x6_kernel; forward, and as the adjoint of deconv3 in the backward pass) and the fp32 →
// x6 plane splitters (iclr17_split_planes, iclr17_split_packed).
// The stand-alone GDN / IGDN kernels (gdn_kernel, gdn_bwd_kernel) are here too, on purpose: compiled
// in a unit of their own, gdn_kernel and the fp32 engine_kernel<N, N, N, 1, 4, EPI_IGDN> both came
// out with 4 more VGPRs and another schedule (they share the gdn_core instantiations), so the
// family stays with the engine instantiations (profiles/engine_split_isa.txt).
// The halo deconv3 kernels of the x6, h3 and bf16 modes are in deconv3_halo.hip, the error state
// and shape checks in runtime.hip.
#include "engine.h"

namespace iclr17 {

// conv3 (+ quantiser) output columns per workgroup: 96 at N = 192, 64 at N = 128
constexpr int conv3_bn(int N) { return N % 96 == 0 ? 96 : 64; }
// x6 conv3 in noise mode (training) on few tiles (B·tiles < 256: B=32 at 256² holds 256
// workgroups, one wave per SIMD): 48-column tiles on 4×1 waves, twice the workgroups. The bit
// partials per image follow (tiles × N/48): iclr17_conv3_x6_partials_per_image.
inline bool conv3_narrow(int N, int tiles, int B, int qmode) {
  return N == 192 && qmode == ICLR17_QUANT_NOISE && (long)tiles * B < 256;
}

// ------------------------------------------------------------------------------ conv1 kernel
// Conv2d(3, N, 9, stride 4, pad 4) on the NCHW image with GDN fused. The 37×37×3 input patch of
// an 8×8 output block is staged once in LDS; K = 243 = (c, kh, kw) padded to 256, each A element
// gathered from the patch through a k → offset table (k ≥ 243 reads a zero slot).
constexpr int P1 = 37;                    // patch side: 8·4 + 9 − 4
constexpr int P1RS = 40;                  // LDS row stride: 10 16-byte pieces (cols 37..39 unused)
constexpr int P1PLANE = P1 * P1RS;
constexpr int P1PIECES = 3 * P1 * 10;     // 16-byte pieces of the patch (1110)
constexpr int P1NI = (P1PIECES + 63) / 64;  // glds wave-instructions (18)
constexpr int P1ZERO = P1NI * 256;        // zero slot, after the DMA'd region

// EPI_GDN: analysis conv1 + bias + GDN1 (forward). EPI_IGDN_BWD: the same contraction is the
// input gradient of the synthesis deconv3 (its adjoint: conv2d(g_recon, W, stride 4, pad 4)),
// fused with the IGDN2 backward.
template <int CO, int EPI, bool G6 = false>
__global__ void __launch_bounds__(256) conv1_gdn_kernel(const EngineArgs a) {
  constexpr int WN = 4;
  constexpr int MT = BM / 16;
  constexpr int NT = CO / WN / 16;
  constexpr int LDS_PB = P1ZERO + 4 + 256 + 64;   // patch + zero slot + k/m tables
  constexpr int LDS_P = LDS_PB + 2 * 32 * CO;                        // + two B stages
  constexpr int LDS_X = gdn_lds_floats(BM, CO, G6) > BM * (CO + 8) + GSTAGE_FLOATS(CO)
                            ? gdn_lds_floats(BM, CO, G6) : BM * (CO + 8) + GSTAGE_FLOATS(CO);
  constexpr int LDS_FLOATS = LDS_P > LDS_X ? LDS_P : LDS_X;
  __shared__ __attribute__((aligned(16))) float smem[LDS_FLOATS];
  int* ktab = (int*)(smem + P1ZERO + 4);
  int* mtab = ktab + 256;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = 0, wn = wave;
  const TileInfo t = decode_tile(a);
  const int ncol0 = wn * (CO / WN);
  const int H = a.Hin, W = a.Win;
  const int iy0 = t.ty * 32 - 4, ix0 = t.tx * 32 - 4;

  // B tiles (32 k-rows × CO, contiguous in the packed [64][CO][4] layout) by LDS-DMA into two
  // stages after the patch; step 0's DMA overlaps the patch staging.
  constexpr int SB = 32 * CO;
  constexpr int NBI = SB * 4 / 1024;
  constexpr int BI_W = (NBI + 3) / 4;
  float* sB = smem + LDS_PB;
  auto issue = [&](int s, int buf) {
    const float* src = a.w + s * SB + lane * 4;
#pragma unroll
    for (int j = 0; j < BI_W; ++j) {
      const int i = wave + 4 * j;
      if (NBI % 4 == 0 || i < NBI) glds16(src + i * 256, sB + buf * SB + i * 256);
    }
  };
  issue(0, 0);

  // Patch by LDS-DMA, one 16-byte piece per lane: piece (c, r, q) holds columns 4q .. 4q+3 of
  // patch row r of channel c. The patch origin ix0 ≡ 0 (mod 4) and W ≡ 0 (mod 16), so a piece is
  // wholly inside or wholly outside the image; outside pieces copy the zero line.
#pragma unroll
  for (int j = 0; j < (P1NI + 3) / 4; ++j) {
    const int i = wave + 4 * j;
    if (i < P1NI) {
      const int pc = i * 64 + lane;
      const int cr = pc / 10, q = pc - cr * 10;
      const int c = cr / P1, r = cr - c * P1;
      const int iy = iy0 + r, ix = ix0 + 4 * q;
      const bool ok = pc < P1PIECES && iy >= 0 && iy < H && ix >= 0 && ix < W;
      glds16(ok ? a.in + (((long)t.b * 3 + c) * H + iy) * W + ix : g_zero16, smem + i * 256);
    }
  }
  if (tid == 0) smem[P1ZERO] = 0.f;
  {
    const int k = tid;  // 256 threads ↔ 256 k values
    int off = P1ZERO;
    if (k < 243) {
      const int c = k / 81, kh = (k % 81) / 9, kw = k % 9;
      off = c * P1PLANE + kh * P1RS + kw;
    }
    ktab[k] = off;
    if (tid < 64) mtab[tid] = (tid >> 3) * 4 * P1RS + (tid & 7) * 4;
  }
  dma_barrier();   // patch (and the tables) published

  f4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};

  int moff[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) moff[mt] = mtab[mt * 16 + (lane & 15)];

  const int boff = ((lane >> 4) * CO + ncol0 + (lane & 15)) * 4;
  for (int s = 0; s < 8; ++s) {
    dma_barrier();   // B stage s landed (and, at s = 0, the patch); stage (s+1)&1 is free
    if (s + 1 < 8) issue(s + 1, (s + 1) & 1);
    const float* bs = sB + (s & 1) * SB + boff;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f4 bf[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) bf[nt] = *(const f4*)(bs + kk * 16 * CO + nt * 64);
      const int kbase = s * 32 + kk * 16 + 4 * (lane >> 4);
      int ko[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) ko[e] = ktab[kbase + e];
      f4 af[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = ko[e] == P1ZERO ? P1ZERO : ko[e] + moff[mt];
          af[mt][e] = smem[o];
        }
      mfma_block<MT, NT>(acc, af, bf);
    }
  }
  __syncthreads();  // patch reads done before the epilogue reuses LDS
  if constexpr (EPI == EPI_GDN) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][nt][r] += a.bias[ncol0 + nt * 16 + (lane & 15)];
    gdn_epilogue<CO, MT, NT, false, BM, 256, G6>(acc, smem, a, t, wm, ncol0, lane);
  } else {
    static_assert(EPI == EPI_IGDN_BWD, "conv1 kernel epilogues: GDN fwd, IGDN bwd");
    gdn_bwd_epilogue<CO, MT, NT, true>(acc, smem, a, t, wm, ncol0, lane);
  }
}

// ------------------------------------------------------------------- conv1, x6 contraction
// conv1 + GDN1 with both contractions in x6 (analysis_17.py:14-17). The 37×37×3 patch arrives
// by LDS-DMA as before and is then split once into three bf16 planes [3][3·37][40] in LDS, so
// the main loop does no splitting. K is reordered so that a lane's 8-deep k-group is 8
// consecutive patch columns of one row: k' = 8g + e with
//   g < 27      : (c, kh) = (g / 9, g % 9), kw = e           — one 16-byte read per plane
//   g = 27      : zero weights (the lane reads a valid row; 0 · finite = 0)
//   g = 28 .. 31: pair (g − 28)·8 + e (zero weights past 26), kw = 8 — gathered element-wise
// (packing ICLR17_W_CONV1_X6, then iclr17_split_packed). The weights' split planes
// [3][32][CO][8] are read from L2 one step ahead, like the x6 GDN γ: no B image in LDS, and no
// barrier in the main loop.
// Split-plane rows are 64 u16 (128 bytes, 16 granules of 4 elements); granule j of row r is
// stored at j ^ 8·((r >> 2) & 1). A fragment read's 32-lane half touches rows r, r+4 (the two
// output-pixel rows of a 16-lane group) and the next k-group's r', r'+4: the 128-byte stride
// puts rows two 64-byte bank quarters apart and the swizzle moves r+4 by one more, so the four
// 64-byte windows fall in distinct quarters (no bank conflicts on the 8-byte reads).
constexpr int X1RS = 64;                  // u16 per split-plane row
constexpr int P1U = 3 * P1 * X1RS;        // u16 elements per split plane (7104)
__host__ __device__ constexpr int x1_off(int row, int gran) {
  return row * X1RS + ((gran ^ (((row >> 2) & 1) << 3)) << 2);
}

template <int CO, int EPI>
__global__ void __launch_bounds__(256, 2) conv1_x6_kernel(const EngineArgs a) {
  constexpr int WN = 4;
  constexpr int MT = BM / 16;
  constexpr int NT = CO / WN / 16;
  constexpr int S_FLOATS = 3 * P1U / 2;                 // split planes (6660 floats)
  constexpr int LDS_P = S_FLOATS + P1NI * 256;          // + the fp32 DMA landing area
  constexpr int LDS_X = EPI == EPI_IGDN_BWD ? BM * (CO + 8) + GSTAGE_FLOATS(CO)
                                            : gdn_lds_floats(BM, CO, true) > BM * (CO + 8)
                                                  ? gdn_lds_floats(BM, CO, true) : BM * (CO + 8);
  constexpr int LDS_FLOATS = LDS_P > LDS_X ? LDS_P : LDS_X;
  __shared__ __attribute__((aligned(16))) float smem[LDS_FLOATS];
  unsigned short* sp = (unsigned short*)smem;
  float* sr = smem + S_FLOATS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = 0, wn = wave;
  const TileInfo t = decode_tile(a);
  const int ncol0 = wn * (CO / WN);
  const int H = a.Hin, W = a.Win;
  const int iy0 = t.ty * 32 - 4, ix0 = t.tx * 32 - 4;

  // Patch by LDS-DMA into the landing area (pieces as in conv1_gdn_kernel).
#pragma unroll
  for (int j = 0; j < (P1NI + 3) / 4; ++j) {
    const int i = wave + 4 * j;
    if (i < P1NI) {
      const int pc = i * 64 + lane;
      const int cr = pc / 10, q = pc - cr * 10;
      const int c = cr / P1, r = cr - c * P1;
      const int iy = iy0 + r, ix = ix0 + 4 * q;
      const bool ok = pc < P1PIECES && iy >= 0 && iy < H && ix >= 0 && ix < W;
      glds16(ok ? a.in + (((long)t.b * 3 + c) * H + iy) * W + ix : g_zero16, sr + i * 256);
    }
  }
  // Weight planes: lane's B fragment base (k-group lane >> 4, column ncol0 + lane & 15).
  constexpr long GP = 32L * CO * 8;                     // plane stride (u16)
  const unsigned short* gb = (const unsigned short*)a.w + ((lane >> 4) * CO + ncol0 + (lane & 15)) * 8;
  u4 b0[3][NT], b1[3][NT];
  auto loadb = [&](int s, u4 (&b)[3][NT]) {
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        b[p][nt] = *(const u4*)(gb + p * GP + (long)s * 4 * CO * 8 + nt * 128);
  };
  loadb(0, b0);
  dma_barrier();   // patch landed

  // Split pass: piece pc (4 floats at column 4q of row cr) → 4 bf16 in each plane.
  for (int pc = tid; pc < P1PIECES; pc += 256) {
    const f4 x = *(const f4*)(sr + pc * 4);
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      h[i] = __float_as_uint(x[i]) & 0xffff0000u;
      const float r = x[i] - __uint_as_float(h[i]);
      m[i] = __float_as_uint(r) & 0xffff0000u;
      l[i] = __float_as_uint(r - __uint_as_float(m[i]));
    }
    const int cr = pc / 10, q = pc - cr * 10;
    const int o = x1_off(cr, q);   // u16 offset of the piece's granule
    *(uint2*)(sp + o) = uint2{__builtin_amdgcn_perm(h[1], h[0], 0x07060302u),
                              __builtin_amdgcn_perm(h[3], h[2], 0x07060302u)};
    *(uint2*)(sp + P1U + o) = uint2{__builtin_amdgcn_perm(m[1], m[0], 0x07060302u),
                                    __builtin_amdgcn_perm(m[3], m[2], 0x07060302u)};
    *(uint2*)(sp + 2 * P1U + o) = uint2{__builtin_amdgcn_perm(l[1], l[0], 0x07060302u),
                                        __builtin_amdgcn_perm(l[3], l[2], 0x07060302u)};
  }
  __syncthreads();   // planes published

  f4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};

  // Output pixel (my, mx) = (2·mt + b, lane & 7), b = (lane >> 3) & 1, reads patch row 4·my
  // (+ the pair's row) and granule mx (column 4·mx). The swizzle bit of row prow + 4b + 8mt does
  // not depend on mt.
  const int mx = lane & 7, b4 = 4 * ((lane >> 3) & 1);
  const int kg = lane >> 4;
  auto pair_row = [](int p) { return (p / 9) * P1 + p % 9; };

  auto mfma6 = [&](int mt, const bf8& Ah, const bf8& Am, const bf8& Al, const u4 (&b)[3][NT]) {
    X6Acc st;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const bf8 Bh = __builtin_bit_cast(bf8, b[0][nt]), Bm = __builtin_bit_cast(bf8, b[1][nt]),
                Bl = __builtin_bit_cast(bf8, b[2][nt]);
      mfma_x6<false>(acc, st, mt, nt, Ah, Am, Al, Bh, Bm, Bl);
    }
    x6_flush<false>(acc, st);
  };
  // Steps 0..6: 8 consecutive columns of one patch row per lane (two 8-byte reads per plane).
  auto step_rows = [&](int s, const u4 (&b)[3][NT]) {
    const int g = 4 * s + kg;
    const int r0 = pair_row(g < 27 ? g : 26) + b4;
    const int lo_off = x1_off(r0, mx), hi_off = x1_off(r0, mx + 1);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const unsigned short* e = sp + mt * 8 * X1RS;
      u4 v[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const uint2 lo2 = *(const uint2*)(e + p * P1U + lo_off);
        const uint2 hi2 = *(const uint2*)(e + p * P1U + hi_off);
        v[p] = u4{lo2.x, lo2.y, hi2.x, hi2.y};
      }
      mfma6(mt, __builtin_bit_cast(bf8, v[0]), __builtin_bit_cast(bf8, v[1]),
            __builtin_bit_cast(bf8, v[2]), b);
    }
  };
  // Step 7: column kw = 8 of pairs 8·kg + e (e = 0..7), gathered element-wise.
  auto step_col8 = [&](const u4 (&b)[3][NT]) {
    int po[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int p = 8 * kg + e;
      po[e] = x1_off(pair_row(p < 27 ? p : 26) + b4, mx + 2);   // column 4·mx + 8
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      u4 v[3];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned lo = sp[p * P1U + po[2 * i] + mt * 8 * X1RS];
          const unsigned hi = sp[p * P1U + po[2 * i + 1] + mt * 8 * X1RS];
          v[p][i] = lo | (hi << 16);
        }
      mfma6(mt, __builtin_bit_cast(bf8, v[0]), __builtin_bit_cast(bf8, v[1]),
            __builtin_bit_cast(bf8, v[2]), b);
    }
  };
  loadb(1, b1);
  step_rows(0, b0);
  loadb(2, b0);
  step_rows(1, b1);
  loadb(3, b1);
  step_rows(2, b0);
  loadb(4, b0);
  step_rows(3, b1);
  loadb(5, b1);
  step_rows(4, b0);
  loadb(6, b0);
  step_rows(5, b1);
  loadb(7, b1);
  step_rows(6, b0);
  step_col8(b1);

  __syncthreads();  // patch reads done before the epilogue reuses LDS
  if constexpr (EPI == EPI_GDN) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][nt][r] += a.bias[ncol0 + nt * 16 + (lane & 15)];
    gdn_epilogue<CO, MT, NT, false, BM, 256, true>(acc, smem, a, t, wm, ncol0, lane);
  } else {
    static_assert(EPI == EPI_IGDN_BWD, "conv1 x6 epilogues: GDN fwd, IGDN bwd");
    gdn_bwd_epilogue<CO, MT, NT, true>(acc, smem, a, t, wm, ncol0, lane);
  }
}

// x → three exact bf16 planes (x6 activation format), 8 values per thread
__global__ void __launch_bounds__(256) split_planes_kernel(const float* __restrict__ x, long n8,
                                                           unsigned short* __restrict__ planes,
                                                           long plane) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    u4 hi, mi, lo;
    split8(*(const f4*)(x + 8 * i), *(const f4*)(x + 8 * i + 4), hi, mi, lo);
    *(u4*)(planes + 8 * i) = hi;
    *(u4*)(planes + plane + 8 * i) = mi;
    *(u4*)(planes + 2 * plane + 8 * i) = lo;
  }
}

// packed fp32 operand [taps][K/4][N][4] → split planes [3][taps][K/8][N][8] bf16 (the
// B-fragment layout of v_mfma_f32_16x16x32_bf16), exact
__global__ void __launch_bounds__(256) split_packed_kernel(const float* __restrict__ w, int taps,
                                                           int K, int N,
                                                           unsigned short* __restrict__ planes) {
  const long n = (long)taps * (K / 8) * N;   // 8-element groups
  for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < n; g += (long)gridDim.x * 256)
    split_packed_group(w, K, N, n * 8, planes, g);
}

// --------------------------------------------------------------------- stand-alone GDN / IGDN
// GDN.forward (models/GDN.py:64-94) on a [B,C,H,W] tensor stored NCHW or NHWC: 64 pixels of one
// image per workgroup (linear pixel order), all C channels, the same fused core as the layers.
template <int C, bool INVERSE, int LAYOUT>
__global__ void __launch_bounds__(256) gdn_kernel(const float* __restrict__ x, int HW,
                                                  const float* __restrict__ beta,
                                                  const float* __restrict__ gp, float* y) {
  constexpr int XS = C + 8;   // must match gdn_core's row stride
  constexpr int WN = 4, MT = 4, NT = C / WN / 16;
  __shared__ __attribute__((aligned(16))) float smem[BM * XS + GSTAGE_FLOATS(C)];   // + γ stages
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = (HW + BM - 1) / BM;
  const int b = blockIdx.x / tiles, p0 = (blockIdx.x % tiles) * BM;
  const int np = HW - p0 < BM ? HW - p0 : BM;
  const int ncol0 = wave * (C / WN);
  if constexpr (LAYOUT == ICLR17_LAYOUT_NCHW) {
    for (int idx = tid; idx < BM * C; idx += 256) {
      const int c = idx / BM, pl = idx % BM;
      smem[pl * XS + c] = pl < np ? x[((long)b * C + c) * HW + p0 + pl] : 0.f;
    }
  } else {
    for (int idx = tid; idx < BM * (C / 4); idx += 256) {
      const int pl = idx / (C / 4), c4 = idx % (C / 4);
      const f4 v = pl < np ? *(const f4*)(x + ((long)b * HW + p0 + pl) * C + c4 * 4) : f4{0.f, 0.f, 0.f, 0.f};
      *(f4*)(smem + pl * XS + c4 * 4) = v;
    }
  }
  __syncthreads();
  f4 v[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        v[mt][nt][r] = smem[(mt * 16 + 4 * (lane >> 4) + r) * XS + ncol0 + nt * 16 + (lane & 15)];
  __syncthreads();
  gdn_core<C, MT, NT, INVERSE>(v, smem, beta, gp, 0, ncol0, lane);
  if constexpr (LAYOUT == ICLR17_LAYOUT_NCHW) {
    for (int idx = tid; idx < BM * C; idx += 256) {
      const int c = idx / BM, pl = idx % BM;
      if (pl < np) y[((long)b * C + c) * HW + p0 + pl] = smem[pl * XS + c];
    }
  } else {
    for (int idx = tid; idx < BM * (C / 4); idx += 256) {
      const int pl = idx / (C / 4), c4 = idx % (C / 4);
      if (pl < np) *(f4*)(y + ((long)b * HW + p0 + pl) * C + c4 * 4) = *(const f4*)(smem + pl * XS + c4 * 4);
    }
  }
}

// ------------------------------------------------------------ stand-alone GDN / IGDN backward
// Autograd of GDN.forward (models/GDN.py:64-94) for the stand-alone module: from x (= u) and
// g = ∂L/∂y, the same op-for-op chain as gdn_bwd_epilogue — n = β + γ·u², s = √n,
//   GDN : ∂u = g/s + 2u·(γᵀ dn),  dn = ((−g·u)/(s·s)) / (2s)
//   IGDN: ∂u = g·s + 2u·(γᵀ dn),  dn = (g·u) / (2s)
// — on 64 pixels of one image per workgroup (linear pixel order, ragged last tile). Writes ∂x in
// the input's layout, dn NHWC [B·HW][C] (for dβ = Σ dn and dγ = Σ dn ⊗ u²) and, for an NCHW
// input, u NHWC (the operand of the γ gradient).
template <int C, bool INVERSE, int LAYOUT>
__global__ void __launch_bounds__(256) gdn_bwd_kernel(const float* __restrict__ x,
                                                      const float* __restrict__ gy, int HW,
                                                      const float* __restrict__ beta,
                                                      const float* __restrict__ gp,
                                                      const float* __restrict__ gpt, float* dx,
                                                      float* dn_out, float* u_out) {
  constexpr int XS = C + 8;
  constexpr int WN = 4, MT = 4, NT = C / WN / 16;
  __shared__ __attribute__((aligned(16))) float smem[BM * XS + GSTAGE_FLOATS(C)];
  float* sX = smem;
  float* sG = smem + BM * XS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = (HW + BM - 1) / BM;
  const int b = blockIdx.x / tiles, p0 = (blockIdx.x % tiles) * BM;
  const int np = HW - p0 < BM ? HW - p0 : BM;
  const int ncol0 = wave * (C / WN);
  auto gidx = [&](int pl, int c) -> long {   // element (pixel p0 + pl, channel c) of x / g / ∂x
    return LAYOUT == ICLR17_LAYOUT_NCHW ? ((long)b * C + c) * HW + p0 + pl
                                        : ((long)b * HW + p0 + pl) * C + c;
  };
  for (int idx = tid; idx < BM * C; idx += 256) {
    const int pl = LAYOUT == ICLR17_LAYOUT_NCHW ? idx % BM : idx / C;
    const int c = LAYOUT == ICLR17_LAYOUT_NCHW ? idx / BM : idx % C;
    sX[pl * XS + c] = pl < np ? x[gidx(pl, c)] : 0.f;
  }
  f4 g[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int pl = mt * 16 + 4 * (lane >> 4) + r, c = ncol0 + nt * 16 + (lane & 15);
        g[mt][nt][r] = pl < np ? gy[gidx(pl, c)] : 0.f;
      }
  f4 acc2[MT][NT];
  chan_gemm_lds<C, MT, NT, true>(acc2, sX, gp, sG, 0, ncol0, lane, wave);   // Σ_j γ[i][j] u_j²
  __syncthreads();
  f4 u[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = ncol0 + nt * 16 + (lane & 15);
        const int i = (mt * 16 + 4 * (lane >> 4) + r) * XS + col;
        const float uu = sX[i];
        const float sq = sqrtf(acc2[mt][nt][r] + beta[col]);
        const float gg = g[mt][nt][r];
        float dn;
        if (INVERSE) {
          g[mt][nt][r] = gg * sq;
          dn = (gg * uu) / (2.0f * sq);
        } else {
          g[mt][nt][r] = gg / sq;
          dn = ((-gg * uu) / (sq * sq)) / (2.0f * sq);
        }
        u[mt][nt][r] = uu;
        sX[i] = dn;
      }
  chan_gemm_lds<C, MT, NT>(acc2, sX, gpt, sG, 0, ncol0, lane, wave);   // w_j = Σ_i γ[i][j] dn_i
  for (int idx = tid; idx < np * (C / 4); idx += 256) {   // dn rows (NHWC)
    const int pl = idx / (C / 4), c4 = idx % (C / 4);
    *(f4*)(dn_out + ((long)b * HW + p0 + pl) * C + c4 * 4) = *(const f4*)(sX + pl * XS + c4 * 4);
  }
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = (mt * 16 + 4 * (lane >> 4) + r) * XS + ncol0 + nt * 16 + (lane & 15);
        sX[i] = g[mt][nt][r] + acc2[mt][nt][r] * (2.0f * u[mt][nt][r]);
      }
  __syncthreads();
  for (int idx = tid; idx < BM * C; idx += 256) {
    const int pl = LAYOUT == ICLR17_LAYOUT_NCHW ? idx % BM : idx / C;
    const int c = LAYOUT == ICLR17_LAYOUT_NCHW ? idx / BM : idx % C;
    if (pl < np) dx[gidx(pl, c)] = sX[pl * XS + c];
  }
  if (u_out != nullptr) {
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          sX[(mt * 16 + 4 * (lane >> 4) + r) * XS + ncol0 + nt * 16 + (lane & 15)] = u[mt][nt][r];
    __syncthreads();
    for (int idx = tid; idx < np * (C / 4); idx += 256) {
      const int pl = idx / (C / 4), c4 = idx % (C / 4);
      *(f4*)(u_out + ((long)b * HW + p0 + pl) * C + c4 * 4) = *(const f4*)(sX + pl * XS + c4 * 4);
    }
  }
}

// ====================================================================================== host
// Launchers: the entry point has filled pointers, B, the input grid Hin × Win and the x6 planes;
// the launcher adds everything derived from them and picks the instantiation.
namespace {

void fill_conv5_taps(TapTable& tt) {
  memset(&tt, 0, sizeof(tt));
  tt.npx = 1;
  tt.nph = 1;
  tt.begin[0] = 0;
  tt.begin[1] = 25;
  for (int kh = 0; kh < 5; ++kh)
    for (int kw = 0; kw < 5; ++kw) tt.dydx[kh * 5 + kw] = pack_tap(kh - 2, kw - 2);
}

// Phase-major tap order; the packing kernel uses the same enumeration (for_each_deconv_tap).
void fill_deconv_taps(TapTable& tt, int K, int s, int p) {
  memset(&tt, 0, sizeof(tt));
  tt.npx = s;
  tt.nph = s * s;
  int n = 0;
  for (int ry = 0; ry < s; ++ry)
    for (int rx = 0; rx < s; ++rx) {
      tt.begin[ry * s + rx] = n;
      for_each_deconv_tap(K, s, p, ry, rx,
                          [&](int dy, int dx, int, int) { tt.dydx[n++] = pack_tap(dy, dx); });
    }
  tt.begin[s * s] = n;
}

void fill_neigh3_taps(TapTable& tt) {
  memset(&tt, 0, sizeof(tt));
  tt.npx = 1;
  tt.nph = 1;
  tt.begin[1] = 9;
  for (int i = 0; i < 9; ++i) tt.dydx[i] = pack_tap(i / 3 - 1, i % 3 - 1);
}

// Output size, base grid gh × gw in 8×8 tiles, and the strides applied to base coordinates.
void set_geometry(EngineArgs& a, int Hout, int Wout, int gh, int gw, int sin, int sout) {
  a.Hout = Hout; a.Wout = Wout;
  a.gh = gh; a.gw = gw; a.tiles_y = (gh + 7) / 8; a.tiles_x = (gw + 7) / 8;
  a.sin = sin; a.sout = sout;
}

// conv1 (k9 s4) on the Hin × Win image. W_SPLIT: a.w holds the split ICLR17_W_CONV1_X6 planes and
// the contraction itself runs in x6 (conv1_x6_kernel).
enum Conv1Weights { W_PACKED, W_SPLIT };

template <int EPI, Conv1Weights WF = W_PACKED>
int launch_conv1(EngineArgs a, int N, hipStream_t st) {
  set_geometry(a, a.Hin / 4, a.Win / 4, a.Hin / 4, a.Win / 4, 4, 1);
  a.tt.npx = 1; a.tt.nph = 1;
  const dim3 grid(a.tiles_x * a.tiles_y * a.B, 1);
  return with_N(N, [&](auto n) {
    constexpr int CN = decltype(n)::value;
    if constexpr (WF == W_SPLIT) {
      hipLaunchKernelGGL((conv1_x6_kernel<CN, EPI>), grid, dim3(256), 0, st, a);
      return check_launch(EPI == EPI_GDN ? "conv1x6_gdn" : "bwd_deconv3_igdn_x6");
    } else if constexpr (EPI == EPI_GDN) {
      if (a.ggamma6 != nullptr)
        hipLaunchKernelGGL((conv1_gdn_kernel<CN, EPI, true>), grid, dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((conv1_gdn_kernel<CN, EPI>), grid, dim3(256), 0, st, a);
      return check_launch("conv1_gdn");
    } else {
      hipLaunchKernelGGL((conv1_gdn_kernel<CN, EPI>), grid, dim3(256), 0, st, a);
      return check_launch("bwd_deconv3_igdn");
    }
  });
}

// k5 s2 convolution on the Hin × Win input grid (conv2, conv3, and the input gradients of the
// deconvs, whose adjoint it is).
template <int EPI>
int launch_conv5(EngineArgs a, int N, hipStream_t st) {
  set_geometry(a, a.Hin / 2, a.Win / 2, a.Hin / 2, a.Win / 2, 2, 1);
  fill_conv5_taps(a.tt);
  const bool X6in = a.in_split != nullptr;
  const int tiles = a.tiles_x * a.tiles_y, B = a.B;
  return with_N(N, [&](auto n) {
    constexpr int CN = decltype(n)::value;
    if constexpr (EPI == EPI_QUANT) {
      // Column split of conv3: 96 columns (2×2 waves) at N = 192 — B=64 gives 512 workgroups, one
      // round of slots, and 20 % fewer operand bytes per MAC than 64-column tiles.
      constexpr int BN = conv3_bn(CN);
      constexpr int WN = (BN / 16) % 4 == 0 ? 4 : 2, WM = 4 / WN;
      a.partials_per_image = tiles * (CN / BN);
      const dim3 grid(tiles * B, CN / BN);
      if constexpr (CN == 192) {
        if (X6in && conv3_narrow(CN, tiles, B, a.qmode)) {
          a.partials_per_image = tiles * (CN / 48);
          a.w6 = nullptr;   // the narrow instantiation splits its weights per k-step
          hipLaunchKernelGGL((engine_kernel<CN, CN, 48, 4, 1, EPI_QUANT, true>),
                             dim3(tiles * B, CN / 48), dim3(256), 0, st, a);
          return check_launch("conv3_quant_rate (48-column tiles)");
        }
      }
      if (X6in && a.w6 != nullptr)
        hipLaunchKernelGGL((engine_kernel<CN, CN, BN, WM, WN, EPI_QUANT, true, true>), grid,
                           dim3(256), 0, st, a);
      else if (X6in)
        hipLaunchKernelGGL((engine_kernel<CN, CN, BN, WM, WN, EPI_QUANT, true>), grid, dim3(256),
                           0, st, a);
      else
        hipLaunchKernelGGL((engine_kernel<CN, CN, BN, WM, WN, EPI_QUANT>), grid, dim3(256), 0, st,
                           a);
      return check_launch("conv3_quant_rate");
    } else if constexpr (EPI == EPI_PLAIN || EPI == EPI_RATE_BWD) {
      constexpr int BN = 64;
      const dim3 grid(tiles * B, CN / BN);
      if (EPI == EPI_RATE_BWD && X6in)
        hipLaunchKernelGGL((engine_kernel<CN, CN, BN, 1, 4, EPI, true>), grid, dim3(256), 0, st, a);
      else
        hipLaunchKernelGGL((engine_kernel<CN, CN, BN, 1, 4, EPI>), grid, dim3(256), 0, st, a);
      return check_launch(EPI == EPI_PLAIN ? "conv3" : "bwd_deconv1_rate");
    } else {
      const dim3 grid(tiles * B, 1);
      if constexpr (EPI == EPI_GDN) {
        if (X6in) {
          hipLaunchKernelGGL((engine_kernel<CN, CN, CN, 1, 4, EPI, true>), grid, dim3(256), 0, st, a);
          return check_launch("conv2_gdn");
        }
      } else if constexpr (EPI == EPI_IGDN_BWD) {
        if (X6in) {   // held to 256 VGPRs: two waves per SIMD
          hipLaunchKernelGGL((engine_kernel_occ2<CN, CN, CN, 1, 4, EPI, true>), grid, dim3(256), 0,
                             st, a);
          return check_launch("bwd_deconv_igdn");
        }
      }
      hipLaunchKernelGGL((engine_kernel<CN, CN, CN, 1, 4, EPI>), grid, dim3(256), 0, st, a);
      return check_launch("conv2_gdn");
    }
  });
}

// k5 s2 transposed convolution on the Hin × Win input grid (deconv1, deconv2, and the input
// gradient of conv2 / conv3): one workgroup per (base tile, stride phase), phase-major, the
// 9-tap phase first.
template <int EPI>
int launch_deconv5(EngineArgs a, int N, hipStream_t st) {
  set_geometry(a, 2 * a.Hin, 2 * a.Win, a.Hin, a.Win, 1, 2);
  fill_deconv_taps(a.tt, 5, 2, 2);
  const dim3 grid(a.tiles_x * a.tiles_y * a.B * 4);
  return with_N(N, [&](auto n) {
    constexpr int CN = decltype(n)::value;
    if (a.in_split != nullptr) {
      if constexpr (EPI == EPI_IGDN)
        hipLaunchKernelGGL((engine_kernel<CN, CN, CN, 1, 4, EPI, true>), grid, dim3(256), 0, st, a);
      else   // held to 256 VGPRs: two waves per SIMD
        hipLaunchKernelGGL((engine_kernel_occ2<CN, CN, CN, 1, 4, EPI, true>), grid, dim3(256), 0,
                           st, a);
    } else {
      hipLaunchKernelGGL((engine_kernel<CN, CN, CN, 1, 4, EPI>), grid, dim3(256), 0, st, a);
    }
    return check_launch(EPI == EPI_IGDN ? "deconv_igdn" : "bwd_conv_gdn");
  });
}

// fp32 deconv3 (k9 s4, N → 3) as the engine's all-phase GEMM; a.Hin × a.Win is its input grid.
int launch_deconv3(EngineArgs a, int N, hipStream_t st) {
  set_geometry(a, 4 * a.Hin, 4 * a.Win, a.Hin, a.Win, 1, 4);
  a.partials_per_image = a.tiles_x * a.tiles_y;
  fill_neigh3_taps(a.tt);
  const dim3 grid(a.tiles_x * a.tiles_y * a.B, 1);
  return with_N(N, [&](auto n) {
    constexpr int CN = decltype(n)::value;
    hipLaunchKernelGGL((engine_kernel<CN, 48, 48, 4, 1, EPI_OUT3>), grid, dim3(256), 0, st, a);
    return check_launch("deconv3");
  });
}

// x6 activation planes [3][B][h][w][N]: the plane stride in elements
long plane(int B, int h, int w, int N) { return (long)B * h * w * N; }

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_analysis_conv1_gdn(const float* x, int B, int H, int W, int N, const float* w_packed,
                              const float* bias, const float* beta_eff, const float* gamma_packed,
                              float* out, float* pre_out, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(x && w_packed && bias && beta_eff && gamma_packed && out, ICLR17_EINVAL,
                 "conv1_gdn: null pointer");
  EngineArgs a = zero_args();
  a.in = x; a.w = w_packed; a.bias = bias; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.out = out; a.pre = pre_out;
  a.B = B; a.Hin = H; a.Win = W;
  return launch_conv1<EPI_GDN>(a, N, S(stream));
}

int iclr17_analysis_conv2_gdn(const float* in, int B, int H, int W, int N, const float* w_packed,
                              const float* bias, const float* beta_eff, const float* gamma_packed,
                              float* out, float* pre_out, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in && w_packed && bias && beta_eff && gamma_packed && out, ICLR17_EINVAL,
                 "conv2_gdn: null pointer");
  EngineArgs a = zero_args();
  a.in = in; a.w = w_packed; a.bias = bias; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.out = out; a.pre = pre_out;
  a.B = B; a.Hin = H / 4; a.Win = W / 4;
  return launch_conv5<EPI_GDN>(a, N, S(stream));
}

int iclr17_conv3_x6_partials_per_image(int B, int H, int W, int N, int quant_mode) {
  const int gh = H / 16, gw = W / 16, tiles = ((gh + 7) / 8) * ((gw + 7) / 8);
  return tiles * (conv3_narrow(N, tiles, B, quant_mode) ? N / 48 : N / conv3_bn(N));
}

int iclr17_rate_partials_per_image(int H, int W, int N) {
  const int gh = H / 16, gw = W / 16;
  return ((gh + 7) / 8) * ((gw + 7) / 8) * (N / conv3_bn(N));
}

int iclr17_analysis_conv3_quant_rate(const float* in, int B, int H, int W, int N,
                                     const float* w_packed, int quant_mode, const float* noise,
                                     const float* rate_packed, const float* rate_table,
                                     float* y_out, float* y_hat, double* bits_partial,
                                     void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in && w_packed && rate_packed && y_hat && bits_partial, ICLR17_EINVAL,
                 "conv3_quant_rate: null pointer");
  ICLR17_REQUIRE(quant_mode == ICLR17_QUANT_ROUND || (quant_mode == ICLR17_QUANT_NOISE && noise),
                 ICLR17_EINVAL, "conv3_quant_rate: bad quant mode %d / missing noise", quant_mode);
  EngineArgs a = zero_args();
  a.in = in; a.w = w_packed; a.out = y_out;
  a.qmode = quant_mode; a.noise = noise; a.rate = rate_packed; a.rtab = rate_table;
  a.yhat = y_hat; a.partial = bits_partial;
  a.B = B; a.Hin = H / 8; a.Win = W / 8;
  return launch_conv5<EPI_QUANT>(a, N, S(stream));
}

int iclr17_analysis_conv3(const float* in, int B, int H, int W, int N, const float* w_packed,
                          float* y_out, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in && w_packed && y_out, ICLR17_EINVAL, "conv3: null pointer");
  EngineArgs a = zero_args();
  a.in = in; a.w = w_packed; a.out = y_out;
  a.B = B; a.Hin = H / 8; a.Win = W / 8;
  return launch_conv5<EPI_PLAIN>(a, N, S(stream));
}

int iclr17_synthesis_deconv_igdn(const float* in, int B, int h, int w, int N,
                                 const float* w_packed, const float* bias, const float* beta_eff,
                                 const float* gamma_packed, float* out, float* pre_out,
                                 void* stream) {
  if (int rc = check_grid("deconv_igdn", B, h, w, N)) return rc;
  ICLR17_REQUIRE(in && w_packed && bias && beta_eff && gamma_packed && out, ICLR17_EINVAL,
                 "deconv_igdn: null pointer");
  EngineArgs a = zero_args();
  a.in = in; a.w = w_packed; a.bias = bias; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.out = out; a.pre = pre_out;
  a.B = B; a.Hin = h; a.Win = w;
  return launch_deconv5<EPI_IGDN>(a, N, S(stream));
}

int iclr17_output_partials_per_image(int H, int W) {
  return ((H / 4 + 7) / 8) * ((W / 4 + 7) / 8);
}

int iclr17_synthesis_deconv3(const float* in, int B, int H, int W, int N, const float* w_packed,
                             const float* bias, const float* x, float* clipped, float* recon,
                             double* sse_partial, int sse_unclipped, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in && w_packed && bias && clipped, ICLR17_EINVAL, "deconv3: null pointer");
  ICLR17_REQUIRE(x == nullptr || sse_partial != nullptr, ICLR17_EINVAL,
                 "deconv3: sse_partial required with x");
  ICLR17_REQUIRE(!sse_unclipped || recon != nullptr, ICLR17_EINVAL,
                 "deconv3: the unclipped SSE needs the recon output");
  EngineArgs a = zero_args();
  a.in = in; a.w = w_packed; a.bias = bias; a.out = clipped; a.recon = recon;
  a.xref = x; a.partial = sse_partial; a.sse_unclipped = sse_unclipped;
  a.B = B; a.Hin = H / 4; a.Win = W / 4;
  return launch_deconv3(a, N, S(stream));
}

// ------------------------------------------------------------------ x6 (bf16x6) precision mode
int iclr17_split_planes(const float* x, long n, uint16_t* planes, void* stream) {
  ICLR17_REQUIRE(x && planes && n > 0 && n % 8 == 0, ICLR17_EINVAL,
                 "split_planes: null pointer or n=%ld not a positive multiple of 8", n);
  const long n8 = n / 8;
  const int blocks = (int)((n8 + 255) / 256 < 4096 ? (n8 + 255) / 256 : 4096);
  hipLaunchKernelGGL(split_planes_kernel, dim3(blocks), dim3(256), 0, S(stream), x, n8,
                     (unsigned short*)planes, n);
  return check_launch("split_planes");
}

int iclr17_split_packed(const float* packed, int taps, int K, int N, uint16_t* planes,
                        void* stream) {
  ICLR17_REQUIRE(packed && planes && taps > 0 && K > 0 && K % 8 == 0 && N > 0, ICLR17_EINVAL,
                 "split_packed: bad arguments");
  const long n = (long)taps * (K / 8) * N;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(split_packed_kernel, dim3(blocks), dim3(256), 0, S(stream), packed, taps, K,
                     N, (unsigned short*)planes);
  return check_launch("split_packed");
}

int iclr17_analysis_conv1_gdn_x6(const float* x, int B, int H, int W, int N,
                                 const float* w_packed, const float* bias, const float* beta_eff,
                                 const float* gamma_packed, const uint16_t* gamma_split,
                                 float* out, uint16_t* out_split, float* pre_out, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(x && w_packed && bias && beta_eff && gamma_packed && (out || out_split),
                 ICLR17_EINVAL, "conv1_gdn_x6: null pointer");
  EngineArgs a = zero_args();
  a.in = x; a.w = w_packed; a.bias = bias; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.ggamma6 = gamma_split;
  a.out = out; a.pre = pre_out;
  a.out_split = out_split; a.out_plane = plane(B, H / 4, W / 4, N);
  a.B = B; a.Hin = H; a.Win = W;
  return launch_conv1<EPI_GDN>(a, N, S(stream));
}

int iclr17_analysis_conv1x6_gdn(const float* x, int B, int H, int W, int N,
                                const uint16_t* w_split, const float* bias, const float* beta_eff,
                                const uint16_t* gamma_split, float* out, uint16_t* out_split,
                                float* pre_out, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(x && w_split && bias && beta_eff && gamma_split && (out || out_split),
                 ICLR17_EINVAL, "conv1x6_gdn: null pointer");
  EngineArgs a = zero_args();
  a.in = x; a.w = (const float*)w_split; a.bias = bias; a.gbeta = beta_eff;
  a.ggamma6 = gamma_split;
  a.out = out; a.pre = pre_out;
  a.out_split = out_split; a.out_plane = plane(B, H / 4, W / 4, N);
  a.B = B; a.Hin = H; a.Win = W;
  return launch_conv1<EPI_GDN, W_SPLIT>(a, N, S(stream));
}

int iclr17_analysis_conv2_gdn_x6(const uint16_t* in_split, int B, int H, int W, int N,
                                 const float* w_packed, const float* bias, const float* beta_eff,
                                 const float* gamma_packed, const uint16_t* gamma_split,
                                 float* out, uint16_t* out_split, float* pre_out, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in_split && w_packed && bias && beta_eff && gamma_packed && gamma_split &&
                     (out || out_split),
                 ICLR17_EINVAL, "conv2_gdn_x6: null pointer");
  EngineArgs a = zero_args();
  a.w = w_packed; a.bias = bias; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.ggamma6 = gamma_split;
  a.out = out; a.pre = pre_out;
  a.in_split = in_split; a.in_plane = plane(B, H / 4, W / 4, N);
  a.out_split = out_split; a.out_plane = plane(B, H / 8, W / 8, N);
  a.B = B; a.Hin = H / 4; a.Win = W / 4;
  return launch_conv5<EPI_GDN>(a, N, S(stream));
}

// w_split: nullable; the weights pre-split by iclr17_split_packed(w_packed, 25, N, N)
static int conv3_quant_rate_x6(const char* what, const uint16_t* in_split, int B, int H, int W,
                               int N, const float* w_packed, const uint16_t* w_split,
                               int quant_mode, const float* noise, const float* rate_packed,
                               const float* rate_table, float* y_out, float* y_hat,
                               uint16_t* y_hat_split, double* bits_partial, void* stream) {
  ICLR17_REQUIRE(quant_mode == ICLR17_QUANT_ROUND || (quant_mode == ICLR17_QUANT_NOISE && noise),
                 ICLR17_EINVAL, "%s: bad quant mode %d / missing noise", what, quant_mode);
  EngineArgs a = zero_args();
  a.w = w_packed; a.out = y_out;
  a.w6 = w_split; a.w6_plane = w_split ? 25L * N * N : 0;
  a.qmode = quant_mode; a.noise = noise; a.rate = rate_packed; a.rtab = rate_table;
  a.yhat = y_hat; a.partial = bits_partial;
  a.in_split = in_split; a.in_plane = plane(B, H / 8, W / 8, N);
  a.out_split = y_hat_split; a.out_plane = plane(B, H / 16, W / 16, N);
  a.B = B; a.Hin = H / 8; a.Win = W / 8;
  return launch_conv5<EPI_QUANT>(a, N, S(stream));
}

int iclr17_analysis_conv3_quant_rate_x6(const uint16_t* in_split, int B, int H, int W, int N,
                                        const float* w_packed, int quant_mode, const float* noise,
                                        const float* rate_packed, const float* rate_table,
                                        float* y_out, float* y_hat, uint16_t* y_hat_split,
                                        double* bits_partial, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in_split && w_packed && rate_packed && y_hat && bits_partial,
                 ICLR17_EINVAL, "conv3_quant_rate_x6: null pointer");
  return conv3_quant_rate_x6("conv3_quant_rate_x6", in_split, B, H, W, N, w_packed, nullptr,
                             quant_mode, noise, rate_packed, rate_table, y_out, y_hat, y_hat_split,
                             bits_partial, stream);
}

int iclr17_analysis_conv3_quant_rate_x6w(const uint16_t* in_split, int B, int H, int W, int N,
                                         const float* w_packed, const uint16_t* w_split,
                                         int quant_mode, const float* noise,
                                         const float* rate_packed, const float* rate_table,
                                         float* y_out, float* y_hat, uint16_t* y_hat_split,
                                         double* bits_partial, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in_split && w_packed && w_split && rate_packed && y_hat && bits_partial,
                 ICLR17_EINVAL, "conv3_quant_rate_x6w: null pointer");
  return conv3_quant_rate_x6("conv3_quant_rate_x6w", in_split, B, H, W, N, w_packed, w_split,
                             quant_mode, noise, rate_packed, rate_table, y_out, y_hat, y_hat_split,
                             bits_partial, stream);
}

static int deconv_igdn_x6(const uint16_t* in_split, int B, int h, int w, int N,
                          const float* w_packed, const float* bias, const float* beta_eff,
                          const float* gamma_packed, const uint16_t* gamma_split, float* out,
                          uint16_t* out_split, float* pre_out, void* stream, int out_cm) {
  if (int rc = check_grid("deconv_igdn_x6", B, h, w, N)) return rc;
  ICLR17_REQUIRE(in_split && w_packed && bias && beta_eff && gamma_packed && gamma_split &&
                     (out || out_split),
                 ICLR17_EINVAL, "deconv_igdn_x6: null pointer");
  EngineArgs a = zero_args();
  a.w = w_packed; a.bias = bias; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.ggamma6 = gamma_split;
  a.out = out; a.pre = pre_out;
  a.in_split = in_split; a.in_plane = plane(B, h, w, N);
  a.out_split = out_split; a.out_plane = plane(B, 2 * h, 2 * w, N); a.out_cm = out_cm;
  a.B = B; a.Hin = h; a.Win = w;
  return launch_deconv5<EPI_IGDN>(a, N, S(stream));
}

int iclr17_synthesis_deconv_igdn_x6(const uint16_t* in_split, int B, int h, int w, int N,
                                    const float* w_packed, const float* bias,
                                    const float* beta_eff, const float* gamma_packed,
                                    const uint16_t* gamma_split, float* out, uint16_t* out_split,
                                    float* pre_out, void* stream) {
  return deconv_igdn_x6(in_split, B, h, w, N, w_packed, bias, beta_eff, gamma_packed, gamma_split,
                        out, out_split, pre_out, stream, 0);
}

int iclr17_synthesis_deconv_igdn_x6_cm(const uint16_t* in_split, int B, int h, int w, int N,
                                       const float* w_packed, const float* bias,
                                       const float* beta_eff, const float* gamma_packed,
                                       const uint16_t* gamma_split, float* out,
                                       uint16_t* out_split_cm, float* pre_out, void* stream) {
  return deconv_igdn_x6(in_split, B, h, w, N, w_packed, bias, beta_eff, gamma_packed, gamma_split,
                        out, out_split_cm, pre_out, stream, 1);
}

// ------------------------------------------------------------------ fused backward entry points
// Each takes its upstream gradient and writes the input gradient in fp32, as x6 planes, or both.
int iclr17_bwd_deconv3_igdn(const float* g_recon, int B, int H, int W, int N,
                            const float* w_packed, const uint16_t* w_split, const float* v_saved,
                            const float* beta_eff, const float* gamma_packed,
                            const float* gamma_packed_t,
                            const uint16_t* gamma_split, const uint16_t* gamma_t_split, float* g_v, uint16_t* g_v_split,
                            float* dn, float* colsum_gv, float* colsum_dn, void* stream) {
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(g_recon && (w_packed || w_split) && v_saved && beta_eff && gamma_packed &&
                     gamma_packed_t && (g_v || g_v_split) && dn, ICLR17_EINVAL, "bwd_deconv3_igdn: null pointer");
  EngineArgs a = zero_args();
  a.in = g_recon; a.gbeta = beta_eff; a.ggamma = gamma_packed; a.ggammaT = gamma_packed_t;
  a.ggamma6 = gamma_split; a.ggammaT6 = gamma_t_split;
  a.saved = v_saved; a.out = g_v; a.tout = dn; a.colsum_out = colsum_gv; a.colsum_t = colsum_dn;
  a.out_split = g_v_split; a.out_plane = plane(B, H / 4, W / 4, N);
  a.B = B; a.Hin = H; a.Win = W;
  if (w_split != nullptr) {   // the contraction in x6, on the split ICLR17_W_CONV1_X6 planes
    a.w = (const float*)w_split;
    return launch_conv1<EPI_IGDN_BWD, W_SPLIT>(a, N, S(stream));
  }
  a.w = w_packed;
  return launch_conv1<EPI_IGDN_BWD>(a, N, S(stream));
}

int iclr17_bwd_deconv_igdn(const float* g_v, const uint16_t* g_v_split, int B, int h, int w,
                           int N, const float* w_packed, const float* v_prev,
                           const float* beta_eff, const float* gamma_packed,
                           const float* gamma_packed_t,
                            const uint16_t* gamma_split, const uint16_t* gamma_t_split, float* g_v_prev, uint16_t* g_v_prev_split,
                           float* dn, float* colsum_gv, float* colsum_dn, void* stream) {
  if (int rc = check_grid("bwd_deconv_igdn", B, h, w, N)) return rc;
  ICLR17_REQUIRE((g_v || g_v_split) && w_packed && v_prev && beta_eff && gamma_packed &&
                     gamma_packed_t && (g_v_prev || g_v_prev_split) && dn, ICLR17_EINVAL,
                 "bwd_deconv_igdn: null pointer");
  EngineArgs a = zero_args();
  a.in = g_v; a.w = w_packed; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.ggammaT = gamma_packed_t; a.ggamma6 = gamma_split; a.ggammaT6 = gamma_t_split;
  a.saved = v_prev; a.out = g_v_prev; a.tout = dn;
  a.colsum_out = colsum_gv; a.colsum_t = colsum_dn;
  a.in_split = g_v_split; a.in_plane = plane(B, 2 * h, 2 * w, N);
  a.out_split = g_v_prev_split; a.out_plane = plane(B, h, w, N);
  a.B = B; a.Hin = 2 * h; a.Win = 2 * w;
  return launch_conv5<EPI_IGDN_BWD>(a, N, S(stream));
}

int iclr17_rate_bwd_partials(int h, int w) { return ((h + 7) / 8) * ((w + 7) / 8); }

/* Workgroups (= column-sum partial rows) per image of each fused backward kernel. */
int iclr17_bwd_tiles(int kind, int h, int w) {
  // kind 0: conv-type over an output grid h×w (bwd_deconv_igdn, bwd_deconv3_igdn: pass H/4, W/4)
  // kind 1: deconv-type over an input grid h×w (bwd_conv_gdn): 4 stride phases
  const int t = ((h + 7) / 8) * ((w + 7) / 8);
  return kind == 1 ? 4 * t : t;
}

int iclr17_bwd_deconv_rate(const float* g_v, const uint16_t* g_v_split, int B, int h, int w,
                           int N, const float* w_packed, const float* y_tilde,
                           const float* rate_packed, const float* g_bpp, float count, float* g_y,
                           uint16_t* g_y_split, float* rate_partial, void* stream) {
  if (int rc = check_grid("bwd_deconv_rate", B, h, w, N)) return rc;
  ICLR17_REQUIRE((g_v || g_v_split) && w_packed && g_y, ICLR17_EINVAL,
                 "bwd_deconv_rate: null pointer");
  ICLR17_REQUIRE(g_bpp == nullptr || (y_tilde && rate_packed && rate_partial && count > 0),
                 ICLR17_EINVAL, "bwd_deconv_rate: rate term needs y_tilde, rate params, partials");
  EngineArgs a = zero_args();
  a.in = g_v; a.w = w_packed; a.out = g_y;
  a.saved = y_tilde; a.rate = rate_packed; a.gscale = g_bpp; a.count = count;
  a.rpart = rate_partial;
  a.in_split = g_v_split; a.in_plane = plane(B, 2 * h, 2 * w, N);
  a.out_split = g_y_split; a.out_plane = plane(B, h, w, N);
  a.B = B; a.Hin = 2 * h; a.Win = 2 * w;
  return launch_conv5<EPI_RATE_BWD>(a, N, S(stream));
}

int iclr17_bwd_conv_gdn(const float* g_u, const uint16_t* g_u_split, int B, int h, int w, int N,
                        const float* w_packed, const float* u_prev, const float* beta_eff,
                        const float* gamma_packed, const float* gamma_packed_t,
                            const uint16_t* gamma_split, const uint16_t* gamma_t_split, float* g_u_prev,
                        uint16_t* g_u_prev_split, float* dn, float* colsum_gu, float* colsum_dn,
                        void* stream) {
  if (int rc = check_grid("bwd_conv_gdn", B, h, w, N)) return rc;
  ICLR17_REQUIRE((g_u || g_u_split) && w_packed && u_prev && beta_eff && gamma_packed &&
                     gamma_packed_t && (g_u_prev || g_u_prev_split) && dn, ICLR17_EINVAL, "bwd_conv_gdn: null pointer");
  EngineArgs a = zero_args();
  a.in = g_u; a.w = w_packed; a.gbeta = beta_eff; a.ggamma = gamma_packed;
  a.ggammaT = gamma_packed_t; a.ggamma6 = gamma_split; a.ggammaT6 = gamma_t_split;
  a.saved = u_prev; a.out = g_u_prev; a.tout = dn;
  a.colsum_out = colsum_gu; a.colsum_t = colsum_dn;
  a.in_split = g_u_split; a.in_plane = plane(B, h, w, N);
  a.out_split = g_u_prev_split; a.out_plane = plane(B, 2 * h, 2 * w, N);
  a.B = B; a.Hin = h; a.Win = w;
  return launch_deconv5<EPI_GDN_BWD>(a, N, S(stream));
}

// ------------------------------------------------------------------ stand-alone GDN / IGDN
int iclr17_gdn_bwd(const float* x, const float* g, int B, int C, int H, int W, int layout,
                   int inverse, const float* beta_eff, const float* gamma_packed,
                   const float* gamma_packed_t, float* dx, float* dn, float* u_nhwc,
                   void* stream) {
  ICLR17_REQUIRE(B > 0 && H > 0 && W > 0, ICLR17_EINVAL, "gdn_bwd: bad shape");
  ICLR17_REQUIRE(C == 128 || C == 192, ICLR17_EUNSUPPORTED, "gdn_bwd: C=%d unsupported (128, 192)", C);
  ICLR17_REQUIRE(layout == ICLR17_LAYOUT_NCHW || layout == ICLR17_LAYOUT_NHWC, ICLR17_EINVAL,
                 "gdn_bwd: bad layout %d", layout);
  ICLR17_REQUIRE(x && g && beta_eff && gamma_packed && gamma_packed_t && dx && dn, ICLR17_EINVAL,
                 "gdn_bwd: null pointer");
  const int HW = H * W;
  const dim3 grid(B * ((HW + BM - 1) / BM));
  with_N(C, [&](auto c) { return with_bool(inverse, [&](auto inv) {
    return with_bool(layout == ICLR17_LAYOUT_NHWC, [&](auto nhwc) {
      hipLaunchKernelGGL((gdn_bwd_kernel<decltype(c)::value, decltype(inv)::value, decltype(nhwc)::value>),
                         grid, dim3(256), 0, S(stream), x, g, HW, beta_eff, gamma_packed,
                         gamma_packed_t, dx, dn, u_nhwc);
      return 0;
    }); }); });
  return check_launch("gdn_bwd");
}

int iclr17_gdn(const float* x, int B, int C, int H, int W, int layout, int inverse,
               const float* beta_eff, const float* gamma_packed, float* y, void* stream) {
  ICLR17_REQUIRE(B > 0 && H > 0 && W > 0, ICLR17_EINVAL, "gdn: bad shape");
  ICLR17_REQUIRE(C == 128 || C == 192, ICLR17_EUNSUPPORTED, "gdn: C=%d unsupported (128, 192)", C);
  ICLR17_REQUIRE(layout == ICLR17_LAYOUT_NCHW || layout == ICLR17_LAYOUT_NHWC, ICLR17_EINVAL,
                 "gdn: bad layout %d", layout);
  ICLR17_REQUIRE(x && beta_eff && gamma_packed && y, ICLR17_EINVAL, "gdn: null pointer");
  const int HW = H * W;
  const dim3 grid(B * ((HW + BM - 1) / BM));
  with_N(C, [&](auto c) { return with_bool(inverse, [&](auto inv) {
    return with_bool(layout == ICLR17_LAYOUT_NHWC, [&](auto nhwc) {
      hipLaunchKernelGGL((gdn_kernel<decltype(c)::value, decltype(inv)::value, decltype(nhwc)::value>),
                         grid, dim3(256), 0, S(stream), x, HW, beta_eff, gamma_packed, y);
      return 0;
    }); }); });
  return check_launch("gdn");
}

}  // extern "C"
