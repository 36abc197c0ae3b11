// deconv3 halo kernels (gfx950): the synthesis transform's last layer (ConvTranspose2d(N, 3, 9, s4,
// p4, op3) + clamp) on a 16×16 base block whose 18×18 input patch is staged once per 32-channel
// chunk, for the three operand forms that share the scheme and its D3_* layout:
//   x6    deconv3_x6_kernel<CI>         three bf16 planes, six part products per MAC
//   h3    deconv3_x6_kernel<CI, true>   two fp16 planes, three part products (the default chain's
//                                       last kernel; the rest of that chain is engine_h3.hip)
//   bf16  deconv3_bf16_kernel<CI>       one bf16 product per MAC (the rest: engine_bf16.hip)
// The fp32 deconv3 is an instantiation of the 8×8-tile engine (engine_fp32.hip).
#include "engine.h"

namespace iclr17 {

// --------------------------------------------------------------- deconv3, x6 halo kernel
// synthesis_17.py:23 deconv3 (ConvTranspose2d(N, 3, 9, s4, p4, op3)) + model.py:59 clamp, on the
// x6 activation format. The all-phase GEMM of the engine (M = base pixels, N = 48 = 3 channels ×
// 16 output phases, K = 9 taps × CI) with two changes that cut the bytes staged per MFMA:
//   - a 16×16 base block per workgroup (M = 256; each wave 64 rows = 4 base rows × 16), so one
//     6 KB weight stage feeds 4× the pixels of the 8×8 engine tile;
//   - per 32-channel chunk, the 18×18 input patch (the block plus its 3×3 halo) is staged ONCE
//     in LDS (three bf16 planes, 62 KB) and the 9 taps read shifted windows of it, instead of
//     DMA-ing each tap's 64 rows again (324 vs 9·256 staged pixels).
// Patch layout: slot = plane·324 + p (p = r·18 + c), 64 bytes per slot; 16-byte piece g of slot
// p sits at g ^ 2·((p >> 2) & 1), conflict-free for ds_read_b128 lane groups at every window
// offset (checked exhaustively). One A stage (single-buffered: the chunk boundary is a
// barrier-bounded refill the co-resident workgroup covers) + two 6 KB B stages = 73 KB, two
// workgroups per CU. Epilogue: bias, clamp, 64×64 output block through LDS, per-8×8-quadrant SSE
// partials in the engine's partial layout (iclr17_output_partials_per_image).
constexpr int D3_BS = 16;                       // base block side
constexpr int D3_PS = D3_BS + 2;                // patch side
constexpr int D3_PPX = D3_PS * D3_PS;           // 324 patch pixels per plane
constexpr int D3_NAI = (3 * D3_PPX + 15) / 16;  // 61 A wave-instructions per chunk
constexpr int D3_SA = D3_NAI * 256;             // A stage floats (976 slots × 16)
constexpr int D3_SB6 = 3 * 32 * 48 / 2;         // x6 B stage floats: [3 planes][4 k8][48][8] u16
constexpr int D3_LDS = D3_SA + 2 * D3_SB6;      // 80,896 B: two workgroups per CU
// deconv3 epilogue tile [3][64][64] fp32 (channel, output row, output column): row stride D3_ES,
// channel stride D3_EC floats. A write instruction's 16 lanes of a group hold 16 (channel, ry, rx)
// columns of one base pixel (d3_col order) and the lane groups base columns 16 floats apart; the
// earlier [3][64][65] tile put those columns on ≈5 banks (6.7 LDS cycles per 32-lane group, 88 %
// of the kernel's bank-conflict cycles); rows of 67 and channels of 64·67 + 11 floats spread them
// (1.7 cycles, the best of the strides 64..99 × 64·stride + 0..39), and the store phase's reads
// (8 columns × 4 rows per group) stay conflict-free.
constexpr int D3_ES = 67, D3_EC = 64 * D3_ES + 11;

// first weight block (tile-tap) of tap t in the compact per-chunk weight stage: taps 0-2 touch
// one column tile, taps 3 and 6 two, the others three (see d3_col)
__host__ __device__ constexpr int d3_boff(int t) {
  return t <= 3 ? t : (t == 4 ? 5 : (t == 5 ? 8 : (t == 6 ? 11 : (t == 7 ? 13 : (t == 8 ? 16 : 19)))));
}

// Column order of the in-loop-split path: logical column j (tile j / 16, lane j % 16) reads packed
// column co·16 + ry·4 + rx, taking first the 12 columns with ry = 0, then the 9 with rx = 0 < ry,
// then the rest, each (ry, rx, co)-lexicographic. A tap with dy = −1 feeds only phase ry = 0 and
// one with dx = −1 only rx = 0 (the packed weights are zero elsewhere), so with this order the
// three dy = −1 taps need tile 0 alone and the two other dx = −1 taps tiles 0–1: 19 tile-taps
// per chunk instead of 27. The skipped products are exact zeros, so results are unchanged.
__device__ __forceinline__ int d3_col(int j) {
  int ry, rx, co;
  if (j < 12) {          // ry = 0
    ry = 0; rx = j / 3; co = j % 3;
  } else if (j < 21) {   // rx = 0 < ry
    ry = 1 + (j - 12) / 3; rx = 0; co = (j - 12) % 3;
  } else {
    const int k = j - 21;
    ry = 1 + k / 9; rx = 1 + (k / 3) % 3; co = k % 3;
  }
  return co * 16 + ry * 4 + rx;
}

// H3: the input in the h3 form (two fp16 planes, chunk-major from the h3 deconv2) and the
// weights as iclr17_split_packed_h3's two planes; three v_mfma_f32_16x16x32_f16 per tile and tap
// (lo_a·hi_w, hi_a·lo_w, hi_a·(hi_w·2¹¹)) instead of six bf16 ones, scaled back exactly before
// the bias. Two thirds of the x6 stage bytes per step (41 A and 6 / 4 B pieces).
template <int CI, bool H3 = false>
__global__ void __launch_bounds__(256, 2) deconv3_x6_kernel(const EngineArgs a) {
  constexpr int KCH = 32, NCH = CI / KCH;
  constexpr int MT = 4, NT = 3;
  constexpr int NPL = H3 ? 2 : 3;                         // input (and weight) planes
  // A wave-instructions per chunk (x6: 61; h3: 41, rounded up to whole rounds of the 4 waves:
  // the 41-piece form hit a compiler fault, "Operand has incorrect register class"; the three
  // padding pieces load the zero line)
  constexpr int NAI = H3 ? ((NPL * D3_PPX + 15) / 16 + 3) / 4 * 4 : (NPL * D3_PPX + 15) / 16;
  constexpr int AI_W = (NAI + 3) / 4;   // x6: 16 (wave 0..3 takes i = w + 4j, i < 61)
  static_assert(3 * D3_EC <= D3_LDS, "epilogue block fits the stages");
  __shared__ __attribute__((aligned(16))) float smem[D3_LDS];
  // H3: the range flag of the chain (set by an upstream h3 kernel whose output did not fit the
  // form, |x| ≥ 2²²) makes every result of this last kernel NaN — the reconstruction, the SSE
  // partials and the folded bit totals — so an out-of-range input can never pass for a result.
  // The upstream kernels all completed before this launch, so the flag is final here.
  const bool poison = H3 && a.range != nullptr && *(const volatile int*)a.range != 0;
  if (a.fold_partial != nullptr && blockIdx.x == 0) fold_bits<256>(a, (double*)smem, poison);
  float* const sA = smem;
  float* const sB = smem + D3_SA;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int b = bid / a.tiles_y;

  // A DMA sources: per instruction j of this wave, slot q = 16i + lane/4 (plane, patch pixel),
  // physical piece lane & 3 ← logical piece (lane & 3) ^ swizzle(p). -1: zero line.
  int asrc[AI_W];
#pragma unroll
  for (int j = 0; j < AI_W; ++j) {
    const int i = wave + 4 * j;
    const int q = i * 16 + (lane >> 2);
    const int pl = q / D3_PPX, p = q - pl * D3_PPX;
    const int r = p / D3_PS, c = p - r * D3_PS;
    const int iy = ty * D3_BS - 1 + r, ix = tx * D3_BS - 1 + c;
    const bool ok = i < NAI && pl < NPL && (unsigned)iy < (unsigned)a.Hin &&
                    (unsigned)ix < (unsigned)a.Win;
    const int g = (lane & 3) ^ (((p >> 2) & 1) << 1);
    // pixel stride: CI (NHWC planes) or 32 (chunk-major planes, a.in_cm)
    asrc[j] = ok ? (iy * a.Win + ix) * (a.in_cm ? KCH : CI) + g * 8 : -1;
  }
  const unsigned short* __restrict__ inb = a.in_split + (long)b * a.Hin * a.Win * CI;
  const long cstride = a.in_cm ? (long)a.Hin * a.Win * KCH : KCH;   // chunk stride (elements)
  auto issue_a = [&](int cc) {
#pragma unroll
    for (int j = 0; j < AI_W; ++j) {
      const int i = wave + 4 * j;
      if (i < NAI) {
        const int q = i * 16 + (lane >> 2);
        const int pl = q / D3_PPX;
        const unsigned short* src = inb + (long)(pl < NPL ? pl : 0) * a.in_plane + asrc[j] + cc * cstride;
        glds16(asrc[j] >= 0 ? (const float*)src : g_zero16, sA + i * 256);
      }
    }
  };
  // B DMA: the weights arrive pre-split (iclr17_split_packed of the ICLR17_W_DECONV9 packing:
  // [3][9][CI/8][48][8] bf16), so no wave splits them in the loop. A tap stages only the column
  // tiles it touches (the others hold exact zeros for it, see d3_col): tap t's block is
  // [plane 3][k8 4][16·ntt(t)][8], slot = logical column (the d3_col order the fragment reads
  // walk), so a 16-lane group reads 16 consecutive 16-byte slots (conflict-free). The three
  // one-tile taps (dy = −1) share one step: 7 steps of 9 / 6 / 9 / 9 / 6 / 9 / 9 KB per chunk
  // instead of 9 of 9 KB, 57 DMA pieces instead of 81 and 7 barriers instead of 9.
  const unsigned short* __restrict__ w6 = (const unsigned short*)a.w;
  constexpr long WPL = 9L * CI * 48;   // u16 per weight plane
  // taps of step st: st = 0 → taps 0, 1, 2; else tap st + 2
  auto issue_b = [&](int cc, int st, int buf) {
    float* sb = sB + buf * D3_SB6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int piece = wave + 4 * k;
      if (piece >= 3 * NPL || ((st == 1 || st == 4) && piece >= 2 * NPL)) break;   // wave-uniform
      const int slot = piece * 64 + lane;
      int tap, pl, k8, col;
      if (st == 0) {
        tap = slot / (64 * NPL);
        const int r = slot - tap * 64 * NPL;
        pl = r / 64; k8 = (r >> 4) & 3; col = r & 15;
      } else {
        tap = st + 2;
        const int nc = st == 1 || st == 4 ? 32 : 48;   // 16·ntt
        pl = slot / (4 * nc);
        const int r = slot - pl * 4 * nc;
        k8 = r / nc; col = r - k8 * nc;
      }
      const unsigned short* src =
          w6 + pl * WPL + (((long)tap * (CI / 8) + cc * 4 + k8) * 48 + d3_col(col)) * 8;
      glds16((const float*)src, sb + piece * 256);
    }
  };

  f4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4;
  const int prow = (4 * wave + 1) * D3_PS + 1 + (lane & 15);   // window origin for mt = 0
  int pcol[NT];   // packed column of this lane in tile nt
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
    pcol[nt] = d3_col(nt * 16 + (lane & 15));

  // tap `tap` from its block at u16 offset `boff` of stage buf: [plane][k8][16·NTT][8]
  auto compute = [&](int buf, int tap, int boff, auto ntt) {
    X6Acc st;
    constexpr int NTT = decltype(ntt)::value;   // tiles this tap touches
    constexpr int NC = 16 * NTT;
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    const unsigned short* sb = (const unsigned short*)(sB + buf * D3_SB6) + boff + g * NC * 8;
    if constexpr (H3) {
      u4 Bh[NTT], Bl[NTT], Bh11[NTT];
#pragma unroll
      for (int nt = 0; nt < NTT; ++nt) {
        const int jc = nt * 16 + (lane & 15);
        Bh[nt] = *(const u4*)(sb + jc * 8);
        Bl[nt] = *(const u4*)(sb + 4 * NC * 8 + jc * 8);
        Bh11[nt] = h3_x2048(Bh[nt]);
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int p = prow + (mt + dy) * D3_PS + dx;
        const unsigned short* sa =
            (const unsigned short*)(sA + p * 16 + ((g ^ (((p >> 2) & 1) << 1)) * 4));
        const h8v Ah = __builtin_bit_cast(h8v, *(const u4*)(sa));
        const h8v Al = __builtin_bit_cast(h8v, *(const u4*)(sa + D3_PPX * 32));
#pragma unroll
        for (int nt = 0; nt < NTT; ++nt) {
          f4 c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, __builtin_bit_cast(h8v, Bh[nt]), acc[mt][nt], 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, __builtin_bit_cast(h8v, Bl[nt]), c, 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, __builtin_bit_cast(h8v, Bh11[nt]), c, 0, 0, 0);
        }
      }
    } else {
    bf8 Bh[NTT], Bm[NTT], Bl[NTT];
#pragma unroll
    for (int nt = 0; nt < NTT; ++nt) {
      const int jc = nt * 16 + (lane & 15);
      Bh[nt] = __builtin_bit_cast(bf8, *(const u4*)(sb + jc * 8));
      Bm[nt] = __builtin_bit_cast(bf8, *(const u4*)(sb + 4 * NC * 8 + jc * 8));
      Bl[nt] = __builtin_bit_cast(bf8, *(const u4*)(sb + 8 * NC * 8 + jc * 8));
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int p = prow + (mt + dy) * D3_PS + dx;
      const unsigned short* sa =
          (const unsigned short*)(sA + p * 16 + ((g ^ (((p >> 2) & 1) << 1)) * 4));
      const bf8 Ah = __builtin_bit_cast(bf8, *(const u4*)(sa));
      const bf8 Am = __builtin_bit_cast(bf8, *(const u4*)(sa + D3_PPX * 32));
      const bf8 Al = __builtin_bit_cast(bf8, *(const u4*)(sa + 2 * D3_PPX * 32));
#pragma unroll
      for (int nt = 0; nt < NTT; ++nt) {
        mfma_x6<false>(acc, st, mt, nt, Ah, Am, Al, Bh[nt], Bm[nt], Bl[nt]);
      }
    }
    x6_flush<false>(acc, st);
    }
  };

  issue_a(0);
  issue_b(0, 0, 0);
  // steps unrolled inside the chunk loop: each tap's code is specialised (no joins between the
  // three tile counts, whose register shuffles cost more VALU than the split itself). The
  // accumulation order (chunk, tap 0..8) is that of the per-tap schedule.
  for (int cc = 0; cc < NCH; ++cc) {
#pragma unroll
    for (int st = 0; st < 7; ++st) {
      const int s = cc * 7 + st;
      dma_barrier();   // A (at a chunk start) and B of step s landed
      if (st != 6) issue_b(cc, st + 1, (s + 1) & 1);
      if (st == 0) {
        compute(s & 1, 0, 0, std::integral_constant<int, 1>{});
        compute(s & 1, 1, 64 * NPL * 8, std::integral_constant<int, 1>{});
        compute(s & 1, 2, 2 * 64 * NPL * 8, std::integral_constant<int, 1>{});
      } else if (st == 1 || st == 4) {
        compute(s & 1, st + 2, 0, std::integral_constant<int, 2>{});
      } else {
        compute(s & 1, st + 2, 0, std::integral_constant<int, 3>{});
      }
      if (st == 6 && cc + 1 < NCH) {
        __syncthreads();   // every wave is done with this chunk's patch
        issue_a(cc + 1);
        issue_b(cc + 1, 0, (s + 1) & 1);
      }
    }
  }
  __syncthreads();     // stage reads done before the epilogue reuses LDS
  if constexpr (H3) {   // 2¹¹·σ_a·σ_w off, exactly
    const float dsc = a.wscale[1];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = acc[mt][nt] * dsc;
  }

  // epilogue: column n = co·16 + ry·4 + rx of row m = (by, bx) → output (4by + ry, 4bx + rx)
  constexpr int OS = 4 * D3_BS;
  float* sO = smem;   // [3][64][64], strides D3_EC / D3_ES
  const int H = a.Hout, W = a.Wout;
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
          const int by = 4 * wave + mt, bx = 4 * g + r;
          const int co = pcol[nt] >> 4, ph = pcol[nt] & 15;
          float v = acc[mt][nt][r] + a.bias[co];
          if (pass == 0) v = fminf(fmaxf(v, 0.0f), 1.0f);
          if (poison) v = __builtin_nanf("");
          sO[co * D3_EC + (by * 4 + (ph >> 2)) * D3_ES + bx * 4 + (ph & 3)] = v;
        }
    __syncthreads();
    // wave w stores output quadrant (qy, qx) = (w >> 1, w & 1): 3 × 32 rows × 8 float4
    const int qy = wave >> 1, qx = wave & 1;
    const bool sse_pass = pass == (a.sse_unclipped ? 1 : 0) && a.xref != nullptr;
    for (int k = lane; k < 3 * 32 * 8; k += 64) {
      const int c4 = k & 7, row = (k >> 3) & 31, co = k >> 8;
      const int oyl = qy * 32 + row, oxl = qx * 32 + c4 * 4;
      const int oy = ty * OS + oyl, ox = tx * OS + oxl;
      if (oy >= H || ox >= W) continue;
      const float* sp = sO + co * D3_EC + oyl * D3_ES + oxl;
      const f4 v = f4{sp[0], sp[1], sp[2], sp[3]};
      const long off = (((long)b * 3 + co) * H + oy) * W + ox;
      *(f4*)(dst + off) = v;
      if (sse_pass) {
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
    const int ty8 = 2 * ty + (wave >> 1), tx8 = 2 * tx + (wave & 1);
    const int tiles_x8 = (a.gw + 7) / 8;
    if (lane == 0 && ty8 * 8 < a.gh && tx8 * 8 < a.gw)
      a.partial[(long)b * a.partials_per_image + ty8 * tiles_x8 + tx8] = (double)sse;
  }
}

// ------------------------------------------------------------ deconv3 in the bf16 mode
// synthesis_17.py:23-25 + model.py:59 on a bf16 NHWC input: the all-phase GEMM of
// deconv3_x6_kernel (48 columns = 16 output phases × 3 channels, d3_col order, dy = −1 / dx = −1
// taps on the tiles that hold their non-zero weights) with one bf16 product per MAC, but all 9
// taps of a 32-channel chunk per barrier: the chunk's 18×18 patch and its 9 weight slices are
// double-buffered by LDS-DMA (153 KB, one workgroup of 8 waves per CU), so a chunk costs one
// barrier instead of nine. Wave w owns base rows 2w, 2w+1. The accumulation order (chunk, tap)
// and the operands (weights rounded to bf16 in the loop, one bf16 product per MAC) are those of the
// per-tap bf16 kernel this replaces, so the results are bit-identical to it.
template <int CI>
__global__ void __launch_bounds__(512) deconv3_bf16_kernel(const EngineArgs a) {
  constexpr int KCH = 32, NCH = CI / KCH, MT = 2, NT = 3, NW = 8;
  constexpr int NAI = (D3_PPX + 15) / 16;   // 21 patch wave-instructions per chunk (16 px each)
  constexpr int SA = NAI * 256;             // patch buffer floats
  constexpr int NBI = 19;                   // weight blocks per chunk: the 19 tile-taps
  constexpr int PB = NBI * 256;             // weight floats per chunk: [block][k8 4][16][8] bf16
  constexpr int KA = (NAI + NW - 1) / NW, KB = (NBI + NW - 1) / NW;
  constexpr int LDS = 2 * SA + 2 * PB;
  static_assert(3 * D3_EC + 16 <= LDS, "epilogue block fits");
  __shared__ __attribute__((aligned(16))) float smem[LDS];
  if (a.fold_partial != nullptr && blockIdx.x == 0) fold_bits<512>(a, (double*)smem);
  float* const sA = smem;
  float* const sB = smem + 2 * SA;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  const int b = bid / a.tiles_y;

  // patch DMA: instruction i, slot q = 16i + lane/4 (patch pixel), physical piece lane & 3 ←
  // logical piece (lane & 3) ^ swizzle(q); -1: zero line
  int asrc[KA];
#pragma unroll
  for (int j = 0; j < KA; ++j) {
    const int i = wave + NW * j;
    const int p = i * 16 + (lane >> 2);
    const int r = p / D3_PS, c = p - r * D3_PS;
    const int iy = ty * D3_BS - 1 + r, ix = tx * D3_BS - 1 + c;
    const bool ok = i < NAI && p < D3_PPX && (unsigned)iy < (unsigned)a.Hin &&
                    (unsigned)ix < (unsigned)a.Win;
    const int g = (lane & 3) ^ (((p >> 2) & 1) << 1);
    asrc[j] = ok ? (iy * a.Win + ix) * CI + g * 8 : -1;
  }
  // weight DMA (iclr17_round_packed of the ICLR17_W_DECONV9 packing: [9][CI/8][48][8] bf16): only
  // the column tiles a tap touches (d3_col; the others are exact zeros for it), one 1 KB block
  // [k8 4][16][8] per tile-tap, taps in order (1, 1, 1, 2, 3, 3, 2, 3, 3 tiles): 19 KB per chunk
  // instead of 27. Instruction i = block i, slot (k8, c) ← packed (cc·4 + k8, d3_col(16·tt + c)).
  int bsrc[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    const int i = wave + NW * j;
    int t = 0;
    while (t < 8 && d3_boff(t + 1) <= i) ++t;
    const int tt = i - d3_boff(t), k8 = lane >> 4, c = lane & 15;
    bsrc[j] = ((t * (CI / 8) + k8) * 48 + d3_col(16 * tt + c)) * 8;
  }
  const unsigned short* __restrict__ wb = (const unsigned short*)a.w;
  const unsigned short* __restrict__ inb = a.in_split + (long)b * a.Hin * a.Win * CI;
  auto issue = [&](int cc, int buf) {
#pragma unroll
    for (int j = 0; j < KA; ++j) {
      const int i = wave + NW * j;
      if (i < NAI)
        glds16(asrc[j] >= 0 ? (const float*)(inb + asrc[j] + cc * KCH) : g_zero16,
               sA + buf * SA + i * 256);
    }
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      const int i = wave + NW * j;
      if (i < NBI) glds16((const float*)(wb + cc * 4 * 48 * 8 + bsrc[j]), sB + buf * PB + i * 256);
    }
  };

  f4 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f4{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4;
  const int prow = (2 * wave + 1) * D3_PS + 1 + (lane & 15);   // window origin for mt = 0
  auto compute = [&](int buf, int tap, auto ntt) {
    constexpr int NTT = decltype(ntt)::value;   // tiles this tap touches
    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
    const u4* sb = (const u4*)(sB + buf * PB + d3_boff(tap) * 256) + g * 16 + (lane & 15);
    bf8 Bb[NTT];
#pragma unroll
    for (int nt = 0; nt < NTT; ++nt) Bb[nt] = __builtin_bit_cast(bf8, sb[nt * 64]);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int p = prow + (mt + dy) * D3_PS + dx;
      const unsigned short* sa =
          (const unsigned short*)(sA + buf * SA + p * 16 + ((g ^ (((p >> 2) & 1) << 1)) * 4));
      const bf8 Ab = __builtin_bit_cast(bf8, *(const u4*)(sa));
#pragma unroll
      for (int nt = 0; nt < NTT; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ab, Bb[nt], acc[mt][nt], 0, 0, 0);
    }
  };

  issue(0, 0);
  for (int cc = 0; cc < NCH; ++cc) {
    dma_barrier();   // chunk cc landed; buffer (cc+1)&1 is free
    if (cc + 1 < NCH) issue(cc + 1, (cc + 1) & 1);
    const int buf = cc & 1;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (tap < 3)
        compute(buf, tap, std::integral_constant<int, 1>{});
      else if (tap == 3 || tap == 6)
        compute(buf, tap, std::integral_constant<int, 2>{});
      else
        compute(buf, tap, std::integral_constant<int, 3>{});
    }
  }
  __syncthreads();     // stage reads done before the epilogue reuses LDS

  // epilogue: column n = co·16 + ry·4 + rx of row m = (by, bx) → output (4by + ry, 4bx + rx);
  // the waves 2q, 2q+1 store output quadrant q's upper / lower 16 rows
  constexpr int OS = 4 * D3_BS;
  float* sO = smem;   // [3][64][64], strides D3_EC / D3_ES
  float* red = smem + 3 * D3_EC;
  const int H = a.Hout, W = a.Wout;
  float sse = 0.f;
  int pcol[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) pcol[nt] = d3_col(nt * 16 + (lane & 15));
  const int q = wave >> 1, hf = wave & 1, qy = q >> 1, qx = q & 1;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1 && a.recon == nullptr) break;
    float* dst = pass == 0 ? a.out : a.recon;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int by = 2 * wave + mt, bx = 4 * g + r;
          const int co = pcol[nt] >> 4, ph = pcol[nt] & 15;
          float v = acc[mt][nt][r] + a.bias[co];
          if (pass == 0) v = fminf(fmaxf(v, 0.0f), 1.0f);
          sO[co * D3_EC + (by * 4 + (ph >> 2)) * D3_ES + bx * 4 + (ph & 3)] = v;
        }
    __syncthreads();
    const bool sse_pass = pass == (a.sse_unclipped ? 1 : 0) && a.xref != nullptr;
    for (int k = lane; k < 3 * 16 * 8; k += 64) {
      const int c4 = k & 7, row = (k >> 3) & 15, co = k >> 7;
      const int oyl = qy * 32 + hf * 16 + row, oxl = qx * 32 + c4 * 4;
      const int oy = ty * OS + oyl, ox = tx * OS + oxl;
      if (oy >= H || ox >= W) continue;
      const float* sp = sO + co * D3_EC + oyl * D3_ES + oxl;
      const f4 v = f4{sp[0], sp[1], sp[2], sp[3]};
      const long off = (((long)b * 3 + co) * H + oy) * W + ox;
      *(f4*)(dst + off) = v;
      if (sse_pass) {
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
    if (lane == 0) red[wave] = sse;
    __syncthreads();
    const int ty8 = 2 * ty + qy, tx8 = 2 * tx + qx;
    const int tiles_x8 = (a.gw + 7) / 8;
    if (hf == 0 && lane == 0 && ty8 * 8 < a.gh && tx8 * 8 < a.gw)
      a.partial[(long)b * a.partials_per_image + ty8 * tiles_x8 + tx8] =
          (double)(red[wave] + red[wave + 1]);
  }
}

// ====================================================================================== host
namespace {

// conv3's bit partials [B][T], reduced inside the kernel (fold_bits)
struct FoldBits {
  const double* partial;
  int T;
  double* per_image;
  float* total;
  double scale;
};

// What distinguishes the six entry points: the operand form, the input layout and the optional
// bits fold. w is iclr17_split_packed(9, N, 48) of the ICLR17_W_DECONV9 packing (x6),
// iclr17_split_packed_h3's planes (h3) or iclr17_round_packed(9, N, 48) (bf16).
enum D3Form { D3_X6, D3_H3, D3_BF16 };
struct HaloForm {                   // {form, in_cm, fold, range}
  D3Form form;
  int in_cm = 0;                    // input in the chunk-major split form
  const FoldBits* fold = nullptr;
  const int* range = nullptr;       // h3: the chain's range flag (read only, the poison check)
};

int launch_deconv3_halo(const HaloForm& f, const uint16_t* in, int B, int H, int W, int N,
                        const void* w, const float* bias, const float* x, float* clipped,
                        float* recon, double* sse_partial, int sse_unclipped, void* stream) {
  const char* what = f.form == D3_BF16 ? "deconv3_bf16" : (f.form == D3_H3 ? "deconv3_h3" : "deconv3_x6");
  if (int rc = check_image(B, H, W, N)) return rc;
  ICLR17_REQUIRE(in && w && bias && clipped, ICLR17_EINVAL, "%s: null pointer", what);
  ICLR17_REQUIRE(x == nullptr || sse_partial != nullptr, ICLR17_EINVAL,
                 "%s: sse_partial required with x", what);
  ICLR17_REQUIRE(!sse_unclipped || recon != nullptr, ICLR17_EINVAL,
                 "%s: the unclipped SSE needs the recon output", what);
  EngineArgs a = zero_args();
  a.sse_unclipped = sse_unclipped;
  a.in_split = (const unsigned short*)in;
  a.in_cm = f.in_cm;
  a.w = (const float*)w; a.bias = bias; a.out = clipped; a.recon = recon; a.xref = x;
  a.partial = sse_partial;
  a.B = B; a.Hin = H / 4; a.Win = W / 4; a.Hout = H; a.Wout = W;
  a.gh = H / 4; a.gw = W / 4;
  a.in_plane = (long)B * a.Hin * a.Win * N;
  a.tiles_y = (a.gh + D3_BS - 1) / D3_BS; a.tiles_x = (a.gw + D3_BS - 1) / D3_BS;
  a.partials_per_image = ((a.gh + 7) / 8) * ((a.gw + 7) / 8);
  if (f.fold != nullptr) {
    ICLR17_REQUIRE(f.fold->partial && f.fold->T > 0 && f.fold->total, ICLR17_EINVAL,
                   "%s: bits fold needs the partials, their count and a total", what);
    a.fold_partial = f.fold->partial; a.fold_T = f.fold->T; a.fold_per_image = f.fold->per_image;
    a.fold_total = f.fold->total; a.fold_scale = f.fold->scale;
  }
  if (f.form == D3_H3) {
    a.wscale = (const float*)((const uint16_t*)w + 2L * 9 * N * 48);
    a.range = const_cast<int*>(f.range);
  }
  const dim3 grid(a.tiles_x * a.tiles_y * B);
  const hipStream_t st = S(stream);
  with_N(N, [&](auto n) {
    constexpr int CN = decltype(n)::value;
    if (f.form == D3_BF16)
      hipLaunchKernelGGL((deconv3_bf16_kernel<CN>), grid, dim3(512), 0, st, a);
    else if (f.form == D3_H3)
      hipLaunchKernelGGL((deconv3_x6_kernel<CN, true>), grid, dim3(256), 0, st, a);
    else
      hipLaunchKernelGGL((deconv3_x6_kernel<CN>), grid, dim3(256), 0, st, a);
    return 0;
  });
  return check_launch(what);
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_synthesis_deconv3_h3(const uint16_t* in_h3_cm, int B, int H, int W, int N,
                                const uint16_t* w_h3, const float* bias, const float* x,
                                float* clipped, float* recon, double* sse_partial,
                                int sse_unclipped, const double* bits_partial, int bits_T,
                                double* bits_per_image, float* bpp_total, double bits_scale,
                                const int* range_flag, void* stream) {
  const FoldBits fold = {bits_partial, bits_T, bits_per_image, bpp_total, bits_scale};
  const HaloForm f = {D3_H3, 1, bits_partial ? &fold : nullptr, range_flag};
  return launch_deconv3_halo(f, in_h3_cm, B, H, W, N, w_h3, bias, x, clipped, recon, sse_partial,
                             sse_unclipped, stream);
}

int iclr17_synthesis_deconv3_x6(const uint16_t* in_split, int B, int H, int W, int N,
                                const uint16_t* w_split, const float* bias, const float* x,
                                float* clipped, float* recon, double* sse_partial,
                                int sse_unclipped, void* stream) {
  return launch_deconv3_halo({D3_X6}, in_split, B, H, W, N, w_split, bias, x, clipped, recon, sse_partial,
                             sse_unclipped, stream);
}

int iclr17_synthesis_deconv3_x6_cm(const uint16_t* in_split_cm, int B, int H, int W, int N,
                                   const uint16_t* w_split, const float* bias, const float* x,
                                   float* clipped, float* recon, double* sse_partial,
                                   int sse_unclipped, void* stream) {
  return launch_deconv3_halo({D3_X6, 1}, in_split_cm, B, H, W, N, w_split, bias, x, clipped, recon,
                             sse_partial, sse_unclipped, stream);
}

int iclr17_synthesis_deconv3_x6_cm_bits(const uint16_t* in_split_cm, int B, int H, int W, int N,
                                        const uint16_t* w_split, const float* bias, const float* x,
                                        float* clipped, float* recon, double* sse_partial,
                                        int sse_unclipped, const double* bits_partial, int bits_T,
                                        double* bits_per_image, float* bpp_total, double bits_scale,
                                        void* stream) {
  const FoldBits fold = {bits_partial, bits_T, bits_per_image, bpp_total, bits_scale};
  return launch_deconv3_halo({D3_X6, 1, &fold}, in_split_cm, B, H, W, N, w_split, bias, x, clipped, recon,
                             sse_partial, sse_unclipped, stream);
}

int iclr17_synthesis_deconv3_bf16_bits(const uint16_t* in, int B, int H, int W, int N,
                                       const uint16_t* w_bf16, const float* bias, const float* x_ref,
                                       float* clipped, float* recon, double* sse_partial,
                                       int sse_unclipped, const double* bits_partial, int bits_T,
                                       double* bits_per_image, float* bpp_total, double bits_scale,
                                       void* stream) {
  const FoldBits fold = {bits_partial, bits_T, bits_per_image, bpp_total, bits_scale};
  return launch_deconv3_halo({D3_BF16, 0, &fold}, in, B, H, W, N, w_bf16, bias, x_ref, clipped, recon, sse_partial,
                             sse_unclipped, stream);
}

int iclr17_synthesis_deconv3_bf16(const uint16_t* in, int B, int H, int W, int N,
                                  const uint16_t* w_bf16, const float* bias, const float* x_ref,
                                  float* clipped, float* recon, double* sse_partial,
                                  int sse_unclipped, void* stream) {
  return launch_deconv3_halo({D3_BF16}, in, B, H, W, N, w_bf16, bias, x_ref, clipped, recon, sse_partial,
                             sse_unclipped, stream);
}

}  // extern "C"
