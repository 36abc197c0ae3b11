// Entropy coding of the quantised latent ŷ with the factorised BitEstimator — SURVEY §8(f) row 4.
// The reference only ESTIMATES the rate (model.py:71-78: bits = Σ −log2(F(ŷ+½) − F(ŷ−½))); this
// turns the same per-channel distribution into a real bitstream and back, bit-exactly.
//
// Alphabet per channel: values v ∈ [−K, K] (symbol v + K) and one escape symbol (2K + 1) for
// |v| > K, followed by v + 32768 as one uniform 16-bit symbol (|v| ≤ 32767). Probabilities:
// p(v) = F(v + ½) − F(v − ½) with F the BitEstimator CDF evaluated exactly as the rate kernel
// does (common.h bitparm_cdf), p(escape) = F(−K − ½) + (1 − F(K + ½)); quantised to 16-bit
// frequencies (each ≥ 1, summing to 2^16).
//
// Coder: interleaved rANS, 32-bit states in [2^16, 2^32), 16-bit renormalisation words, 16-bit
// probability precision. One wave codes a stream: lane l owns symbols l, l + 64, … with its own
// state; a block's renormalisation words are ordered by lane (ballot + prefix count), so the
// stream stays one word sequence. The encoder writes back to front into its own scratch slot;
// the offsets scan and the pack kernel then concatenate the streams.
//
// The file has one coder and three layouts.
//   Body: encode_stream / decode_stream code one stream with one wave. They hold every rule of
//     the stream format: the classification and escape rule, the order of the sub-rounds, the
//     word placement, the 64 leading states and the status bits. Nothing else in the file does.
//   Layout: a small struct that tells the body what a stream is made of: nsym(), the symbol
//     count, at(i, e), the table row of symbol i and its element e of the latent tensor, and
//     idle(), any readable row, for the lanes past the end of the encoder's last block; a
//     layout with kWindow also has walk_down(blk) / walk_up(blk), which the body calls before a
//     block so the layout can restage its LDS window. Row is a const int* into LDS or a TabRow.
//       PlainLayout  a stream per (image, channel group), symbols in (channel, row, column)
//                    order, every channel's table in LDS;
//       MapLayout    the same streams with a table set per block of latent positions
//                    (DESIGN.md §0i), the tables in an LDS window or in global memory;
//       TileLayout   a stream per (image, tile, channel group).
//   Shell: the six kernels stage tables where their layout does, find their stream, build the
//     layout and call the body.
#include <type_traits>

#include "common.h"

namespace iclr17 {
namespace {

constexpr unsigned kProbBits = 16;
constexpr unsigned kProbScale = 1u << kProbBits;   // Σ freq
constexpr unsigned kL = 1u << 16;                   // state lower bound

// cum[c][0 .. 2K+2]: symbol i covers [cum[i], cum[i+1]) of the 2^16 slots
__global__ void __launch_bounds__(256) tables_kernel(const float* __restrict__ rp, int N, int K,
                                                     int* __restrict__ cum) {
  const int c = blockIdx.x;
  const int NS = 2 * K + 2;   // symbols incl. escape
  extern __shared__ int tsh[];
  float* sc = (float*)tsh;   // [2K + 2] CDF values, then [NS] freqs (as int)
  for (int j = threadIdx.x; j < 2 * K + 2; j += blockDim.x)
    sc[j] = bitparm_cdf((float)(j - K) - 0.5f, rp, N, c);
  __syncthreads();
  if (threadIdx.x != 0) return;
  int* freq = (int*)(sc + 2 * K + 2);
  const float spread = (float)(kProbScale - (unsigned)NS);
  int total = 0, imax = 0;
  float pmax = -1.f;
  for (int i = 0; i < NS; ++i) {
    float p = i < NS - 1 ? sc[i + 1] - sc[i] : sc[0] + (1.0f - sc[2 * K + 1]);
    p = fmaxf(p, 0.f);
    const int f = 1 + (int)floorf(p * spread);
    freq[i] = f;
    total += f;
    if (p > pmax) { pmax = p; imax = i; }
  }
  freq[imax] += (int)kProbScale - total;   // exact sum; the most probable symbol absorbs it
  int* cc = cum + (long)c * (NS + 1);
  int acc = 0;
  for (int i = 0; i < NS; ++i) {
    cc[i] = acc;
    acc += freq[i];
  }
  cc[NS] = acc;
}

struct StreamGeo {
  int HW, N, cpg;   // pixels per channel, channels, channels per stream group
  int P;            // streams per image
};

constexpr int W = 64;   // interleaved lanes per stream (one wave)

__device__ __forceinline__ long sym_index(const StreamGeo& g, int b, int grp, int i) {
  const int cl = i / g.HW, pix = i - cl * g.HW;
  return ((long)b * g.HW + pix) * g.N + grp * g.cpg + cl;   // NHWC element
}

// status bits
enum : int { ST_NONINT = 1, ST_RANGE = 2, ST_OVERRUN = 4, ST_TRAIL = 8 };

// every channel's table into LDS (N·(2K + 3) ints), by a workgroup of T threads
template <int T = W>
__device__ __forceinline__ void load_tables(const int* __restrict__ cum, int n, int* sc) {
  for (int i = threadIdx.x; i < n; i += T) sc[i] = cum[i];
  __syncthreads();
}

__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
  return v;
}

// lanes with `need` get consecutive ranks in lane order; returns (rank, count)
__device__ __forceinline__ int2 lane_rank(bool need, int lane) {
  const unsigned long long m = __ballot(need);
  return make_int2(__popcll(m & ((1ull << lane) - 1ull)), __popcll(m));
}

// ----------------------------------------------------------------------------- the body
// Encodes stream s of layout `lay` with the calling wave. Blocks of 64 symbols are encoded last
// to first; inside a block the escape payloads go first, then the symbols (the decoder's
// reverse). Renormalisation words of a (block, sub-round) are placed back to front as a group,
// lane order ascending, so the decoder reading forward hands each lane its own word. The 64
// final states (high word first) lead the stream.
template <class L>
__device__ __forceinline__ void encode_stream(L& lay, int s, int lane, const float* __restrict__ y,
                                              int K, unsigned short* __restrict__ scratch, long cap,
                                              unsigned* __restrict__ lengths,
                                              int* __restrict__ status) {
  const int NS = 2 * K + 2;
  unsigned short* out = scratch + (long)s * cap;
  long ptr = cap;
  unsigned x = kL;
  int bad = 0;
  const int nsym = lay.nsym();
  const int nblk = (nsym + W - 1) / W;
  for (int blk = nblk - 1; blk >= 0; --blk) {
    if constexpr (L::kWindow) lay.walk_down(blk);
    const int i = blk * W + lane;
    const bool act = i < nsym;
    int sym = 0, pay = -1;
    typename L::Row cc = lay.idle();   // an idle lane reads a row it never codes
    if (act) {
      long e;
      cc = lay.at(i, e);
      const float v = y[e];
      const float r = rintf(v);
      if (!(r == v)) { bad |= ST_NONINT; sym = K; }   // NaN / non-integer
      else if (fabsf(v) > 32767.f) { bad |= ST_RANGE; sym = K; }
      else {
        const int iv = (int)v;
        sym = (iv >= -K && iv <= K) ? iv + K : NS - 1;
        if (sym == NS - 1) pay = iv + 32768;
      }
    }
    // sub-round B: escape payloads (uniform, freq 1: always one word out)
    {
      const bool need = pay >= 0;
      const int2 rc = lane_rank(need, lane);
      if (need) {
        out[ptr - rc.y + rc.x] = (unsigned short)(x & 0xffffu);
        x = ((x >> 16) << 16) + (unsigned)pay;
      }
      ptr -= rc.y;
    }
    // sub-round A: the symbols
    {
      const unsigned start = (unsigned)cc[sym], f = (unsigned)cc[sym + 1] - start;
      const bool need = act && x >= (f << 16);
      const int2 rc = lane_rank(need, lane);
      if (need) {
        out[ptr - rc.y + rc.x] = (unsigned short)(x & 0xffffu);
        x >>= 16;
      }
      ptr -= rc.y;
      if (act) x = ((x / f) << 16) + (x % f) + start;
    }
  }
  ptr -= 2 * W;
  out[ptr + 2 * lane] = (unsigned short)(x >> 16);
  out[ptr + 2 * lane + 1] = (unsigned short)(x & 0xffffu);
  if (lane == 0) lengths[s] = (unsigned)(cap - ptr);
  bad = wave_or(bad);
  if (lane == 0 && bad) atomicOr(status, bad);
}

// Decodes the n words at `in` as a stream of layout `lay` with the calling wave. A stream too
// short for its states makes the whole wave leave, so no barrier of the layout follows.
template <class L>
__device__ __forceinline__ void decode_stream(L& lay, int lane, const unsigned short* __restrict__ in,
                                              long n, int K, float* __restrict__ y,
                                              int* __restrict__ status) {
  const int NS = 2 * K + 2;
  int bad = 0;
  if (n < 2 * W) {
    if (lane == 0) atomicOr(status, ST_OVERRUN);
    return;
  }
  unsigned x = ((unsigned)in[2 * lane] << 16) | in[2 * lane + 1];
  long ptr = 2 * W;
  auto word = [&](bool need, int& fail) -> unsigned {
    const int2 rc = lane_rank(need, lane);
    unsigned w = 0;
    if (need) {
      if (ptr + rc.x < n) w = in[ptr + rc.x];
      else fail |= ST_OVERRUN;
    }
    ptr += rc.y;
    return w;
  };
  const int nsym = lay.nsym();
  const int nblk = (nsym + W - 1) / W;
  for (int blk = 0; blk < nblk; ++blk) {
    if constexpr (L::kWindow) lay.walk_up(blk);
    const int i = blk * W + lane;
    const bool act = i < nsym;
    int v = 0;
    bool esc = false;
    long e = 0;
    if (act) {
      const typename L::Row cc = lay.at(i, e);
      const unsigned slot = x & 0xffffu;
      int lo = 0, hi = NS;   // cc[lo] ≤ slot < cc[hi]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned)cc[mid] <= slot) lo = mid; else hi = mid;
      }
      const unsigned start = (unsigned)cc[lo], f = (unsigned)cc[lo + 1] - start;
      x = f * (x >> 16) + slot - start;
      v = lo - K;
      esc = lo == NS - 1;
    }
    // Sub-round A renormalises after the symbols, sub-round B takes the escape payloads. Where a
    // lane's words lie follows from the ranks alone, so both loads go out before either is used:
    // one memory wait per block, not two (profiles/rans_coder_refactor_ab.txt).
    const bool need = act && x < kL;
    const unsigned wa = word(need, bad), wb = word(esc, bad);
    if (need) x = (x << 16) | wa;
    if (esc) {
      v = (int)(x & 0xffffu) - 32768;
      x = (x & 0xffff0000u) | wb;
    }
    if (act) y[e] = (float)v;
  }
  if (x != kL) bad |= ST_TRAIL;
  if (lane == 0 && ptr != n) bad |= ST_TRAIL;
  bad = wave_or(bad);
  if (lane == 0 && bad) atomicOr(status, bad);
}

// ----------------------------------------------------------------------------- plain streams
// Each image's channels are cut into P contiguous groups, one stream per (image, group), symbols
// in (channel, row, column) order; one wave per workgroup, workgroup s codes stream s.
struct PlainLayout {
  using Row = const int*;
  static constexpr bool kWindow = false;
  const StreamGeo& g;
  const int* sc;   // every channel's table, in LDS
  int TS, b, grp;
  __device__ __forceinline__ PlainLayout(const StreamGeo& geo, const int* tables, int K, int s)
      : g(geo), sc(tables), TS(2 * K + 3), b(s / geo.P), grp(s - b * geo.P) {}
  __device__ __forceinline__ int nsym() const { return g.cpg * g.HW; }
  __device__ __forceinline__ Row idle() const { return sc; }
  __device__ __forceinline__ Row at(int i, long& e) const {
    e = sym_index(g, b, grp, i);
    return sc + (grp * g.cpg + i / g.HW) * TS;
  }
};

__global__ void __launch_bounds__(W) encode_kernel(const float* __restrict__ y, StreamGeo g,
                                                   const int* __restrict__ cum, int K,
                                                   unsigned short* __restrict__ scratch, long cap,
                                                   unsigned* __restrict__ lengths,
                                                   int* __restrict__ status) {
  extern __shared__ int sc[];
  load_tables(cum, g.N * (2 * K + 3), sc);
  const int s = blockIdx.x;
  PlainLayout lay(g, sc, K, s);
  encode_stream(lay, s, threadIdx.x, y, K, scratch, cap, lengths, status);
}

__global__ void __launch_bounds__(W) decode_kernel(const unsigned short* __restrict__ words,
                                                   const long* __restrict__ offsets, StreamGeo g,
                                                   const int* __restrict__ cum, int K,
                                                   float* __restrict__ y, int* __restrict__ status) {
  extern __shared__ int sc[];
  load_tables(cum, g.N * (2 * K + 3), sc);
  const int s = blockIdx.x;
  PlainLayout lay(g, sc, K, s);
  decode_stream(lay, threadIdx.x, words + offsets[s], offsets[s + 1] - offsets[s], K, y, status);
}

// offsets[0] = 0, offsets[i + 1] = offsets[i] + lengths[i]   (one workgroup; n ≤ a few 10^5)
__global__ void __launch_bounds__(1024) offsets_kernel(const unsigned* __restrict__ len, int n,
                                                       long* __restrict__ offsets) {
  __shared__ long part[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int i0 = t * per, i1 = min(n, i0 + per);
  long s = 0;
  for (int i = i0; i < i1; ++i) s += len[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    long a = 0;
    for (int k = 0; k < 1024; ++k) {
      const long v = part[k];
      part[k] = a;
      a += v;
    }
  }
  __syncthreads();
  long a = part[t];
  for (int i = i0; i < i1; ++i) {
    offsets[i] = a;
    a += len[i];
  }
  if (i1 == n && i0 < i1) offsets[n] = a;
  if (n == 0 && t == 0) offsets[0] = 0;
}

__global__ void __launch_bounds__(256) pack_kernel(const unsigned short* __restrict__ scratch,
                                                   long cap, const long* __restrict__ offsets,
                                                   unsigned short* __restrict__ words) {
  const int s = blockIdx.x;
  const long o = offsets[s], n = offsets[s + 1] - o;
  const unsigned short* src = scratch + (long)s * cap + (cap - n);
  for (long i = threadIdx.x; i < n; i += 256) words[o + i] = src[i];
}

// ----------------------------------------------------------------------------- step maps (§0i)
// MapLayout: PlainLayout's streams with a table row per symbol: the symbol of channel c at latent
// position (i, j) of image b is coded with row slot·N + c of the stacked tables
// cum[S][N][2K + 3], slot = slots[b][i >> lg][j >> lg].
//
// S·N tables do not fit the LDS (32 steps × 192 channels × 67 ints = 1.6 MB), and a stream walks
// its channels in order, so the LDS holds a WINDOW: the rows of wc consecutive channels for all S
// slots, sc[slot][wc][2K + 3]. When a block's leading channel (the decoder walks up, the encoder
// down) has left the window, the wave stages the next one (one wave per workgroup: the barrier
// is cheap). A lane whose channel lies outside the window — a block that straddles its edge, or
// a latent so small that a block of 64 symbols spans more channels than the window holds — reads
// its row from global memory. wc = 0: no window, every row from global memory.
struct MapTab {
  const int* cum;               // [S][N][2K + 3]
  const unsigned char* slots;   // [B][mhw]
  int S, w, mw, mhw, lg;
  int wc;                       // channels per LDS window
};

struct TabRow {   // one symbol's table row, in the window or in global memory
  const int* l;
  const int* g;
  bool in;
  __device__ __forceinline__ int operator[](int i) const { return in ? l[i] : g[i]; }
};

struct Window {
  int c0 = 0, n = 0;   // channels [c0, c0 + n) are staged
};

// stage channels [c0, c0 + n) of every slot (n ≤ wc); all lanes call it
__device__ __forceinline__ void stage_window(const MapTab& m, int N, int TS, int c0, int n,
                                             int* sc) {
  __syncthreads();   // every lane is done with the window that goes
  for (int s = 0; s < m.S; ++s) {
    const int* src = m.cum + ((long)s * N + c0) * TS;
    int* dst = sc + (long)s * m.wc * TS;
    for (int i = threadIdx.x; i < n * TS; i += W) dst[i] = src[i];
  }
  __syncthreads();
}

// the row of symbol i (channel cl of the stream's group) of stream (b, grp)
__device__ __forceinline__ TabRow map_row(const MapTab& m, const StreamGeo& g, int TS,
                                          const Window& win, const int* sc, int b, int grp,
                                          int i) {
  const int cl = i / g.HW, pix = i - cl * g.HW;
  const int r = pix / m.w, q = pix - r * m.w;
  int slot = m.slots[(long)b * m.mhw + (r >> m.lg) * m.mw + (q >> m.lg)];
  slot = slot < m.S ? slot : m.S - 1;   // the caller checked the map; never read past the tables
  const int c = grp * g.cpg + cl;
  TabRow t;
  t.in = c >= win.c0 && c < win.c0 + win.n;
  t.l = sc + ((long)slot * m.wc + (c - win.c0)) * TS;
  t.g = m.cum + ((long)slot * g.N + c) * TS;
  return t;
}

struct MapLayout {
  using Row = TabRow;
  static constexpr bool kWindow = true;
  const StreamGeo& g;
  const MapTab& m;
  int* sc;   // the window, in LDS
  int TS, b, grp;
  Window win;
  __device__ __forceinline__ MapLayout(const StreamGeo& geo, const MapTab& tab, int* window, int K,
                                       int s)
      : g(geo), m(tab), sc(window), TS(2 * K + 3), b(s / geo.P), grp(s - b * geo.P) {}
  __device__ __forceinline__ int nsym() const { return g.cpg * g.HW; }
  __device__ __forceinline__ Row idle() const { return {sc, m.cum, false}; }
  __device__ __forceinline__ Row at(int i, long& e) const {
    e = sym_index(g, b, grp, i);
    return map_row(m, g, TS, win, sc, b, grp, i);
  }
  // the encoder walks down: restage once the block's last channel is below the window
  __device__ __forceinline__ void walk_down(int blk) {
    if (m.wc == 0) return;
    const int last = blk * W + W - 1 < nsym() ? blk * W + W - 1 : nsym() - 1;
    const int chi = grp * g.cpg + last / g.HW;
    if (win.n == 0 || chi < win.c0) {
      win.c0 = chi - m.wc + 1 > grp * g.cpg ? chi - m.wc + 1 : grp * g.cpg;
      win.n = chi - win.c0 + 1;
      stage_window(m, g.N, TS, win.c0, win.n, sc);
    }
  }
  // the decoder walks up: restage once the block's first channel is above the window
  __device__ __forceinline__ void walk_up(int blk) {
    if (m.wc == 0) return;
    const int clo = grp * g.cpg + blk * W / g.HW;
    if (win.n == 0 || clo >= win.c0 + win.n) {
      const int end = (grp + 1) * g.cpg;
      win.c0 = clo;
      win.n = end - clo < m.wc ? end - clo : m.wc;
      stage_window(m, g.N, TS, win.c0, win.n, sc);
    }
  }
};

__global__ void __launch_bounds__(W) encode_map_kernel(const float* __restrict__ y, StreamGeo g,
                                                       MapTab m, int K,
                                                       unsigned short* __restrict__ scratch,
                                                       long cap, unsigned* __restrict__ lengths,
                                                       int* __restrict__ status) {
  extern __shared__ int sc[];
  const int s = blockIdx.x;
  MapLayout lay(g, m, sc, K, s);
  encode_stream(lay, s, threadIdx.x, y, K, scratch, cap, lengths, status);
}

__global__ void __launch_bounds__(W) decode_map_kernel(const unsigned short* __restrict__ words,
                                                       const long* __restrict__ offsets,
                                                       StreamGeo g, MapTab m, int K,
                                                       float* __restrict__ y,
                                                       int* __restrict__ status) {
  extern __shared__ int sc[];
  const int s = blockIdx.x;
  MapLayout lay(g, m, sc, K, s);
  decode_stream(lay, threadIdx.x, words + offsets[s], offsets[s + 1] - offsets[s], K, y, status);
}

// The window of a map launch: as many channels as the S slots' rows allow in 64 KiB of LDS, at
// most the stream's; 0 (every row from global memory) when asked or when one channel does not fit.
int map_window(int S, int K, int cpg, int window) {
  if (!window) return 0;
  const long per_channel = (long)S * (2 * K + 3) * sizeof(int);
  const long wc = 64 * 1024 / per_channel;
  return (int)(wc < cpg ? wc : cpg);
}

// ----------------------------------------------------------------------------- tiles (§0k)
// TileLayout: a stream per spatial tile: the h×w latent is cut into tiles of t×t positions
// (t = 2^lg; ragged at the bottom and right), one stream per (image, tile row, tile column,
// channel group) in that order, symbols in (channel, row in tile, column in tile) order, every
// channel's table in LDS. The body codes it, so a tile's words are the oracle's encode_stream of
// its sequence.
//
// A launch codes the streams of a rectangle of tiles, nr×nc from tile (r0, c0), against a tensor
// [B][oh][ow][N] whose origin is the rectangle's first position: the whole grid and the whole
// latent for the encoder and a full decode, a few tiles and a compact window for a region decode.
// Every stream's place follows from its index and this geometry, which the host has checked; no
// address comes from device memory.
//
// WAVES waves share one workgroup and one staged table set, one stream each. Staging ends in the
// kernels' only barrier: after it the waves run independently and those without a stream have
// returned, which is why this layout has no per-block hook.
struct TileGeo {
  int h, w, N, cpg, P;   // the latent, its channels, channels per group, groups
  int lg;                // log2 of the tile edge
  int r0, c0, nr, nc;    // the rectangle of tiles
  int oh, ow;            // the tensor's rows and columns
  int ns;                // streams of the launch: B·nr·nc·P
};

// n / d for a divisor that is the same for the whole wave and every n below a bound known when
// the stream starts: one multiply where m = ⌊2^32/d⌋ + 1 is exact (n·d < 2^32, d > 1), the
// division otherwise. Worth 2 % of the tiled encoder and nothing measurable in the decoder (§0k).
struct Divisor {
  unsigned d, m;
  bool fast;
  __device__ __forceinline__ void set(unsigned divisor, unsigned long long bound) {
    d = divisor;
    fast = d > 1 && bound * d < (1ull << 32);
    m = fast ? (unsigned)((1ull << 32) / d) + 1u : 0u;
  }
  __device__ __forceinline__ unsigned operator()(unsigned n) const {
    return fast ? __umulhi(n, m) : n / d;
  }
};

struct TileStream {
  int b, grp;
  long e0;       // the element of the tile's origin and the group's first channel in the tensor
  int th, tw;    // the tile's extent
  Divisor by_hw, by_tw;
};

__device__ __forceinline__ TileStream tile_stream(const TileGeo& g, int s) {
  TileStream d;
  d.grp = s % g.P;
  int q = s / g.P;
  const int tc = q % g.nc;
  q /= g.nc;
  const int tr = q % g.nr;
  d.b = q / g.nr;
  const int t = 1 << g.lg;
  d.e0 = (((long)d.b * g.oh + tr * t) * g.ow + tc * t) * g.N + d.grp * g.cpg;
  d.th = min(t, g.h - (g.r0 + tr) * t);
  d.tw = min(t, g.w - (g.c0 + tc) * t);
  d.by_hw.set((unsigned)(d.th * d.tw), (unsigned long long)g.cpg * d.th * d.tw + W);
  d.by_tw.set((unsigned)d.tw, (unsigned long long)d.th * d.tw);
  return d;
}

// symbol i of the stream: its channel within the group and its element of the tensor
__device__ __forceinline__ long tile_index(const TileGeo& g, const TileStream& d, int i, int& cl) {
  const int hw = d.th * d.tw;
  cl = (int)d.by_hw((unsigned)i);
  const int pix = i - cl * hw;
  const int r = (int)d.by_tw((unsigned)pix), q = pix - r * d.tw;
  return d.e0 + ((long)r * g.ow + q) * g.N + cl;
}

struct TileLayout {
  using Row = const int*;
  static constexpr bool kWindow = false;
  const TileGeo& g;
  const int* sc;   // every channel's table, in LDS
  int TS;
  TileStream d;
  __device__ __forceinline__ TileLayout(const TileGeo& geo, const int* tables, int K, int s)
      : g(geo), sc(tables), TS(2 * K + 3), d(tile_stream(geo, s)) {}
  __device__ __forceinline__ int nsym() const { return g.cpg * d.th * d.tw; }
  __device__ __forceinline__ Row idle() const { return sc; }
  __device__ __forceinline__ Row at(int i, long& e) const {
    int cl;
    e = tile_index(g, d, i, cl);
    return sc + (d.grp * g.cpg + cl) * TS;
  }
};

template <int WAVES>
__global__ void __launch_bounds__(W * WAVES) encode_tiled_kernel(
    const float* __restrict__ y, TileGeo g, const int* __restrict__ cum, int K,
    unsigned short* __restrict__ scratch, long cap, unsigned* __restrict__ lengths,
    int* __restrict__ status) {
  extern __shared__ int sc[];
  load_tables<W * WAVES>(cum, g.N * (2 * K + 3), sc);   // the only barrier
  const int s = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (s >= g.ns) return;
  TileLayout lay(g, sc, K, s);
  encode_stream(lay, s, threadIdx.x & (W - 1), y, K, scratch, cap, lengths, status);
}

template <int WAVES>
__global__ void __launch_bounds__(W * WAVES) decode_tiled_kernel(
    const unsigned short* __restrict__ words, const long* __restrict__ offsets, long total,
    TileGeo g, const int* __restrict__ cum, int K, float* __restrict__ y,
    int* __restrict__ status) {
  extern __shared__ int sc[];
  load_tables<W * WAVES>(cum, g.N * (2 * K + 3), sc);   // the only barrier
  const int s = blockIdx.x * WAVES + (threadIdx.x >> 6), lane = threadIdx.x & (W - 1);
  if (s >= g.ns) return;
  const long o0 = offsets[s], o1 = offsets[s + 1];
  // the offsets come from a stream: never read outside the words, whatever they say
  if (o0 < 0 || o1 > total) {
    if (lane == 0) atomicOr(status, ST_OVERRUN);
    return;
  }
  TileLayout lay(g, sc, K, s);
  decode_stream(lay, lane, words + o0, o1 - o0, K, y, status);
}

// Waves per workgroup when the caller leaves it open (§0k, profiles/tiled_ab.txt). The coder is
// bound by one wave's chain of dependent steps, not by throughput: while every stream can have a
// workgroup of its own resident — the LDS holds ⌊160 KiB / tables⌋ of them per CU — one wave per
// workgroup spreads the streams over the most CUs and is the faster by 0–9 %. With more streams
// than that, one-wave workgroups queue behind the LDS limit while SIMDs idle, and four waves
// sharing a staged table set are 1.3–1.7× faster.
int tiled_waves(int ns, size_t shm) {
  static int cus = 0;
  if (!cus) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  const long resident = (long)cus * (long)((160 * 1024) / shm);
  return ns <= resident ? 1 : 4;
}

// The geometry of a tiled launch from the caller's scalars, or false with the reason in `why`.
bool tile_geo(int B, int h, int w, int N, int P, int log2_t, int r0, int c0, int nr, int nc,
              TileGeo& g, const char*& why) {
  why = "bad shape";
  if (B <= 0 || h <= 0 || w <= 0 || N <= 0 || P <= 0 || N % P) return false;
  why = "log2 of the tile edge is not 3..6";
  if (log2_t < 3 || log2_t > 6) return false;
  const int t = 1 << log2_t, th = (h + t - 1) / t, tw = (w + t - 1) / t;
  why = "the tile rectangle is not inside the tile grid";
  if (r0 < 0 || c0 < 0 || nr <= 0 || nc <= 0 || r0 > th - nr || c0 > tw - nc) return false;
  why = "too many streams";
  const long ns = (long)B * nr * nc * P;
  if (ns > (1L << 24)) return false;
  g.h = h; g.w = w; g.N = N; g.cpg = N / P; g.P = P; g.lg = log2_t;
  g.r0 = r0; g.c0 = c0; g.nr = nr; g.nc = nc;
  g.oh = (h < (r0 + nr) * t ? h : (r0 + nr) * t) - r0 * t;
  g.ow = (w < (c0 + nc) * t ? w : (c0 + nc) * t) - c0 * t;
  g.ns = (int)ns;
  return true;
}

// The bytes of N channels' tables, which a launch that stages them all must fit in the LDS.
int table_bytes(const char* what, int N, int K, size_t& shm) {
  shm = (size_t)N * (2 * K + 3) * sizeof(int);
  ICLR17_REQUIRE(shm <= 64 * 1024, ICLR17_EINVAL, "%s: tables of %zu bytes exceed LDS", what, shm);
  return 0;
}

// The geometry, tables and dynamic LDS of a mapped launch from the caller's (checked) scalars.
struct MapLaunch {
  StreamGeo g;
  MapTab m;
  size_t shm;
};

MapLaunch map_launch(int h, int w, int N, int P, const int32_t* cum, int S, int K,
                     const uint8_t* slots, int log2_g, int window) {
  const StreamGeo g{h * w, N, N / P, P};
  const int gb = 1 << log2_g, mh = (h + gb - 1) / gb, mw = (w + gb - 1) / gb;
  const MapTab m{(const int*)cum, (const unsigned char*)slots, S, w, mw, mh * mw, log2_g,
                 map_window(S, K, g.cpg, window)};
  return {g, m, (size_t)S * m.wc * (2 * K + 3) * sizeof(int)};
}

// launch(integral_constant<int, waves>) for a supported number of waves per workgroup
template <class F>
bool with_waves(int waves, F&& launch) {
  switch (waves) {
    case 1: launch(std::integral_constant<int, 1>{}); return true;
    case 2: launch(std::integral_constant<int, 2>{}); return true;
    case 4: launch(std::integral_constant<int, 4>{}); return true;
    case 8: launch(std::integral_constant<int, 8>{}); return true;
    case 16: launch(std::integral_constant<int, 16>{}); return true;
    default: return false;
  }
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_entropy_tables(const float* rate_packed, int N, int K, int32_t* cum, void* stream) {
  ICLR17_REQUIRE(rate_packed && cum && N > 0 && K >= 1 && K <= 1024, ICLR17_EINVAL,
                 "entropy_tables: bad arguments (K=%d)", K);
  const size_t shm = (size_t)(2 * K + 2) * 4 + (size_t)(2 * K + 2) * 4;
  hipLaunchKernelGGL(tables_kernel, dim3(N), dim3(256), shm, (hipStream_t)stream, rate_packed,
                     N, K, (int*)cum);
  return check_launch("entropy_tables");
}

long iclr17_rans_capacity(int h, int w, int N, int streams_per_image) {
  if (h <= 0 || w <= 0 || N <= 0 || streams_per_image <= 0 || N % streams_per_image) return 0;
  return 2L * W + 2L * (N / streams_per_image) * h * w;
}

int iclr17_rans_encode(const float* y_hat, int B, int h, int w, int N, int streams_per_image,
                       const int32_t* cum, int K, uint16_t* scratch, long scratch_words,
                       uint32_t* lengths, int32_t* status, void* stream) {
  const long cap = iclr17_rans_capacity(h, w, N, streams_per_image);
  ICLR17_REQUIRE(y_hat && cum && scratch && lengths && status && B > 0 && cap > 0 && K >= 1,
                 ICLR17_EINVAL, "rans_encode: bad arguments");
  size_t shm;
  if (const int rc = table_bytes("rans_encode", N, K, shm)) return rc;
  const int ns = B * streams_per_image;
  ICLR17_REQUIRE(scratch_words >= cap * ns, ICLR17_EINVAL,
                 "rans_encode: scratch of %ld words < %ld", scratch_words, cap * ns);
  StreamGeo g{h * w, N, N / streams_per_image, streams_per_image};
  hipLaunchKernelGGL(encode_kernel, dim3(ns), dim3(W), shm, (hipStream_t)stream, y_hat, g,
                     (const int*)cum, K, (unsigned short*)scratch, cap, (unsigned*)lengths,
                     (int*)status);
  return check_launch("rans_encode");
}

int iclr17_rans_offsets(const uint32_t* lengths, int n, int64_t* offsets, void* stream) {
  ICLR17_REQUIRE(lengths && offsets && n >= 0, ICLR17_EINVAL, "rans_offsets: bad arguments");
  hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream,
                     (const unsigned*)lengths, n, (long*)offsets);
  return check_launch("rans_offsets");
}

int iclr17_rans_pack(const uint16_t* scratch, long cap, const int64_t* offsets, int n,
                     uint16_t* words, void* stream) {
  ICLR17_REQUIRE(scratch && offsets && words && n > 0 && cap > 0, ICLR17_EINVAL,
                 "rans_pack: bad arguments");
  hipLaunchKernelGGL(pack_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned short*)scratch, cap, (const long*)offsets,
                     (unsigned short*)words);
  return check_launch("rans_pack");
}

int iclr17_rans_decode(const uint16_t* words, const int64_t* offsets, int B, int h, int w, int N,
                       int streams_per_image, const int32_t* cum, int K, float* y_hat,
                       int32_t* status, void* stream) {
  ICLR17_REQUIRE(words && offsets && cum && y_hat && status && B > 0 && h > 0 && w > 0 &&
                     N > 0 && streams_per_image > 0 && N % streams_per_image == 0 && K >= 1,
                 ICLR17_EINVAL, "rans_decode: bad arguments");
  size_t shm;
  if (const int rc = table_bytes("rans_decode", N, K, shm)) return rc;
  const int ns = B * streams_per_image;
  StreamGeo g{h * w, N, N / streams_per_image, streams_per_image};
  hipLaunchKernelGGL(decode_kernel, dim3(ns), dim3(W), shm, (hipStream_t)stream,
                     (const unsigned short*)words, (const long*)offsets, g, (const int*)cum, K,
                     y_hat, (int*)status);
  return check_launch("rans_decode");
}

int iclr17_rans_encode_map(const float* y_hat, int B, int h, int w, int N, int streams_per_image,
                           const int32_t* cum, int S, int K, const uint8_t* slots, int log2_g,
                           int window, uint16_t* scratch, long scratch_words, uint32_t* lengths,
                           int32_t* status, void* stream) {
  const long cap = iclr17_rans_capacity(h, w, N, streams_per_image);
  ICLR17_REQUIRE(y_hat && cum && slots && scratch && lengths && status && B > 0 && cap > 0 &&
                     K >= 1 && K <= 1024,
                 ICLR17_EINVAL, "rans_encode_map: bad arguments");
  ICLR17_REQUIRE(S >= 1 && S <= 32, ICLR17_EINVAL, "rans_encode_map: S=%d table sets (1..32)", S);
  ICLR17_REQUIRE(log2_g >= 0 && log2_g <= 4, ICLR17_EINVAL,
                 "rans_encode_map: log2 of the block edge is %d (0..4)", log2_g);
  const int ns = B * streams_per_image;
  ICLR17_REQUIRE(scratch_words >= cap * ns, ICLR17_EINVAL,
                 "rans_encode_map: scratch of %ld words < %ld", scratch_words, cap * ns);
  const MapLaunch l = map_launch(h, w, N, streams_per_image, cum, S, K, slots, log2_g, window);
  hipLaunchKernelGGL(encode_map_kernel, dim3(ns), dim3(W), l.shm, (hipStream_t)stream, y_hat, l.g,
                     l.m, K, (unsigned short*)scratch, cap, (unsigned*)lengths, (int*)status);
  return check_launch("rans_encode_map");
}

int iclr17_rans_decode_map(const uint16_t* words, const int64_t* offsets, int B, int h, int w,
                           int N, int streams_per_image, const int32_t* cum, int S, int K,
                           const uint8_t* slots, int log2_g, int window, float* y_hat,
                           int32_t* status, void* stream) {
  ICLR17_REQUIRE(words && offsets && cum && slots && y_hat && status && B > 0 && h > 0 && w > 0 &&
                     N > 0 && streams_per_image > 0 && N % streams_per_image == 0 && K >= 1 &&
                     K <= 1024,
                 ICLR17_EINVAL, "rans_decode_map: bad arguments");
  ICLR17_REQUIRE(S >= 1 && S <= 32, ICLR17_EINVAL, "rans_decode_map: S=%d table sets (1..32)", S);
  ICLR17_REQUIRE(log2_g >= 0 && log2_g <= 4, ICLR17_EINVAL,
                 "rans_decode_map: log2 of the block edge is %d (0..4)", log2_g);
  const int ns = B * streams_per_image;
  const MapLaunch l = map_launch(h, w, N, streams_per_image, cum, S, K, slots, log2_g, window);
  hipLaunchKernelGGL(decode_map_kernel, dim3(ns), dim3(W), l.shm, (hipStream_t)stream,
                     (const unsigned short*)words, (const long*)offsets, l.g, l.m, K, y_hat,
                     (int*)status);
  return check_launch("rans_decode_map");
}

long iclr17_rans_tiled_capacity(int N, int streams_per_tile, int log2_t) {
  if (N <= 0 || streams_per_tile <= 0 || N % streams_per_tile || log2_t < 3 || log2_t > 6) return 0;
  return 2L * W + 2L * (N / streams_per_tile) * (1L << (2 * log2_t));
}

int iclr17_rans_tiled_streams(int h, int w, int streams_per_tile, int log2_t) {
  if (h <= 0 || w <= 0 || streams_per_tile <= 0 || log2_t < 3 || log2_t > 6) return 0;
  const long t = 1L << log2_t;
  const long n = ((h + t - 1) / t) * ((w + t - 1) / t) * streams_per_tile;
  return n > (1L << 24) ? 0 : (int)n;
}

int iclr17_rans_encode_tiled(const float* y_hat, int B, int h, int w, int N, int streams_per_tile,
                             int log2_t, const int32_t* cum, int K, int waves, uint16_t* scratch,
                             long scratch_words, uint32_t* lengths, int32_t* status,
                             void* stream) {
  ICLR17_REQUIRE(y_hat && cum && scratch && lengths && status && K >= 1 && K <= 1024,
                 ICLR17_EINVAL, "rans_encode_tiled: bad arguments");
  TileGeo g;
  const char* why;
  const int t = log2_t >= 3 && log2_t <= 6 ? 1 << log2_t : 1;
  ICLR17_REQUIRE(tile_geo(B, h, w, N, streams_per_tile, log2_t, 0, 0, (h + t - 1) / t,
                          (w + t - 1) / t, g, why),
                 ICLR17_EINVAL, "rans_encode_tiled: %s", why);
  size_t shm;
  if (const int rc = table_bytes("rans_encode_tiled", N, K, shm)) return rc;
  const long cap = iclr17_rans_tiled_capacity(N, streams_per_tile, log2_t);
  ICLR17_REQUIRE(scratch_words >= cap * g.ns, ICLR17_EINVAL,
                 "rans_encode_tiled: scratch of %ld words < %ld", scratch_words, cap * g.ns);
  if (!waves) waves = tiled_waves(g.ns, shm);
  const bool ok = with_waves(waves, [&](auto wv) {
    constexpr int WV = decltype(wv)::value;
    hipLaunchKernelGGL(encode_tiled_kernel<WV>, dim3((g.ns + WV - 1) / WV), dim3(W * WV), shm,
                       (hipStream_t)stream, y_hat, g, (const int*)cum, K, (unsigned short*)scratch,
                       cap, (unsigned*)lengths, (int*)status);
  });
  ICLR17_REQUIRE(ok, ICLR17_EINVAL,
                 "rans_encode_tiled: %d waves per workgroup (0, 1, 2, 4, 8, 16)", waves);
  return check_launch("rans_encode_tiled");
}

int iclr17_rans_decode_tiled(const uint16_t* words, long total_words, const int64_t* offsets,
                             int B, int h, int w, int N, int streams_per_tile, int log2_t, int r0,
                             int c0, int nr, int nc, const int32_t* cum, int K, int waves,
                             float* y_hat, long y_elems, int32_t* status, void* stream) {
  ICLR17_REQUIRE(words && offsets && cum && y_hat && status && total_words >= 0 && K >= 1 &&
                     K <= 1024,
                 ICLR17_EINVAL, "rans_decode_tiled: bad arguments");
  TileGeo g;
  const char* why;
  ICLR17_REQUIRE(tile_geo(B, h, w, N, streams_per_tile, log2_t, r0, c0, nr, nc, g, why),
                 ICLR17_EINVAL, "rans_decode_tiled: %s", why);
  size_t shm;
  if (const int rc = table_bytes("rans_decode_tiled", N, K, shm)) return rc;
  const long need = (long)B * g.oh * g.ow * N;
  ICLR17_REQUIRE(y_elems >= need, ICLR17_EINVAL,
                 "rans_decode_tiled: output of %ld elements < %ld", y_elems, need);
  if (!waves) waves = tiled_waves(g.ns, shm);
  const bool ok = with_waves(waves, [&](auto wv) {
    constexpr int WV = decltype(wv)::value;
    hipLaunchKernelGGL(decode_tiled_kernel<WV>, dim3((g.ns + WV - 1) / WV), dim3(W * WV), shm,
                       (hipStream_t)stream, (const unsigned short*)words, (const long*)offsets,
                       total_words, g, (const int*)cum, K, y_hat, (int*)status);
  });
  ICLR17_REQUIRE(ok, ICLR17_EINVAL,
                 "rans_decode_tiled: %d waves per workgroup (0, 1, 2, 4, 8, 16)", waves);
  return check_launch("rans_decode_tiled");
}

}  // extern "C"
