// A quantiser step per block of latent positions: region-of-interest coding.
//
// The latent of a canvas is h×w positions; a block is g×g of them (g = 2^lg, lg = 0..4) and the
// map is mh×mw = ⌈h/g⌉×⌈w/g⌉ per image, row-major, the last row and column ragged. Position (i, j)
// belongs to block (i >> lg, j >> lg); every channel of a position shares its block's step.
//
//   quantise_step_map    ŷ = rintf(y/Δ_e) and Δ_e·ŷ in one pass, e the block's ladder index (u8
//                        map); ratectl.hip's quantise_step with the step looked up per element
//   dequantise_step_map  Δ_e·ŷ alone (the decoder's half)
//   rate_sweep_offsets   bits[b][s] for every base index s = 0..31 from ONE read of y, an element's
//                        step at base s being Δ_clamp(s + off, 0, 31) with off its block's signed
//                        offset (i8 map)
//
// The offset sweep is ratectl.hip's rate_sweep_kernel with the step looked up: the same 4096-
// element chunks, thread → element map, LDS accumulators and order of additions, reduced by
// iclr17_reduce_partials. With zero offsets it computes rate_sweep's 32-step result bit for bit,
// and with one offset c for a whole image its row s is rate_sweep's row clamp(s + c).
#include <math.h>

#include "common.h"

namespace iclr17 {
namespace {

constexpr int kLadder = 32;          // ladder indices: the sweep's bases and the map's values
constexpr int kSweepChunk = 4096;    // ratectl.hip's kSweepChunk
constexpr int kSweepThreads = 256;

struct Ladder {
  float d[kLadder];
};

struct MapGeo {
  int hw, w;      // latent positions per image, latent width
  int mhw, mw;    // map entries per image, map width
  int lg;         // log2 of the block edge
};

// the map entry of latent position `pos` (b·h·w + i·w + j)
__device__ __forceinline__ long map_entry(const MapGeo& g, long pos) {
  const long b = pos / g.hw;
  const int pix = (int)(pos - b * g.hw);
  const int i = pix / g.w, j = pix - i * g.w;
  return b * g.mhw + (long)(i >> g.lg) * g.mw + (j >> g.lg);
}

__device__ __forceinline__ void stage_ladder(const Ladder& st, float* sd) {
  if (threadIdx.x < kLadder) sd[threadIdx.x] = st.d[threadIdx.x];
  __syncthreads();
}

enum : int { ST_NAN = 1, ST_RANGE = 2 };

__global__ void __launch_bounds__(256) quantise_step_map_kernel(
    const float* __restrict__ y, long n, int C, MapGeo g, const unsigned char* __restrict__ idx,
    Ladder st, float* __restrict__ y_hat, float* __restrict__ y_deq, int* __restrict__ status) {
  __shared__ float sd[kLadder];
  stage_ladder(st, sd);
  int bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = sd[idx[map_entry(g, i / C)] & (kLadder - 1)];
    const float q = rintf(y[i] / d);
    if (!(q == q)) bad |= ST_NAN;
    else if (fabsf(q) > 32767.f) bad |= ST_RANGE;
    y_hat[i] = q;
    y_deq[i] = d * q;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(status, bad);
}

__global__ void __launch_bounds__(256) dequantise_step_map_kernel(
    const float* __restrict__ y_hat, long n, int C, MapGeo g,
    const unsigned char* __restrict__ idx, Ladder st, float* __restrict__ y_deq) {
  __shared__ float sd[kLadder];
  stage_ladder(st, sd);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    y_deq[i] = sd[idx[map_entry(g, i / C)] & (kLadder - 1)] * y_hat[i];
}

// rate_sweep_kernel (ratectl.hip) over the 32 bases, the step of (element, base s) read from the
// ladder in LDS at clamp(s + offset of the element's block). partial[b][s][chunk].
__global__ void __launch_bounds__(kSweepThreads) rate_sweep_offsets_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ rp, Ladder st,
    MapGeo g, const signed char* __restrict__ off, double* __restrict__ partial, int chunks) {
  extern __shared__ float lds[];
  __shared__ float red[4][kLadder];
  __shared__ float sd[kLadder];
  float* sp = lds;                         // [11][C]
  float* acc = lds + kRateRows * C;        // [32][256]
  const int tid = threadIdx.x;
  for (int i = tid; i < kRateRows * C; i += kSweepThreads) sp[i] = rp[i];
  for (int s = 0; s < kLadder; ++s) acc[s * kSweepThreads + tid] = 0.f;
  stage_ladder(st, sd);
  const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const long lo = (long)ch * kSweepChunk;
  const long hi = lo + kSweepChunk < per_image ? lo + kSweepChunk : per_image;
  for (long j = lo + tid; j < hi; j += kSweepThreads) {
    const int c = (int)(j % C);
    const float v = y[(long)b * per_image + j];
    const int o = off[map_entry(g, (long)b * g.hw + j / C)];
    float p[kRateRows];
#pragma unroll
    for (int k = 0; k < kRateRows; ++k) p[k] = sp[k * C + c];
#pragma unroll 1
    for (int s = 0; s < kLadder; ++s) {
      const int e = min(max(s + o, 0), kLadder - 1);
      const float d = sd[e];
      const float z = rintf(v / d);
      acc[s * kSweepThreads + tid] += bits_regs(z, p[0] * d, p);
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  for (int s = 0; s < kLadder; ++s) {
    const float t = wave_sum(acc[s * kSweepThreads + tid]);
    if (lane == 0) red[wave][s] = t;
  }
  __syncthreads();
  if (tid < kLadder) {
    double t = 0.0;
    for (int w = 0; w < 4; ++w) t += (double)red[w][tid];
    partial[((long)b * kLadder + tid) * chunks + ch] = t;
  }
}

unsigned elementwise_blocks(long n) {
  const long blocks = (n + 255) / 256;
  return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

// the ladder by value; false (and the error set) on a step that is not finite and positive
bool ladder_of(const char* what, const float* steps, Ladder& st) {
  for (int s = 0; s < kLadder; ++s) {
    if (!(isfinite(steps[s]) && steps[s] > 0.f)) {
      set_error(ICLR17_EINVAL, "%s: step %d (%g) is not finite and positive", what, s,
                (double)steps[s]);
      return false;
    }
    st.d[s] = steps[s];
  }
  return true;
}

MapGeo geo_of(int h, int w, int lg) {
  const int g = 1 << lg;
  const int mh = (h + g - 1) / g, mw = (w + g - 1) / g;
  return MapGeo{h * w, w, mh * mw, mw, lg};
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_quantise_step_map(const float* y, int B, int h, int w, int N, const uint8_t* indices,
                             int log2_g, const float* steps, float* y_hat, float* y_deq,
                             int32_t* status, void* stream) {
  ICLR17_REQUIRE(y && indices && steps && y_hat && y_deq && status, ICLR17_EINVAL,
                 "quantise_step_map: null pointer");
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "quantise_step_map: bad shape B=%d h=%d w=%d N=%d", B, h, w, N);
  ICLR17_REQUIRE(log2_g >= 0 && log2_g <= 4, ICLR17_EINVAL,
                 "quantise_step_map: log2 of the block edge is %d (0..4)", log2_g);
  Ladder st;
  if (!ladder_of("quantise_step_map", steps, st)) return ICLR17_EINVAL;
  const long n = (long)B * h * w * N;
  hipLaunchKernelGGL(quantise_step_map_kernel, dim3(elementwise_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, y, n, N, geo_of(h, w, log2_g),
                     (const unsigned char*)indices, st, y_hat, y_deq, (int*)status);
  return check_launch("quantise_step_map");
}

int iclr17_dequantise_step_map(const float* y_hat, int B, int h, int w, int N,
                               const uint8_t* indices, int log2_g, const float* steps,
                               float* y_deq, void* stream) {
  ICLR17_REQUIRE(y_hat && indices && steps && y_deq, ICLR17_EINVAL,
                 "dequantise_step_map: null pointer");
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "dequantise_step_map: bad shape B=%d h=%d w=%d N=%d", B, h, w, N);
  ICLR17_REQUIRE(log2_g >= 0 && log2_g <= 4, ICLR17_EINVAL,
                 "dequantise_step_map: log2 of the block edge is %d (0..4)", log2_g);
  Ladder st;
  if (!ladder_of("dequantise_step_map", steps, st)) return ICLR17_EINVAL;
  const long n = (long)B * h * w * N;
  hipLaunchKernelGGL(dequantise_step_map_kernel, dim3(elementwise_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, y_hat, n, N, geo_of(h, w, log2_g),
                     (const unsigned char*)indices, st, y_deq);
  return check_launch("dequantise_step_map");
}

int iclr17_rate_sweep_offsets(const float* y, int B, int h, int w, int N,
                              const float* rate_packed, const float* steps, const int8_t* offsets,
                              int log2_g, double* partial, double* bits, void* stream) {
  ICLR17_REQUIRE(y && rate_packed && steps && offsets && partial && bits, ICLR17_EINVAL,
                 "rate_sweep_offsets: null pointer");
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "rate_sweep_offsets: bad shape B=%d h=%d w=%d N=%d", B, h, w, N);
  ICLR17_REQUIRE(log2_g >= 0 && log2_g <= 4, ICLR17_EINVAL,
                 "rate_sweep_offsets: log2 of the block edge is %d (0..4)", log2_g);
  Ladder st;
  if (!ladder_of("rate_sweep_offsets", steps, st)) return ICLR17_EINVAL;
  const size_t shm = ((size_t)kRateRows * N + (size_t)kLadder * kSweepThreads) * sizeof(float);
  ICLR17_REQUIRE(shm <= 64 * 1024 - sizeof(float) * 5 * kLadder, ICLR17_EUNSUPPORTED,
                 "rate_sweep_offsets: N=%d needs %zu bytes of LDS", N, shm);
  const int chunks = iclr17_rate_sweep_partials(h, w, N);
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks * kLadder < (1L << 31), ICLR17_EUNSUPPORTED,
                 "rate_sweep_offsets: %ld workgroups x %d bases", blocks, kLadder);
  hipLaunchKernelGGL(rate_sweep_offsets_kernel, dim3((unsigned)blocks), dim3(kSweepThreads), shm,
                     (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, st,
                     geo_of(h, w, log2_g), (const signed char*)offsets, partial, chunks);
  const int rc = check_launch("rate_sweep_offsets");
  if (rc) return rc;
  // bits[b][s] = Σ_chunk partial[b][s][chunk], in reduce_partials' fixed order
  return iclr17_reduce_partials(partial, B * kLadder, chunks, bits, nullptr, 1.0, stream);
}

}  // extern "C"
