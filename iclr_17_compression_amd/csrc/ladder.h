// What the step-ladder units share (ratectl.hip, stepmap.hip, rdoq.hip, quality.hip and the forward
// of steptrain.hip): the quantiser's lines and the frame of a sweep, each written once.
//
//   the quantiser   ŷ = rintf(y/Δ) with its two status bits, the stores of ŷ and Δ·ŷ, and the
//                   status word. quantise_kernel / dequantise_kernel are one body over a *step
//                   source*, which says where an element's Δ comes from: OneStep (a scalar),
//                   ImageSteps (steps[b]) or MapSteps (the ladder in LDS at the index of the
//                   element's block). quantise_rdo (rdoq.hip) puts its pick between the same
//                   flagging and storing functions.
//   a sweep         one workgroup per (image, 4096-element chunk of its NHWC latent): sweep_chunk
//                   gives the chunk, sweep_wave / sweep_store are the tail (fp32 per thread,
//                   wave_sum, float64 over waves 0..3, partial[b][s][chunk]) and run_sweep is the
//                   host's sequence up to iclr17_reduce_partials. chunk_sum_store is the tail of
//                   one sum.
//   a step pack     the rate parameters with row 0 · Δ_b staged in LDS (stage_step_pack) and the
//                   shape checks of a kernel that stages one: steptrain.hip and refine.hip.
//
// The chunk is aux.hip's kRateChunk and the thread → element map is rate_bits_kernel's, so a
// sweep's partials are rate_bits' own, term for term and in its order of addition: no atomics in a
// sum, bitwise reproducible, and an image's result does not depend on its batch.
#pragma once

#include <math.h>

#include "common.h"

namespace iclr17 {

constexpr int kLadder = 32;      // ladder steps: a sweep's steps per launch, a map's index range
constexpr int kChunk = 4096;     // latents per partial
constexpr int kThreads = 256;
enum : int { ST_NAN = 1, ST_RANGE = 2 };   // the quantisers' status bits

struct Steps {   // up to 32 steps by value: a sweep's steps, a map's ladder
  float d[kLadder];
};

struct MapGeo {
  int hw, w;      // latent positions per image, latent width
  int mhw, mw;    // map entries per image, map width
  int lg;         // log2 of the block edge
};

// ------------------------------------------------------------------------------------ host
inline bool good_step(float d) { return isfinite(d) && d > 0.f; }

inline unsigned elementwise_blocks(long n) {
  const long blocks = (n + kThreads - 1) / kThreads;
  return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

// st = steps[0..S) and 1.0 beyond; the error set on a step that is not finite and positive
inline int fill_steps(const char* what, const float* steps, int S, Steps& st) {
  for (int s = 0; s < kLadder; ++s) st.d[s] = 1.0f;
  for (int s = 0; s < S; ++s) {
    ICLR17_REQUIRE(good_step(steps[s]), ICLR17_EINVAL,
                   "%s: step %d (%g) is not finite and positive", what, s, (double)steps[s]);
    st.d[s] = steps[s];
  }
  return 0;
}

inline int check_latent(const char* what, int B, int h, int w, int N) {
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "%s: bad shape B=%d h=%d w=%d N=%d", what, B, h, w, N);
  return 0;
}

inline int check_block(const char* what, int log2_g) {
  ICLR17_REQUIRE(log2_g >= 0 && log2_g <= 4, ICLR17_EINVAL,
                 "%s: log2 of the block edge is %d (0..4)", what, log2_g);
  return 0;
}

inline int check_count(const char* what, int S) {
  ICLR17_REQUIRE(S >= 1 && S <= kLadder, ICLR17_EINVAL, "%s: S=%d steps (1..%d)", what, S, kLadder);
  return 0;
}

inline MapGeo geo_of(int h, int w, int lg) {
  const int g = 1 << lg;
  const int mh = (h + g - 1) / g, mw = (w + g - 1) / g;
  return MapGeo{h * w, w, mh * mw, mw, lg};
}

// A sweep entry point after its pointer check. log2_g: the block edge of its map, null without
// one (a mapped sweep's steps are its bases).
struct SweepCall {
  const char* what;
  int B, h, w, N;
  const int* log2_g;
  const float* steps;
  int S;
  double *partial, *out;
  void* stream;
};

// The checks, the steps by value, the grid of (image, chunk) workgroups and its limit, then
// launch(st, chunks, blocks), which checks its LDS need, launches and returns 0 or the error's
// code; out[b][s] = Σ_chunk partial[b][s][chunk] in reduce_partials' fixed order.
template <class Launch>
int run_sweep(const SweepCall& c, Launch launch) {
  int rc = check_latent(c.what, c.B, c.h, c.w, c.N);
  if (!rc && c.log2_g) rc = check_block(c.what, *c.log2_g);
  if (!rc) rc = check_count(c.what, c.S);
  Steps st;
  if (!rc) rc = fill_steps(c.what, c.steps, c.S, st);
  if (rc) return rc;
  const int chunks = iclr17_rate_sweep_partials(c.h, c.w, c.N);
  const long blocks = (long)c.B * chunks;
  ICLR17_REQUIRE(blocks * c.S < (1L << 31), ICLR17_EUNSUPPORTED, "%s: %ld workgroups x %d %s",
                 c.what, blocks, c.S, c.log2_g ? "bases" : "steps");
  rc = launch(st, chunks, (unsigned)blocks);
  if (!rc) rc = check_launch(c.what);
  if (rc) return rc;
  return iclr17_reduce_partials(c.partial, c.B * c.S, chunks, c.out, nullptr, 1.0, c.stream);
}

// --------------------------------------------------------------------------------- step maps
// The latent of a canvas is h×w positions; a block is g×g of them (g = 2^lg) and a map has
// ⌈h/g⌉×⌈w/g⌉ entries per image, row-major. The map entry of latent position `pos`
// (b·h·w + i·w + j):
__device__ __forceinline__ long map_entry(const MapGeo& g, long pos) {
  const long b = pos / g.hw;
  const int pix = (int)(pos - b * g.hw);
  const int i = pix / g.w, j = pix - i * g.w;
  return b * g.mhw + (long)(i >> g.lg) * g.mw + (j >> g.lg);
}

__device__ __forceinline__ void stage_ladder(const Steps& st, float* sd) {
  if (threadIdx.x < kLadder) sd[threadIdx.x] = st.d[threadIdx.x];
  __syncthreads();
}

// ------------------------------------------------------------------------------ the quantiser
// the status bits of a level r = rintf(y/Δ): what the entropy coder cannot carry
__device__ __forceinline__ int level_status(float r) {
  return !(r == r) ? ST_NAN : fabsf(r) > 32767.f ? ST_RANGE : 0;
}

// ŷ[i] = q and Δ·ŷ; with null_hat (a constant where it is called) y_hat may be null. The kernels'
// parameters carry __restrict__; repeated on these inlined helpers it keeps the compiler from
// vectorising the quantisers' loops.
__device__ __forceinline__ void store_level(float q, float d, long i, float* y_hat, float* y_deq,
                                            bool null_hat = false) {
  if (!null_hat || y_hat) y_hat[i] = q;
  y_deq[i] = d * q;
}

// element i, value v at step d; returns its status bits
__device__ __forceinline__ int quantise_element(float v, float d, long i, float* y_hat,
                                                float* y_deq, bool null_hat) {
  const float q = rintf(v / d);
  const int bad = level_status(q);
  store_level(q, d, i, y_hat, y_deq, null_hat);
  return bad;
}

// the OR of a wave's status bits into the status word
__device__ __forceinline__ void report_status(int bad, int* __restrict__ status) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(status, bad);
}

// Step sources. stage(sd) runs once before the loop (sd: 32 floats of LDS for a source that wants
// them), base(n) is the first element of the block's range of n, at(sd, i) element i's step;
// kNullHat: its entry point takes a null ŷ.
struct OneStep {
  static constexpr bool kNullHat = false;
  float d;
  __device__ __forceinline__ void stage(float*) const {}
  __device__ __forceinline__ long base(long) const { return 0; }
  __device__ __forceinline__ float at(const float*, long) const { return d; }
};

struct ImageSteps {   // grid (blocks per image, B): block (x, b) strides image b's n elements
  static constexpr bool kNullHat = true;
  const float* __restrict__ steps;
  __device__ __forceinline__ void stage(float*) const {}
  __device__ __forceinline__ long base(long n) const { return (long)blockIdx.y * n; }
  __device__ __forceinline__ float at(const float*, long) const { return steps[blockIdx.y]; }
};

struct MapSteps {   // ladder[idx[the block of the element's position]], C channels a position
  static constexpr bool kNullHat = false;
  int C;
  MapGeo g;
  const unsigned char* __restrict__ idx;
  Steps st;
  __device__ __forceinline__ void stage(float* sd) const { stage_ladder(st, sd); }
  __device__ __forceinline__ long base(long) const { return 0; }
  __device__ __forceinline__ float at(const float* sd, long i) const {
    return sd[idx[map_entry(g, i / C)] & (kLadder - 1)];
  }
};

template <class Src>
__global__ void __launch_bounds__(kThreads) quantise_kernel(const float* __restrict__ y, long n,
                                                            Src src, float* __restrict__ y_hat,
                                                            float* __restrict__ y_deq,
                                                            int* __restrict__ status) {
  __shared__ float sd[kLadder];
  src.stage(sd);
  const long base = src.base(n);
  const long stride = (long)gridDim.x * kThreads;
  int bad = 0;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride)
    bad |= quantise_element(y[base + i], src.at(sd, base + i), base + i, y_hat, y_deq,
                            Src::kNullHat);
  report_status(bad, status);
}

// Δ·ŷ alone: the decoder's half
template <class Src>
__global__ void __launch_bounds__(kThreads) dequantise_kernel(const float* __restrict__ y_hat,
                                                              long n, Src src,
                                                              float* __restrict__ y_deq) {
  __shared__ float sd[kLadder];
  src.stage(sd);
  const long base = src.base(n);
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads)
    y_deq[base + i] = src.at(sd, base + i) * y_hat[base + i];
}

// ------------------------------------------------------------------------------ the sweep frame
struct Chunk {
  int b, ch;        // image, chunk of the image
  long lo, hi;      // the chunk's elements of the image's per_image
  int lane, wave;   // of this thread
};

__device__ __forceinline__ Chunk sweep_chunk(int chunks, long per_image) {
  Chunk k;
  k.b = blockIdx.x / chunks;
  k.ch = blockIdx.x % chunks;
  k.lo = (long)k.ch * kChunk;
  k.hi = k.lo + kChunk < per_image ? k.lo + kChunk : per_image;
  k.lane = threadIdx.x & 63;
  k.wave = threadIdx.x >> 6;
  return k;
}

// The tail of a sum per step: sweep_wave for every step s with the thread's fp32 sum v, then
// sweep_store (its barrier ends them): float64 over waves 0..3 into partial[b][s][chunk].
template <int SMAX>
__device__ __forceinline__ void sweep_wave(float (&red)[4][SMAX], const Chunk& k, int s, float v) {
  const float t = wave_sum(v);
  if (k.lane == 0) red[k.wave][s] = t;
}

template <int SMAX>
__device__ __forceinline__ void sweep_store(const float (&red)[4][SMAX], int S, const Chunk& k,
                                            int chunks, double* __restrict__ partial) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid < S) {
    double t = 0.0;
    for (int w = 0; w < 4; ++w) t += (double)red[w][tid];
    partial[((long)k.b * S + tid) * chunks + k.ch] = t;
  }
}

// the tail of one sum: partial[b][chunk]
__device__ __forceinline__ void chunk_sum_store(float v, const Chunk& k, int chunks,
                                                double* __restrict__ partial) {
  __shared__ float red[4][1];
  sweep_wave(red, k, 0, v);
  sweep_store(red, 1, k, chunks, partial);
}

// ------------------------------------------------------------------------------ step packs
constexpr size_t kStepLdsMax = 64 * 1024;

// The step pack of image b in LDS: the [11][C] rate floats with row 0 · Δ_b, the fp32 product
// pack_rate_step_kernel (ratectl.hip) makes. Shared by steptrain.hip and refine.hip.
__device__ __forceinline__ void stage_step_pack(const float* __restrict__ rp, int C, float d,
                                                float* __restrict__ sp) {
  for (int i = threadIdx.x; i < kRateRows * C; i += blockDim.x) sp[i] = i < C ? rp[i] * d : rp[i];
  __syncthreads();
}

// the shape checks of a kernel that stages a step pack; *shm: its LDS bytes
inline int check_step_shape(const char* what, int B, int h, int w, int N, size_t* shm) {
  const int rc = check_latent(what, B, h, w, N);
  if (rc) return rc;
  *shm = (size_t)kRateRows * N * sizeof(float);
  ICLR17_REQUIRE(*shm <= kStepLdsMax - 64, ICLR17_EUNSUPPORTED, "%s: N=%d needs %zu bytes of LDS",
                 what, N, *shm);
  ICLR17_REQUIRE((long)B * h * w * N < (1L << 40), ICLR17_EUNSUPPORTED, "%s: %ld latents", what,
                 (long)B * h * w * N);
  return 0;
}

}  // namespace iclr17
