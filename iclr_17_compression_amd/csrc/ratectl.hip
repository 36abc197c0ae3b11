// Rate control by a scaled quantiser: many rates from one set of weights.
//
// With a step Δ the codec codes ŷ = rint(y/Δ) and synthesises from Δ·ŷ. The factorised model's
// first layer is v·softplus(h1) + b1 (common.h bitparm_cdf), so F(Δ·u) is the same function with
// row 0 of the packed [11][N] rate parameters multiplied by Δ: with that *step pack* the existing
// entropy_tables, rate_table, rate_bits and rANS kernels code the scaled alphabet unchanged.
//
//   pack_rate_step   the step pack of a pack (row 0 · Δ, one fp32 product per channel)
//   quantise_step    ŷ = rintf(y/Δ) and Δ·ŷ in one pass, with a status word (rans.hip's style)
//   dequantise_step  Δ·ŷ alone (the decoder's half)
//   rate_sweep       bits[b][s] = Σ element_bits(rintf(y/Δ_s), pack_s) for up to 32 steps from ONE
//                    read of y: what rate_bits(quantise_step(y, Δ_s), pack_s) gives per step
//   rate_sweep_offsets  the same kernel at all 32 base indices with a ladder offset per block of
//                    latent positions
//
// The quantisers are ladder.h's one body with a scalar step. The sweeps are one kernel over where
// the step comes from, in ladder.h's frame: their partials are rate_bits' own, term for term and
// in its order of addition, and iclr17_reduce_partials sums them.
#include <math.h>

#include "ladder.h"

namespace iclr17 {
namespace {

// Where the sweep's step of (element, s) comes from. stage(sd) ends with the barrier that the
// kernel's LDS needs, steps(S) is the number of steps, of(b, p) what at(sd, s, ·) wants of the
// element at latent position p of image b.
struct SweepSteps {   // steps[s], read from the kernel argument
  Steps st;
  __device__ __forceinline__ void stage(float*) const { __syncthreads(); }
  __device__ __forceinline__ int steps(int S) const { return S; }
  __device__ __forceinline__ int of(int, long) const { return 0; }
  __device__ __forceinline__ float at(const float*, int s, int) const { return st.d[s]; }
};

// All 32 base indices s, an element's step the ladder's (in LDS) at clamp(s + off, 0, 31) with
// off its block's signed offset (i8 map, stepmap.hip's geometry). With zero offsets rate_sweep's
// 32-step result bit for bit; with one offset c for a whole image row s is its row clamp(s + c).
struct OffsetSteps {
  Steps st;
  MapGeo g;
  const signed char* __restrict__ off;
  __device__ __forceinline__ void stage(float* sd) const { stage_ladder(st, sd); }
  __device__ __forceinline__ int steps(int) const { return kLadder; }
  __device__ __forceinline__ int of(int b, long p) const {
    return off[map_entry(g, (long)b * g.hw + p)];
  }
  __device__ __forceinline__ float at(const float* sd, int s, int o) const {
    return sd[min(max(s + o, 0), kLadder - 1)];
  }
};

// One workgroup per (image, 4096-element chunk of its NHWC latent). LDS: the 11·C rate floats,
// staged once, then one fp32 accumulator per (step, thread), so that the step loop needs no
// unrolling (32 inlined copies of the model would not fit the instruction cache). A thread
// holds one element and its channel's 11 parameters in registers and loops the steps.
// partial[b][s][chunk].
template <class Look>
__global__ void __launch_bounds__(kThreads) rate_sweep_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ rp, Look look,
    int S, double* __restrict__ partial, int chunks) {
  extern __shared__ float lds[];
  __shared__ float red[4][kLadder];
  __shared__ float sd[kLadder];
  float* sp = lds;                         // [11][C]
  float* acc = lds + kRateRows * C;        // [S][256]
  const int tid = threadIdx.x;
  S = look.steps(S);
  for (int i = tid; i < kRateRows * C; i += kThreads) sp[i] = rp[i];
  for (int s = 0; s < S; ++s) acc[s * kThreads + tid] = 0.f;
  look.stage(sd);
  const Chunk k = sweep_chunk(chunks, per_image);
  for (long j = k.lo + tid; j < k.hi; j += kThreads) {
    const int c = (int)(j % C);
    const float v = y[(long)k.b * per_image + j];
    const int o = look.of(k.b, j / C);
    float p[kRateRows];
#pragma unroll
    for (int r = 0; r < kRateRows; ++r) p[r] = sp[r * C + c];
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      const float d = look.at(sd, s, o);
      const float z = rintf(v / d);
      acc[s * kThreads + tid] += bits_regs(z, p[0] * d, p);
    }
  }
  for (int s = 0; s < S; ++s) sweep_wave(red, k, s, acc[s * kThreads + tid]);
  sweep_store(red, S, k, chunks, partial);
}

__global__ void pack_rate_step_kernel(const float* __restrict__ rp, int C, float d,
                                      float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kRateRows * C) out[i] = i < C ? rp[i] * d : rp[i];
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_pack_rate_step(const float* rate_packed, int N, float step, float* step_packed,
                          void* stream) {
  ICLR17_REQUIRE(rate_packed && step_packed, ICLR17_EINVAL, "pack_rate_step: null pointer");
  ICLR17_REQUIRE(N > 0, ICLR17_EINVAL, "pack_rate_step: bad shape N=%d", N);
  ICLR17_REQUIRE(good_step(step), ICLR17_EINVAL,
                 "pack_rate_step: the step %g is not finite and positive", (double)step);
  hipLaunchKernelGGL(pack_rate_step_kernel, dim3((kRateRows * N + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, rate_packed, N, step, step_packed);
  return check_launch("pack_rate_step");
}

int iclr17_quantise_step(const float* y, int64_t n, float step, float* y_hat, float* y_deq,
                         int32_t* status, void* stream) {
  ICLR17_REQUIRE(y && y_hat && y_deq && status, ICLR17_EINVAL, "quantise_step: null pointer");
  ICLR17_REQUIRE(n > 0, ICLR17_EINVAL, "quantise_step: bad shape n=%lld", (long long)n);
  ICLR17_REQUIRE(good_step(step), ICLR17_EINVAL,
                 "quantise_step: the step %g is not finite and positive", (double)step);
  hipLaunchKernelGGL(quantise_kernel<OneStep>, dim3(elementwise_blocks(n)), dim3(kThreads), 0,
                     (hipStream_t)stream, y, (long)n, OneStep{step}, y_hat, y_deq, (int*)status);
  return check_launch("quantise_step");
}

int iclr17_dequantise_step(const float* y_hat, int64_t n, float step, float* y_deq, void* stream) {
  ICLR17_REQUIRE(y_hat && y_deq, ICLR17_EINVAL, "dequantise_step: null pointer");
  ICLR17_REQUIRE(n > 0, ICLR17_EINVAL, "dequantise_step: bad shape n=%lld", (long long)n);
  ICLR17_REQUIRE(good_step(step), ICLR17_EINVAL,
                 "dequantise_step: the step %g is not finite and positive", (double)step);
  hipLaunchKernelGGL(dequantise_kernel<OneStep>, dim3(elementwise_blocks(n)), dim3(kThreads), 0,
                     (hipStream_t)stream, y_hat, (long)n, OneStep{step}, y_deq);
  return check_launch("dequantise_step");
}

int iclr17_rate_sweep_partials(int h, int w, int N) {
  if (h <= 0 || w <= 0 || N <= 0) return 0;
  const long n = (long)N * h * w;
  return (int)((n + kChunk - 1) / kChunk);
}

int iclr17_rate_sweep(const float* y, int B, int h, int w, int N, const float* rate_packed,
                      const float* steps, int S, double* partial, double* bits, void* stream) {
  ICLR17_REQUIRE(y && rate_packed && steps && partial && bits, ICLR17_EINVAL,
                 "rate_sweep: null pointer");
  const SweepCall c{"rate_sweep", B, h, w, N, nullptr, steps, S, partial, bits, stream};
  return run_sweep(c, [&](const Steps& st, int chunks, unsigned blocks) -> int {
    const size_t shm = ((size_t)kRateRows * N + (size_t)S * kThreads) * sizeof(float);
    ICLR17_REQUIRE(shm <= 64 * 1024 - sizeof(float) * 4 * kLadder, ICLR17_EUNSUPPORTED,
                   "rate_sweep: N=%d needs %zu bytes of LDS", N, shm);
    hipLaunchKernelGGL(rate_sweep_kernel<SweepSteps>, dim3(blocks), dim3(kThreads), shm,
                       (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, SweepSteps{st}, S,
                       partial, chunks);
    return 0;
  });
}

int iclr17_rate_sweep_offsets(const float* y, int B, int h, int w, int N,
                              const float* rate_packed, const float* steps, const int8_t* offsets,
                              int log2_g, double* partial, double* bits, void* stream) {
  ICLR17_REQUIRE(y && rate_packed && steps && offsets && partial && bits, ICLR17_EINVAL,
                 "rate_sweep_offsets: null pointer");
  const SweepCall c{"rate_sweep_offsets", B, h, w, N, &log2_g, steps, kLadder, partial, bits,
                    stream};
  return run_sweep(c, [&](const Steps& st, int chunks, unsigned blocks) -> int {
    const size_t shm = ((size_t)kRateRows * N + (size_t)kLadder * kThreads) * sizeof(float);
    ICLR17_REQUIRE(shm <= 64 * 1024 - sizeof(float) * 5 * kLadder, ICLR17_EUNSUPPORTED,
                   "rate_sweep_offsets: N=%d needs %zu bytes of LDS", N, shm);
    const OffsetSteps look{st, geo_of(h, w, log2_g), (const signed char*)offsets};
    hipLaunchKernelGGL(rate_sweep_kernel<OffsetSteps>, dim3(blocks), dim3(kThreads), shm,
                       (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, look, kLadder,
                       partial, chunks);
    return 0;
  });
}

}  // extern "C"
