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
//
// The sweep's partials are rate_bits' own, term for term and in its order of addition (the same
// 4096-element chunks, the same thread → element map, fp32 per thread and wave, float64 across
// the waves), and iclr17_reduce_partials sums them: no atomics, bitwise reproducible.
#include <math.h>

#include "common.h"

namespace iclr17 {
namespace {

constexpr int kSweepMax = 32;        // steps per launch
constexpr int kSweepChunk = 4096;    // latents per partial: aux.hip's kRateChunk
constexpr int kSweepThreads = 256;

struct Steps {
  float d[kSweepMax];
};

// One workgroup per (image, 4096-element chunk of its NHWC latent). LDS: the 11·C rate floats,
// staged once, then one fp32 accumulator per (step, thread), so that the step loop needs no
// unrolling (32 inlined copies of the model would not fit the instruction cache). A thread
// holds one element and its channel's 11 parameters in registers and loops the steps.
// partial[b][s][chunk].
__global__ void __launch_bounds__(kSweepThreads) rate_sweep_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ rp, Steps st,
    int S, double* __restrict__ partial, int chunks) {
  extern __shared__ float lds[];
  __shared__ float red[4][kSweepMax];
  float* sp = lds;                         // [11][C]
  float* acc = lds + kRateRows * C;        // [S][256]
  const int tid = threadIdx.x;
  for (int i = tid; i < kRateRows * C; i += kSweepThreads) sp[i] = rp[i];
  for (int s = 0; s < S; ++s) acc[s * kSweepThreads + tid] = 0.f;
  __syncthreads();
  const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const long lo = (long)ch * kSweepChunk;
  const long hi = lo + kSweepChunk < per_image ? lo + kSweepChunk : per_image;
  for (long j = lo + tid; j < hi; j += kSweepThreads) {
    const int c = (int)(j % C);
    const float v = y[(long)b * per_image + j];
    float p[kRateRows];
#pragma unroll
    for (int k = 0; k < kRateRows; ++k) p[k] = sp[k * C + c];
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
      const float d = st.d[s];
      const float z = rintf(v / d);
      acc[s * kSweepThreads + tid] += bits_regs(z, p[0] * d, p);
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
  for (int s = 0; s < S; ++s) {
    const float t = wave_sum(acc[s * kSweepThreads + tid]);
    if (lane == 0) red[wave][s] = t;
  }
  __syncthreads();
  if (tid < S) {
    double t = 0.0;
    for (int w = 0; w < 4; ++w) t += (double)red[w][tid];
    partial[((long)b * S + tid) * chunks + ch] = t;
  }
}

enum : int { ST_NAN = 1, ST_RANGE = 2 };

__global__ void __launch_bounds__(256) quantise_step_kernel(const float* __restrict__ y, long n,
                                                            float d, float* __restrict__ y_hat,
                                                            float* __restrict__ y_deq,
                                                            int* __restrict__ status) {
  int bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
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

__global__ void __launch_bounds__(256) dequantise_step_kernel(const float* __restrict__ y_hat,
                                                              long n, float d,
                                                              float* __restrict__ y_deq) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
    y_deq[i] = d * y_hat[i];
}

__global__ void pack_rate_step_kernel(const float* __restrict__ rp, int C, float d,
                                      float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kRateRows * C) out[i] = i < C ? rp[i] * d : rp[i];
}

bool good_step(float d) { return isfinite(d) && d > 0.f; }

unsigned elementwise_blocks(long n) {
  const long blocks = (n + 255) / 256;
  return (unsigned)(blocks > 65536 ? 65536 : blocks);
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
  hipLaunchKernelGGL(quantise_step_kernel, dim3(elementwise_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, y, (long)n, step, y_hat, y_deq, (int*)status);
  return check_launch("quantise_step");
}

int iclr17_dequantise_step(const float* y_hat, int64_t n, float step, float* y_deq, void* stream) {
  ICLR17_REQUIRE(y_hat && y_deq, ICLR17_EINVAL, "dequantise_step: null pointer");
  ICLR17_REQUIRE(n > 0, ICLR17_EINVAL, "dequantise_step: bad shape n=%lld", (long long)n);
  ICLR17_REQUIRE(good_step(step), ICLR17_EINVAL,
                 "dequantise_step: the step %g is not finite and positive", (double)step);
  hipLaunchKernelGGL(dequantise_step_kernel, dim3(elementwise_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, y_hat, (long)n, step, y_deq);
  return check_launch("dequantise_step");
}

int iclr17_rate_sweep_partials(int h, int w, int N) {
  if (h <= 0 || w <= 0 || N <= 0) return 0;
  const long n = (long)N * h * w;
  return (int)((n + kSweepChunk - 1) / kSweepChunk);
}

int iclr17_rate_sweep(const float* y, int B, int h, int w, int N, const float* rate_packed,
                      const float* steps, int S, double* partial, double* bits, void* stream) {
  ICLR17_REQUIRE(y && rate_packed && steps && partial && bits, ICLR17_EINVAL,
                 "rate_sweep: null pointer");
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "rate_sweep: bad shape B=%d h=%d w=%d N=%d", B, h, w, N);
  ICLR17_REQUIRE(S >= 1 && S <= kSweepMax, ICLR17_EINVAL,
                 "rate_sweep: S=%d steps (1..%d)", S, kSweepMax);
  Steps st;
  for (int s = 0; s < kSweepMax; ++s) st.d[s] = 1.0f;
  for (int s = 0; s < S; ++s) {
    ICLR17_REQUIRE(good_step(steps[s]), ICLR17_EINVAL,
                   "rate_sweep: step %d (%g) is not finite and positive", s, (double)steps[s]);
    st.d[s] = steps[s];
  }
  const size_t shm = ((size_t)kRateRows * N + (size_t)S * kSweepThreads) * sizeof(float);
  ICLR17_REQUIRE(shm <= 64 * 1024 - sizeof(float) * 4 * kSweepMax, ICLR17_EUNSUPPORTED,
                 "rate_sweep: N=%d needs %zu bytes of LDS", N, shm);
  const int chunks = iclr17_rate_sweep_partials(h, w, N);
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks * S < (1L << 31), ICLR17_EUNSUPPORTED,
                 "rate_sweep: %ld workgroups x %d steps", blocks, S);
  hipLaunchKernelGGL(rate_sweep_kernel, dim3((unsigned)blocks), dim3(kSweepThreads), shm,
                     (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, st, S, partial,
                     chunks);
  const int rc = check_launch("rate_sweep");
  if (rc) return rc;
  // bits[b][s] = Σ_chunk partial[b][s][chunk], in reduce_partials' fixed order
  return iclr17_reduce_partials(partial, B * S, chunks, bits, nullptr, 1.0, stream);
}

}  // extern "C"
