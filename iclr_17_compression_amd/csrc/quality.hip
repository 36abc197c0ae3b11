// Quality targets: the device half of a PSNR search along the step ladder.
//
//   quantise_steps     quantise_step with a step per image: ŷ = rintf(y/Δ_b) and Δ_b·ŷ, the same
//                      expressions and the same status bits, so that one launch probes every image
//                      of a batch at a ladder index of its own
//   distortion_sweep   E[b][s] = Σ w[c]·e², e = fmaf(Δ_s, rintf(v/Δ_s), −v), for up to 32 steps
//                      from ONE read of y: the weighted squared quantisation error of the latent,
//                      the distortion half of rate_sweep
//
// The sweep has rate_sweep's structure (ratectl.hip): the same 4096-element chunks and thread →
// element map, fp32 per thread and wave, float64 across the waves, iclr17_reduce_partials for the
// chunks; no atomics, bitwise reproducible and independent of the batch. A step costs a divide, a
// rint, an fma, two products and an add, so the step loop is unrolled and the 32 accumulators stay
// in registers: rate_sweep's LDS accumulators exist for the size of its inlined rate model, which
// this kernel does not have.
#include <math.h>

#include "common.h"

namespace iclr17 {
namespace {

constexpr int kSweepMax = 32;        // steps per launch (ratectl.hip)
constexpr int kSweepChunk = 4096;    // latents per partial: iclr17_rate_sweep_partials' chunk
constexpr int kSweepThreads = 256;

struct Steps {
  float d[kSweepMax];
};

enum : int { ST_NAN = 1, ST_RANGE = 2 };

// grid (blocks per image, B): block (x, b) strides image b's per_image elements
__global__ void __launch_bounds__(256) quantise_steps_kernel(
    const float* __restrict__ y, long per_image, const float* __restrict__ steps,
    float* __restrict__ y_hat, float* __restrict__ y_deq, int* __restrict__ status) {
  const int b = blockIdx.y;
  const float d = steps[b];
  const long base = (long)b * per_image;
  int bad = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per_image; i += (long)gridDim.x * 256) {
    const float q = rintf(y[base + i] / d);
    if (!(q == q)) bad |= ST_NAN;
    else if (fabsf(q) > 32767.f) bad |= ST_RANGE;
    if (y_hat) y_hat[base + i] = q;
    y_deq[base + i] = d * q;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if ((threadIdx.x & 63) == 0 && bad) atomicOr(status, bad);
}

// One workgroup per (image, 4096-element chunk of its NHWC latent); a thread holds one element
// and its channel's weight and runs the unrolled step loop on register accumulators.
// partial[b][s][chunk].
__global__ void __launch_bounds__(kSweepThreads) distortion_sweep_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ w, Steps st,
    int S, double* __restrict__ partial, int chunks) {
  __shared__ float red[4][kSweepMax];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const long lo = (long)ch * kSweepChunk;
  const long hi = lo + kSweepChunk < per_image ? lo + kSweepChunk : per_image;
  float acc[kSweepMax];
#pragma unroll
  for (int s = 0; s < kSweepMax; ++s) acc[s] = 0.f;
  for (long j = lo + tid; j < hi; j += kSweepThreads) {
    const float v = y[(long)b * per_image + j];
    const float wc = w[(int)(j % C)];
#pragma unroll
    for (int s = 0; s < kSweepMax; ++s) {
      if (s < S) {   // uniform
        const float d = st.d[s];
        const float e = fmaf(d, rintf(v / d), -v);
        acc[s] += wc * (e * e);
      }
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int s = 0; s < kSweepMax; ++s) {
    if (s < S) {
      const float t = wave_sum(acc[s]);
      if (lane == 0) red[wave][s] = t;
    }
  }
  __syncthreads();
  if (tid < S) {
    double t = 0.0;
    for (int k = 0; k < 4; ++k) t += (double)red[k][tid];
    partial[((long)b * S + tid) * chunks + ch] = t;
  }
}

bool good_step(float d) { return isfinite(d) && d > 0.f; }

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_quantise_steps(const float* y, int B, int64_t per_image, const float* steps_dev,
                          float* y_hat, float* y_deq, int32_t* status, void* stream) {
  ICLR17_REQUIRE(y && steps_dev && y_deq && status, ICLR17_EINVAL, "quantise_steps: null pointer");
  ICLR17_REQUIRE(B > 0 && B <= 65535 && per_image > 0, ICLR17_EINVAL,
                 "quantise_steps: bad shape B=%d per_image=%lld", B, (long long)per_image);
  const long blocks = ((long)per_image + 255) / 256;
  const dim3 grid((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)B);
  hipLaunchKernelGGL(quantise_steps_kernel, grid, dim3(256), 0, (hipStream_t)stream, y,
                     (long)per_image, steps_dev, y_hat, y_deq, (int*)status);
  return check_launch("quantise_steps");
}

int iclr17_distortion_sweep(const float* y, int B, int h, int w, int N, const float* weights,
                            const float* steps, int S, double* partial, double* out,
                            void* stream) {
  ICLR17_REQUIRE(y && weights && steps && partial && out, ICLR17_EINVAL,
                 "distortion_sweep: null pointer");
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "distortion_sweep: bad shape B=%d h=%d w=%d N=%d", B, h, w, N);
  ICLR17_REQUIRE(S >= 1 && S <= kSweepMax, ICLR17_EINVAL,
                 "distortion_sweep: S=%d steps (1..%d)", S, kSweepMax);
  Steps st;
  for (int s = 0; s < kSweepMax; ++s) st.d[s] = 1.0f;
  for (int s = 0; s < S; ++s) {
    ICLR17_REQUIRE(good_step(steps[s]), ICLR17_EINVAL,
                   "distortion_sweep: step %d (%g) is not finite and positive", s,
                   (double)steps[s]);
    st.d[s] = steps[s];
  }
  const int chunks = iclr17_rate_sweep_partials(h, w, N);
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks * S < (1L << 31), ICLR17_EUNSUPPORTED,
                 "distortion_sweep: %ld workgroups x %d steps", blocks, S);
  hipLaunchKernelGGL(distortion_sweep_kernel, dim3((unsigned)blocks), dim3(kSweepThreads), 0,
                     (hipStream_t)stream, y, N, (long)N * h * w, weights, st, S, partial, chunks);
  const int rc = check_launch("distortion_sweep");
  if (rc) return rc;
  // out[b][s] = Σ_chunk partial[b][s][chunk], in reduce_partials' fixed order
  return iclr17_reduce_partials(partial, B * S, chunks, out, nullptr, 1.0, stream);
}

}  // extern "C"
