// Quality targets: the device half of a PSNR search along the step ladder.
//
//   quantise_steps     quantise_step with a step per image: ŷ = rintf(y/Δ_b) and Δ_b·ŷ, the same
//                      expressions and the same status bits, so that one launch probes every image
//                      of a batch at a ladder index of its own
//   distortion_sweep   E[b][s] = Σ w[c]·e², e = fmaf(Δ_s, rintf(v/Δ_s), −v), for up to 32 steps
//                      from ONE read of y: the weighted squared quantisation error of the latent,
//                      the distortion half of rate_sweep
//
// quantise_steps is ladder.h's quantiser with ImageSteps as its step source. The sweep stands in
// ladder.h's frame (the chunks, the thread → element map and the wave sums of rate_sweep; the
// store of the partials is written out in the kernel, which says why) with a body of its own: a step costs a divide, a rint, an fma, two products and an add, so the step loop is
// unrolled and the 32 accumulators stay in registers. rate_sweep's LDS accumulators exist for the
// size of its inlined rate model, which this kernel does not have.
#include <math.h>

#include "ladder.h"

namespace iclr17 {
namespace {

// One workgroup per (image, 4096-element chunk of its NHWC latent); a thread holds one element
// and its channel's weight and runs the unrolled step loop on register accumulators.
// partial[b][s][chunk].
__global__ void __launch_bounds__(kThreads) distortion_sweep_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ w, Steps st,
    int S, double* __restrict__ partial, int chunks) {
  __shared__ float red[4][kLadder];
  const int tid = threadIdx.x;
  const Chunk k = sweep_chunk(chunks, per_image);
  float acc[kLadder];
#pragma unroll
  for (int s = 0; s < kLadder; ++s) acc[s] = 0.f;
  for (long j = k.lo + tid; j < k.hi; j += kThreads) {
    const float v = y[(long)k.b * per_image + j];
    const float wc = w[(int)(j % C)];
#pragma unroll
    for (int s = 0; s < kLadder; ++s) {
      if (s < S) {   // uniform
        const float d = st.d[s];
        const float e = fmaf(d, rintf(v / d), -v);
        acc[s] += wc * (e * e);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < kLadder; ++s) {
    if (s < S) sweep_wave(red, k, s, acc[s]);
  }
  // sweep_store's lines, written out: through the helper the compiler lays the element loop's
  // blocks out with a ladder of branches per element (profiles/step_kernels_refactor_ab.txt)
  __syncthreads();
  if (tid < S) {
    double t = 0.0;
    for (int q = 0; q < 4; ++q) t += (double)red[q][tid];
    partial[((long)k.b * S + tid) * chunks + k.ch] = t;
  }
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_quantise_steps(const float* y, int B, int64_t per_image, const float* steps_dev,
                          float* y_hat, float* y_deq, int32_t* status, void* stream) {
  ICLR17_REQUIRE(y && steps_dev && y_deq && status, ICLR17_EINVAL, "quantise_steps: null pointer");
  ICLR17_REQUIRE(B > 0 && B <= 65535 && per_image > 0, ICLR17_EINVAL,
                 "quantise_steps: bad shape B=%d per_image=%lld", B, (long long)per_image);
  const long blocks = ((long)per_image + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)(blocks > 4096 ? 4096 : blocks), (unsigned)B);
  hipLaunchKernelGGL(quantise_kernel<ImageSteps>, grid, dim3(kThreads), 0, (hipStream_t)stream, y,
                     (long)per_image, ImageSteps{steps_dev}, y_hat, y_deq, (int*)status);
  return check_launch("quantise_steps");
}

int iclr17_distortion_sweep(const float* y, int B, int h, int w, int N, const float* weights,
                            const float* steps, int S, double* partial, double* out,
                            void* stream) {
  ICLR17_REQUIRE(y && weights && steps && partial && out, ICLR17_EINVAL,
                 "distortion_sweep: null pointer");
  const SweepCall c{"distortion_sweep", B, h, w, N, nullptr, steps, S, partial, out, stream};
  return run_sweep(c, [&](const Steps& st, int chunks, unsigned blocks) -> int {
    hipLaunchKernelGGL(distortion_sweep_kernel, dim3(blocks), dim3(kThreads), 0,
                       (hipStream_t)stream, y, N, (long)N * h * w, weights, st, S, partial, chunks);
    return 0;
  });
}

}  // extern "C"
