// Training along the quantiser-step ladder: the quantiser / rate part of a training step whose
// images each have a step of their own.
//
// The coder of §0f codes rint(y/Δ) with the step pack (row 0 of the packed rate parameters · Δ)
// and synthesises from Δ·rint(y/Δ). The training proxy replaces the rounding by noise, per image b:
//
//   z = y/Δ_b + u        (fp32 IEEE divide, then fp32 add; u ∈ [-½, ½))
//   ỹ = Δ_b · z          (one fp32 product: what the synthesis transform receives)
//   bits_b = Σ element_bits(z, step pack of Δ_b)
//
//   step_noise_rate       z, ỹ and the per-chunk bit partials of every image, one pass over y
//   step_noise_rate_bwd   ∂L/∂y = ∂L/∂ỹ + g_bits[b] · ∂bits/∂z / Δ_b and the rate-parameter
//                         partials in the [T][11][C] slots iclr17_rate_param_grad reads
//   grad_recon_images     grad_recon with the MSE weight per image
//
// The forward's partials are rate_bits' own on z (ladder.h's chunks and its tail of one sum: the
// same thread → element map, fp32 per thread and wave, float64 across the waves), laid out
// [B][chunks] for iclr17_reduce_partials; the backward's rows are written by the thread that owns
// the channel. No atomics anywhere: bitwise reproducible.
#include <math.h>

#include "ladder.h"

namespace iclr17 {
namespace {

constexpr int kStepBwdPixels = 16;   // pixels per workgroup (and per partial row) of the backward

// One workgroup per (image, 4096-element chunk of its NHWC latent). noise is NCHW, as
// ImageCompressor._latent_noise draws it and conv3's noise quantiser reads it.
__global__ void __launch_bounds__(kThreads) step_noise_rate_kernel(
    const float* __restrict__ y, const float* __restrict__ noise, int C, int HW,
    const float* __restrict__ steps, const float* __restrict__ rp, float* __restrict__ z_out,
    float* __restrict__ y_deq, double* __restrict__ partial, int chunks) {
  extern __shared__ float sp[];   // [11][C]
  const long per_image = (long)C * HW;
  const Chunk k = sweep_chunk(chunks, per_image);
  const float d = steps[k.b];
  stage_step_pack(rp, C, d, sp);
  float s = 0.f;
  for (long j = k.lo + threadIdx.x; j < k.hi; j += kThreads) {
    const int c = (int)(j % C);
    const long p = j / C;
    const long i = (long)k.b * per_image + j;
    const float z = y[i] / d + noise[(long)k.b * per_image + (long)c * HW + p];
    z_out[i] = z;
    y_deq[i] = d * z;
    s += element_bits(z, sp, C, c);
  }
  chunk_sum_store(s, k, chunks, partial);
}

// One workgroup per (image, block of 16 pixels). Thread t owns the channels t, t + blockDim, …:
// for each it walks the block's pixels (a wave reads 64 consecutive channels of one pixel) with
// the channel's 11 accumulators in registers and stores them itself: rate_partial[row][k][c],
// row = b · blocks + block, slot 0 times Δ_b (∂/∂softplus(h1) = Δ · ∂/∂(softplus(h1)·Δ)).
__global__ void __launch_bounds__(kThreads) step_noise_rate_bwd_kernel(
    const float* __restrict__ z, const float* __restrict__ g_deq, int C, int HW,
    const float* __restrict__ steps, const float* __restrict__ rp, const float* __restrict__ g_bits,
    float* __restrict__ g_y, float* __restrict__ rate_partial, int blocks) {
  extern __shared__ float sp[];   // [11][C]
  const int b = blockIdx.x / blocks, blk = blockIdx.x % blocks;
  const float d = steps[b];
  stage_step_pack(rp, C, d, sp);
  const float gsc = g_bits[b];
  const int p0 = blk * kStepBwdPixels;
  const int p1 = p0 + kStepBwdPixels < HW ? p0 + kStepBwdPixels : HW;
  float* row = rate_partial + (long)blockIdx.x * kRateRows * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float pg[kRateRows];
#pragma unroll
    for (int k = 0; k < kRateRows; ++k) pg[k] = 0.f;
    for (int p = p0; p < p1; ++p) {
      const long i = ((long)b * HW + p) * C + c;
      const float dz = rate_bwd_element(z[i], sp, C, c, gsc, pg);
      g_y[i] = g_deq[i] + dz / d;
    }
    row[c] = pg[0] * d;
#pragma unroll
    for (int k = 1; k < kRateRows; ++k) row[k * C + c] = pg[k];
  }
}

// grad_recon_kernel (aux.hip) with the weight of image b's mean((recon − x)²) in g_mse[b].
__global__ void grad_recon_images_kernel(const float* __restrict__ recon,
                                         const float* __restrict__ x,
                                         const float* __restrict__ g_mse,
                                         const float* __restrict__ g_clip, long per_image, long n,
                                         float numel, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const float r = recon[i];
    float g = 0.0f;
    if (g_mse != nullptr) {
      const float gm = g_mse[i / per_image] / numel;
      g = gm * (2.0f * (r - x[i]));
    }
    if (g_clip != nullptr && r >= 0.0f && r <= 1.0f) g = g + g_clip[i];
    out[i] = g;
  }
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_step_noise_rate(const float* y, const float* noise, int B, int h, int w, int N,
                           const float* steps_dev, const float* rate_packed, float* z,
                           float* y_deq, double* bits_partial, void* stream) {
  ICLR17_REQUIRE(y && noise && steps_dev && rate_packed && z && y_deq && bits_partial,
                 ICLR17_EINVAL, "step_noise_rate: null pointer");
  size_t shm;
  int rc = check_step_shape("step_noise_rate", B, h, w, N, &shm);
  if (rc) return rc;
  const int chunks = iclr17_rate_bits_partials(N, h, w);   // rate_bits' own chunks
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks < (1L << 31), ICLR17_EUNSUPPORTED, "step_noise_rate: %ld workgroups",
                 blocks);
  hipLaunchKernelGGL(step_noise_rate_kernel, dim3((unsigned)blocks), dim3(kThreads), shm,
                     (hipStream_t)stream, y, noise, N, h * w, steps_dev, rate_packed, z, y_deq,
                     bits_partial, chunks);
  return check_launch("step_noise_rate");
}

int iclr17_step_rate_bwd_partials(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return (int)(((long)h * w + kStepBwdPixels - 1) / kStepBwdPixels);
}

int iclr17_step_noise_rate_bwd(const float* z, const float* g_deq, int B, int h, int w, int N,
                               const float* steps_dev, const float* rate_packed,
                               const float* g_bits, float* g_y, float* rate_partial,
                               void* stream) {
  ICLR17_REQUIRE(z && g_deq && steps_dev && rate_packed && g_bits && g_y && rate_partial,
                 ICLR17_EINVAL, "step_noise_rate_bwd: null pointer");
  size_t shm;
  int rc = check_step_shape("step_noise_rate_bwd", B, h, w, N, &shm);
  if (rc) return rc;
  const int per = iclr17_step_rate_bwd_partials(h, w);
  const long blocks = (long)B * per;
  ICLR17_REQUIRE(blocks < (1L << 31), ICLR17_EUNSUPPORTED, "step_noise_rate_bwd: %ld workgroups",
                 blocks);
  // one thread per channel, whole waves, at most 256 (more channels: a thread owns several)
  const int threads = N >= kThreads ? kThreads : (N + 63) / 64 * 64;
  hipLaunchKernelGGL(step_noise_rate_bwd_kernel, dim3((unsigned)blocks), dim3(threads), shm,
                     (hipStream_t)stream, z, g_deq, N, h * w, steps_dev, rate_packed, g_bits, g_y,
                     rate_partial, per);
  return check_launch("step_noise_rate_bwd");
}

int iclr17_grad_recon_images(const float* recon, const float* x, const float* g_mse,
                             const float* g_clip, int B, int64_t per_image, float* g_recon,
                             void* stream) {
  ICLR17_REQUIRE(recon && x && g_recon, ICLR17_EINVAL, "grad_recon_images: null pointer");
  ICLR17_REQUIRE(B > 0 && per_image > 0, ICLR17_EINVAL,
                 "grad_recon_images: bad shape B=%d per_image=%lld", B, (long long)per_image);
  const int64_t n = (int64_t)B * per_image;
  int64_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(grad_recon_images_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, recon, x, g_mse, g_clip, (long)per_image, (long)n,
                     (float)per_image, g_recon);
  return check_launch("grad_recon_images");
}

}  // extern "C"
