// Latent refinement: the per-iteration kernels of an encoder that improves bits + λ·SSE of one
// image by gradient steps on its latent, the decoder unchanged.
//
//   refine_grad_recon   ∂(λ/3 · Σ (recon − ref/255)²)/∂recon over each image's own H×W of the
//                       canvas batch, exact zeros on the padding; ref is the packed uint8 originals
//   refine_step         one pass over the latent per iteration: the rate derivative at ŷ, the Adam
//                       update of y, and the NEXT iterate in the same pass: ŷ' = rintf(y'/Δ_b), Δ_b·ŷ',
//                       the status bits and the bit partials of ŷ'. Without a gradient it is the
//                       pass of iteration 0: the quantiser and the bits of y as it stands
//   refine_keep         J_b = bits_b + (λ_b/3)·SSE_b/255², and where J_b < best_J_b the iterate
//                       becomes the best: a one-workgroup launch decides per image, a second one
//                       copies the latents of the images that improved
//   refine_keep_msssim  the same decision for J_b = bits_b + λ_b·H_b·W_b·(1 − MS-SSIM_b)
//                       (the gradient of that distortion is msssim.hip's)
//
// refine_step stands in ladder.h's sweep frame (one workgroup per image and 4096-element chunk,
// the step pack of Δ_b in LDS, rate_bits' thread → element map and tail of one sum), so its bit
// partials are rate_bits' own on ŷ' with the step pack of Δ_b. No atomics in a sum: bitwise
// reproducible, and an image's result does not depend on its batch.
#include <math.h>

#include "ladder.h"

namespace iclr17 {
namespace {

// int64 descriptor row per image (imageio.hip): byte offset in the packed uint8 buffer, H, W, 0
enum : int { D_OFF = 0, D_H, D_W, D_N = 4 };

// One thread per canvas pixel, its three channels. The 8-bit side is read a byte at a time: any
// byte offset, nothing outside the image touched.
__global__ void __launch_bounds__(256) refine_grad_recon_kernel(
    const float* __restrict__ recon, const unsigned char* __restrict__ ref,
    const long* __restrict__ desc, const float* __restrict__ wt, int Hc, int Wc, long n,
    float* __restrict__ g) {
  const long plane = (long)Hc * Wc;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n; p += (long)gridDim.x * 256) {
    const long b = p / plane;
    const int pix = (int)(p - b * plane);
    const int i = pix / Wc, j = pix - i * Wc;
    const long* d = desc + b * D_N;
    const long H = d[D_H] < Hc ? d[D_H] : Hc, W = d[D_W] < Wc ? d[D_W] : Wc;   // inside the canvas
    const bool inside = i < H && j < W;
    const float wb = wt[b];
    const unsigned char* src = ref + d[D_OFF] + ((long)i * W + j) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long o = (b * 3 + c) * plane + pix;
      float v = 0.0f;
      if (inside) {
        const float x = (float)src[c] / 255.0f;   // the ingest's division
        v = wb * (2.0f * (recon[o] - x));
      }
      g[o] = v;
    }
  }
}

// UPDATE: the rate derivative at ŷ, g = g_ỹ + dz/Δ, Adam on (y, m, v) with the step size · Δ; then
// in both forms the quantiser of y and the bits of its level. y_hat / y_hat_out may be one
// buffer (an element is read and written by one thread), as may y_deq and nothing else.
template <bool UPDATE>
__global__ void __launch_bounds__(kThreads) refine_step_kernel(
    const float* y_hat, const float* __restrict__ g_deq, float* __restrict__ y,
    float* __restrict__ m, float* __restrict__ v, int C, long per_image,
    const float* __restrict__ steps, const float* __restrict__ rp, AdamScalars a,
    float* __restrict__ g_out, float* y_hat_out, float* __restrict__ y_deq,
    int* __restrict__ status, double* __restrict__ partial, int chunks) {
  extern __shared__ float sp[];   // [11][C]
  const Chunk k = sweep_chunk(chunks, per_image);
  const float d = steps[k.b];
  stage_step_pack(rp, C, d, sp);
  a.neg_step_size = a.neg_step_size * d;   // lr_b = lr · Δ_b
  float s = 0.f;
  int bad = 0;
  for (long j = k.lo + threadIdx.x; j < k.hi; j += kThreads) {
    const int c = (int)(j % C);
    const long i = (long)k.b * per_image + j;
    float yv = y[i];
    if constexpr (UPDATE) {
      const float dz = rate_dz_element(y_hat[i], sp, C, c, 1.0f);
      const float g = g_deq[i] + dz / d;
      if (g_out) g_out[i] = g;
      float mv = m[i], vv = v[i];
      yv = adam_element(yv, g, mv, vv, a);
      m[i] = mv;
      v[i] = vv;
      y[i] = yv;
    }
    const float q = rintf(yv / d);
    bad |= level_status(q);
    store_level(q, d, i, y_hat_out, y_deq);
    s += element_bits(q, sp, C, c);
  }
  report_status(bad, status + k.b);
  chunk_sum_store(s, k, chunks, partial);
}

// The distortion term of J and what is recorded of it, per objective:
//   (λ_b/3)·SSE_b/255²            the 8-bit squared error (int64), codec.refine_objective
//   (λ_b·area_b)·(1 − MS-SSIM_b)  the fp32 MS-SSIM of the 8-bit decode over area_b = H_b·W_b
//                                 pixels, codec.refine_objective_msssim
struct SseTerm {
  const long* __restrict__ sse;
  long* __restrict__ best;
  __device__ __forceinline__ double of(int b, double lam) const {
    return ((lam / 3.0) * (double)sse[b]) / 65025.0;
  }
  __device__ __forceinline__ void record(int b) const { best[b] = sse[b]; }
};

struct MsssimTerm {
  const float* __restrict__ ms;
  const double* __restrict__ area;
  float* __restrict__ best;
  __device__ __forceinline__ double of(int b, double lam) const {
    return (lam * area[b]) * (1.0 - (double)ms[b]);
  }
  __device__ __forceinline__ void record(int b) const { best[b] = ms[b]; }
};

// The decision, one body for both objectives. One workgroup, a thread per image: every block of
// the copy then reads one decision.
template <class Term>
__device__ __forceinline__ void refine_decide_body(const double* __restrict__ bits, const Term term,
                                                   const double* __restrict__ lam,
                                                   const int* __restrict__ qstatus,
                                                   const int* __restrict__ rstatus, int B, int iter,
                                                   double* __restrict__ best_J,
                                                   int* __restrict__ best_iter,
                                                   double* __restrict__ best_bits,
                                                   int* __restrict__ flag) {
  const bool recon_bad = rstatus != nullptr && *rstatus != 0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const double J = bits[b] + term.of(b, lam[b]);
    const bool better = !recon_bad && qstatus[b] == 0 && J < best_J[b];   // NaN: not better
    flag[b] = better ? 1 : 0;
    if (better) {
      best_J[b] = J;
      best_iter[b] = iter;
      best_bits[b] = bits[b];
      term.record(b);
    }
  }
}

__global__ void refine_decide_kernel(const double* __restrict__ bits, const long* __restrict__ sse,
                                     const double* __restrict__ lam,
                                     const int* __restrict__ qstatus,
                                     const int* __restrict__ rstatus, int B, int iter,
                                     double* __restrict__ best_J, int* __restrict__ best_iter,
                                     double* __restrict__ best_bits, long* __restrict__ best_sse,
                                     int* __restrict__ flag) {
  refine_decide_body(bits, SseTerm{sse, best_sse}, lam, qstatus, rstatus, B, iter, best_J,
                     best_iter, best_bits, flag);
}

__global__ void refine_decide_msssim_kernel(
    const double* __restrict__ bits, const float* __restrict__ ms, const double* __restrict__ lam,
    const double* __restrict__ area, const int* __restrict__ qstatus,
    const int* __restrict__ rstatus, int B, int iter, double* __restrict__ best_J,
    int* __restrict__ best_iter, double* __restrict__ best_bits, float* __restrict__ best_ms,
    int* __restrict__ flag) {
  refine_decide_body(bits, MsssimTerm{ms, area, best_ms}, lam, qstatus, rstatus, B, iter, best_J,
                     best_iter, best_bits, flag);
}

// grid (blocks per image, B)
__global__ void __launch_bounds__(kThreads) refine_copy_kernel(const float* __restrict__ y_hat,
                                                               long per_image,
                                                               const int* __restrict__ flag,
                                                               float* __restrict__ best) {
  if (!flag[blockIdx.y]) return;
  const long base = (long)blockIdx.y * per_image;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < per_image;
       i += (long)gridDim.x * kThreads)
    best[base + i] = y_hat[base + i];
}

int copy_kept(const char* what, const float* y_hat, int B, int64_t per_image, const int32_t* flag,
              float* best, hipStream_t st) {
  const long blocks = ((long)per_image + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(refine_copy_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks), (unsigned)B),
                     dim3(kThreads), 0, st, y_hat, (long)per_image, (const int*)flag, best);
  return check_launch(what);
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_refine_grad_recon(const float* recon, const uint8_t* ref, const int64_t* desc,
                             const float* wt, int B, int Hc, int Wc, float* g, void* stream) {
  ICLR17_REQUIRE(recon && ref && desc && wt && g, ICLR17_EINVAL, "refine_grad_recon: null pointer");
  ICLR17_REQUIRE(B > 0 && Hc > 0 && Wc > 0 && (long)Hc * Wc < (1L << 31), ICLR17_EINVAL,
                 "refine_grad_recon: bad shape B=%d Hc=%d Wc=%d", B, Hc, Wc);
  const long n = (long)B * Hc * Wc;
  hipLaunchKernelGGL(refine_grad_recon_kernel, dim3(elementwise_blocks(n)), dim3(256), 0,
                     (hipStream_t)stream, recon, (const unsigned char*)ref, (const long*)desc, wt,
                     Hc, Wc, n, g);
  return check_launch("refine_grad_recon");
}

int iclr17_refine_step(const float* y_hat, const float* g_deq, float* y, float* m, float* v, int B,
                       int h, int w, int N, const float* steps_dev, const float* rate_packed,
                       double lr, long step, float* g_out, float* y_hat_out, float* y_deq,
                       int32_t* status, double* bits_partial, void* stream) {
  ICLR17_REQUIRE(y && steps_dev && rate_packed && y_hat_out && y_deq && status && bits_partial,
                 ICLR17_EINVAL, "refine_step: null pointer");
  ICLR17_REQUIRE(!g_deq || (y_hat && m && v), ICLR17_EINVAL,
                 "refine_step: a gradient needs y_hat, m and v");
  ICLR17_REQUIRE(!g_deq || (step >= 1 && isfinite(lr) && lr > 0.0), ICLR17_EINVAL,
                 "refine_step: bad step count %ld or learning rate %g", step, lr);
  size_t shm;
  int rc = check_step_shape("refine_step", B, h, w, N, &shm);
  if (rc) return rc;
  const int chunks = iclr17_rate_bits_partials(N, h, w);   // rate_bits' own chunks
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks < (1L << 31), ICLR17_EUNSUPPORTED, "refine_step: %ld workgroups", blocks);
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(status, 0, (size_t)B * sizeof(int32_t), st);
  if (e != hipSuccess) {
    set_error(ICLR17_ELAUNCH, "refine_step: %s", hipGetErrorString(e));
    return ICLR17_ELAUNCH;
  }
  const long per_image = (long)N * h * w;
  if (g_deq) {
    // torch.optim.Adam's defaults and scalars (optim.hip), the step size per unit Δ
    const double beta1 = 0.9, beta2 = 0.999, eps = 1e-8;
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    const AdamScalars a{(float)(-(lr / bc1)), (float)pow(bc2, 0.5), (float)(1.0 - beta1),
                        (float)beta2, (float)(1.0 - beta2), (float)eps};
    hipLaunchKernelGGL(refine_step_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), shm, st,
                       y_hat, g_deq, y, m, v, N, per_image, steps_dev, rate_packed, a, g_out,
                       y_hat_out, y_deq, (int*)status, bits_partial, chunks);
  } else {
    hipLaunchKernelGGL(refine_step_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), shm, st,
                       (const float*)nullptr, (const float*)nullptr, y, (float*)nullptr,
                       (float*)nullptr, N, per_image, steps_dev, rate_packed, AdamScalars{},
                       (float*)nullptr, y_hat_out, y_deq, (int*)status, bits_partial, chunks);
  }
  return check_launch("refine_step");
}

int iclr17_refine_keep(const double* bits, const int64_t* sse, const double* lam,
                       const int32_t* qstatus, const int32_t* recon_status, const float* y_hat,
                       int B, int64_t per_image, int iter, double* best_J, int32_t* best_iter,
                       double* best_bits, int64_t* best_sse, float* best, int32_t* flag,
                       void* stream) {
  ICLR17_REQUIRE(bits && sse && lam && qstatus && y_hat && best_J && best_iter && best_bits &&
                     best_sse && best && flag,
                 ICLR17_EINVAL, "refine_keep: null pointer");
  ICLR17_REQUIRE(B > 0 && B <= 65535 && per_image > 0 && iter >= 0, ICLR17_EINVAL,
                 "refine_keep: bad shape B=%d per_image=%lld iter=%d", B, (long long)per_image,
                 iter);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(refine_decide_kernel, dim3(1), dim3(256), 0, st, bits, (const long*)sse, lam,
                     (const int*)qstatus, (const int*)recon_status, B, iter, best_J,
                     (int*)best_iter, best_bits, (long*)best_sse, (int*)flag);
  int rc = check_launch("refine_keep (decide)");
  if (rc) return rc;
  return copy_kept("refine_keep", y_hat, B, per_image, flag, best, st);
}

int iclr17_refine_keep_msssim(const double* bits, const float* ms, const double* lam,
                              const double* area, const int32_t* qstatus,
                              const int32_t* recon_status, const float* y_hat, int B,
                              int64_t per_image, int iter, double* best_J, int32_t* best_iter,
                              double* best_bits, float* best_ms, float* best, int32_t* flag,
                              void* stream) {
  ICLR17_REQUIRE(bits && ms && lam && area && qstatus && y_hat && best_J && best_iter &&
                     best_bits && best_ms && best && flag,
                 ICLR17_EINVAL, "refine_keep_msssim: null pointer");
  ICLR17_REQUIRE(B > 0 && B <= 65535 && per_image > 0 && iter >= 0, ICLR17_EINVAL,
                 "refine_keep_msssim: bad shape B=%d per_image=%lld iter=%d", B,
                 (long long)per_image, iter);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(refine_decide_msssim_kernel, dim3(1), dim3(256), 0, st, bits, ms, lam, area,
                     (const int*)qstatus, (const int*)recon_status, B, iter, best_J,
                     (int*)best_iter, best_bits, best_ms, (int*)flag);
  int rc = check_launch("refine_keep_msssim (decide)");
  if (rc) return rc;
  return copy_kept("refine_keep_msssim", y_hat, B, per_image, flag, best, st);
}

}  // extern "C"
