// Rate–distortion optimised quantisation: an encoder-side choice of the level.
//
// At a step Δ the plain quantiser sends r = rintf(y/Δ), the level of least latent distortion
// whatever it costs. Here each element picks, among r, the level one nearer to zero and zero
// itself, the one of least  J(v) = bits(v) + w_c·(v − y/Δ)²,  w_c = lam[c]·Δ·Δ, with bits the
// factorised model's own (common.h bits_regs on the step pack of Δ). The model is factorised, so
// the choice is independent per element; the decoder does not care which integer was sent.
//
//   quantise_rdo     ŷ, Δ·ŷ and the per-image Σ bits(ŷ) from one read of y
//   rate_sweep_rdo   Σ bits(ŷ) of every image at up to 32 steps from one read of y
//
// Both are bound by transcendentals (a CDF is 3 tanhf and 1 expf), so the candidates share what
// they can. Neighbouring levels share a bin edge: for |r| ≤ 32767, r − ½ and (r − 1) + ½ are the
// same fp32 value, so r and its neighbour take 3 CDFs, not 4. The bits of level 0 depend on
// (channel, step) alone and are computed once per workgroup into LDS: an element with r = 0 (most
// of a latent) then costs no CDF at all, one with |r| = 1 two and every other three. Every bit
// total is what bits_regs gives for the picked level, term for term.
//
// Both stand in ladder.h's frame: its chunks and tails for the sums, and for quantise_rdo its
// flagging and storing functions around the pick.
#include <math.h>

#include "ladder.h"

namespace iclr17 {
namespace {

constexpr size_t kLdsLimit = 64 * 1024;

// bits_regs' last lines on two CDF values
__device__ __forceinline__ float bits_of(float hi, float lo) {
  const float prob = hi - lo;
  float bits = (-1.0f * logf(prob + 1e-10f)) / 0.693147182464599609375f;
  bits = fminf(fmaxf(bits, 0.0f), 50.0f);
  return bits;
}

// The pick for one element with r = rintf(t) ≠ 0: candidates r, r − sign(r) and (|r| ≥ 2) zero in
// that order, the first of least J; a strict < moves the pick on, so on equal cost (and on a NaN
// cost) the candidate of less distortion stays. zero_bits: bits_regs(0) of this channel and step.
// Returns the level; its bits in *bits.
__device__ __forceinline__ float rdo_pick(float t, float r, float sp0, const float (&p)[kRateRows],
                                          float w, float zero_bits, float* bits) {
  const float Fa = cdf_regs(r + 0.5f, sp0, p);
  const float Fb = cdf_regs(r - 0.5f, sp0, p);
  float e = r - t;
  float best = r, best_bits = bits_of(Fa, Fb);
  float best_j = best_bits + w * (e * e);
  const bool pos = r > 0.f;
  const float v1 = pos ? r - 1.f : r + 1.f;
  const bool far = fabsf(r) >= 2.f;
  float b1 = zero_bits;
  if (far) {
    // the neighbour's outer edge; its inner edge is r ∓ ½, already evaluated
    const float Fc = cdf_regs(pos ? v1 - 0.5f : v1 + 0.5f, sp0, p);
    b1 = pos ? bits_of(Fb, Fc) : bits_of(Fc, Fa);
  }
  e = v1 - t;
  const float j1 = b1 + w * (e * e);
  if (j1 < best_j) {
    best = v1;
    best_bits = b1;
    best_j = j1;
  }
  if (far) {
    e = 0.f - t;
    const float j2 = zero_bits + w * (e * e);
    if (j2 < best_j) {
      best = 0.f;
      best_bits = zero_bits;
    }
  }
  *bits = best_bits;
  return best;
}

// One workgroup per (image, 4096-element chunk). LDS: the 11·C rate floats, lam[C] and the bits of
// level 0 per channel. partial[b][chunk].
__global__ void __launch_bounds__(kThreads) quantise_rdo_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ rp, float d,
    const float* __restrict__ lam, float* __restrict__ y_hat, float* __restrict__ y_deq,
    double* __restrict__ partial, int chunks, int* __restrict__ status) {
  extern __shared__ float lds[];
  float* sp = lds;                       // [11][C]
  float* lw = lds + kRateRows * C;       // [C]
  float* zb = lw + C;                    // [C]
  const int tid = threadIdx.x;
  for (int i = tid; i < kRateRows * C; i += kThreads) sp[i] = rp[i];
  for (int i = tid; i < C; i += kThreads) lw[i] = lam[i];
  __syncthreads();
  for (int c = tid; c < C; c += kThreads) {
    float p[kRateRows];
#pragma unroll
    for (int m = 0; m < kRateRows; ++m) p[m] = sp[m * C + c];
    zb[c] = bits_regs(0.f, p[0] * d, p);
  }
  __syncthreads();
  const Chunk k = sweep_chunk(chunks, per_image);
  float s = 0.f;
  int bad = 0;
#pragma unroll 1
  for (long j = k.lo + tid; j < k.hi; j += kThreads) {
    const int c = (int)(j % C);
    const long i = (long)k.b * per_image + j;
    const float t = y[i] / d;
    const float r = rintf(t);
    float q = r, bits = zb[c];
    const int flags = level_status(r);
    bad |= flags;
    if (!flags && r != 0.f) {
      float p[kRateRows];
#pragma unroll
      for (int m = 0; m < kRateRows; ++m) p[m] = sp[m * C + c];
      q = rdo_pick(t, r, p[0] * d, p, lw[c] * d * d, zb[c], &bits);
    }
    store_level(q, d, i, y_hat, y_deq);
    s += bits;
  }
  report_status(bad, status);
  chunk_sum_store(s, k, chunks, partial);
}

// One workgroup per (image, chunk) in the sweeps' frame, with a body of its own, not
// rate_sweep_kernel's: the pick's level-0 table per (step, channel) has to fit the LDS. LDS: the
// rate floats, lam, that table and the chunk of y, read from memory once. The step loop is the
// outer one and stays rolled (32 inlined copies of the model would not fit the instruction
// cache); a thread adds its elements' bits of one step in a register, in rate_bits' order, so no
// accumulator per (step, thread) is needed and the level-0 table fits beside the chunk.
// partial[b][s][chunk].
__global__ void __launch_bounds__(kThreads) rate_sweep_rdo_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ rp, Steps st,
    int S, const float* __restrict__ lam, double* __restrict__ partial, int chunks) {
  extern __shared__ float lds[];
  __shared__ float red[4][kLadder];
  __shared__ float ds[kLadder];
  float* sp = lds;                       // [11][C]
  float* lw = lds + kRateRows * C;       // [C]
  float* zb = lw + C;                    // [S][C]
  float* yv = zb + S * C;                // [4096]
  const int tid = threadIdx.x;
  const Chunk k = sweep_chunk(chunks, per_image);
  const int n = (int)(k.hi - k.lo);
  for (int i = tid; i < kRateRows * C; i += kThreads) sp[i] = rp[i];
  for (int i = tid; i < C; i += kThreads) lw[i] = lam[i];
  for (int i = tid; i < n; i += kThreads) yv[i] = y[(long)k.b * per_image + k.lo + i];
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s < kLadder; ++s) ds[s] = st.d[s];   // constant indices: scalar loads
  }
  __syncthreads();
#pragma unroll 1
  for (int i = tid; i < S * C; i += kThreads) {
    const int s = i / C, c = i - s * C;
    float p[kRateRows];
#pragma unroll
    for (int m = 0; m < kRateRows; ++m) p[m] = sp[m * C + c];
    zb[i] = bits_regs(0.f, p[0] * ds[s], p);
  }
  __syncthreads();
  const int c0 = (int)((k.lo + tid) % C);
#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const float d = ds[s];
    float acc = 0.f;
    int c = c0;
#pragma unroll 1
    for (int j = tid; j < n; j += kThreads) {
      const float t = yv[j] / d;
      const float r = rintf(t);
      float bits = zb[s * C + c];
      if (r != 0.f) {
        float p[kRateRows];
#pragma unroll
        for (int m = 0; m < kRateRows; ++m) p[m] = sp[m * C + c];
        if (r == r && fabsf(r) <= 32767.f)
          rdo_pick(t, r, p[0] * d, p, lw[c] * d * d, zb[s * C + c], &bits);
        else
          bits = bits_regs(r, p[0] * d, p);   // what quantise_rdo refuses: rate_sweep's figure
      }
      acc += bits;
      c = (c + kThreads) % C;
    }
    sweep_wave(red, k, s, acc);
  }
  sweep_store(red, S, k, chunks, partial);
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_rate_sweep_rdo_partials(int h, int w, int N) {
  return iclr17_rate_sweep_partials(h, w, N);
}

int iclr17_quantise_rdo(const float* y, int B, int h, int w, int N, const float* rate_packed,
                        float step, const float* lam, float* y_hat, float* y_deq, double* partial,
                        double* bits, int32_t* status, void* stream) {
  ICLR17_REQUIRE(y && rate_packed && lam && y_hat && y_deq && partial && bits && status,
                 ICLR17_EINVAL, "quantise_rdo: null pointer");
  int rc = check_latent("quantise_rdo", B, h, w, N);
  if (rc) return rc;
  ICLR17_REQUIRE(good_step(step), ICLR17_EINVAL,
                 "quantise_rdo: the step %g is not finite and positive", (double)step);
  const size_t shm = ((size_t)kRateRows + 2) * N * sizeof(float);
  ICLR17_REQUIRE(shm <= kLdsLimit - sizeof(float) * 4, ICLR17_EUNSUPPORTED,
                 "quantise_rdo: N=%d needs %zu bytes of LDS", N, shm);
  const int chunks = iclr17_rate_sweep_rdo_partials(h, w, N);
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks < (1L << 31), ICLR17_EUNSUPPORTED, "quantise_rdo: %ld workgroups", blocks);
  hipLaunchKernelGGL(quantise_rdo_kernel, dim3((unsigned)blocks), dim3(kThreads), shm,
                     (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, step, lam, y_hat,
                     y_deq, partial, chunks, (int*)status);
  rc = check_launch("quantise_rdo");
  if (rc) return rc;
  // bits[b] = Σ_chunk partial[b][chunk], in reduce_partials' fixed order
  return iclr17_reduce_partials(partial, B, chunks, bits, nullptr, 1.0, stream);
}

int iclr17_rate_sweep_rdo(const float* y, int B, int h, int w, int N, const float* rate_packed,
                          const float* steps, int S, const float* lam, double* partial,
                          double* bits, void* stream) {
  ICLR17_REQUIRE(y && rate_packed && steps && lam && partial && bits, ICLR17_EINVAL,
                 "rate_sweep_rdo: null pointer");
  const SweepCall c{"rate_sweep_rdo", B, h, w, N, nullptr, steps, S, partial, bits, stream};
  return run_sweep(c, [&](const Steps& st, int chunks, unsigned blocks) -> int {
    const size_t shm = (((size_t)kRateRows + 1 + S) * N + (size_t)kChunk) * sizeof(float);
    ICLR17_REQUIRE(shm <= kLdsLimit - sizeof(float) * 5 * kLadder, ICLR17_EUNSUPPORTED,
                   "rate_sweep_rdo: N=%d and S=%d need %zu bytes of LDS", N, S, shm);
    hipLaunchKernelGGL(rate_sweep_rdo_kernel, dim3(blocks), dim3(kThreads), shm,
                       (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, st, S, lam,
                       partial, chunks);
    return 0;
  });
}

}  // extern "C"
