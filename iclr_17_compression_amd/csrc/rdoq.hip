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
// The sums have rate_bits' structure (aux.hip): 4096-element chunks of the NHWC latent, the same
// thread → element map, fp32 per thread and wave, float64 across the waves, and
// iclr17_reduce_partials over the chunks. No atomics in a sum: bitwise reproducible, and an
// image's result does not depend on its batch.
#include <math.h>

#include "common.h"

namespace iclr17 {
namespace {

constexpr int kRdoMax = 32;        // steps per launch (ratectl.hip's kSweepMax)
constexpr int kRdoChunk = 4096;    // latents per partial: aux.hip's kRateChunk
constexpr int kRdoThreads = 256;
constexpr size_t kLdsLimit = 64 * 1024;

struct Steps {
  float d[kRdoMax];
};

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

enum : int { ST_NAN = 1, ST_RANGE = 2 };

// One workgroup per (image, 4096-element chunk). LDS: the 11·C rate floats, lam[C] and the bits of
// level 0 per channel. partial[b][chunk].
__global__ void __launch_bounds__(kRdoThreads) quantise_rdo_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ rp, float d,
    const float* __restrict__ lam, float* __restrict__ y_hat, float* __restrict__ y_deq,
    double* __restrict__ partial, int chunks, int* __restrict__ status) {
  extern __shared__ float lds[];
  __shared__ float red[4];
  float* sp = lds;                       // [11][C]
  float* lw = lds + kRateRows * C;       // [C]
  float* zb = lw + C;                    // [C]
  const int tid = threadIdx.x;
  for (int i = tid; i < kRateRows * C; i += kRdoThreads) sp[i] = rp[i];
  for (int i = tid; i < C; i += kRdoThreads) lw[i] = lam[i];
  __syncthreads();
  for (int c = tid; c < C; c += kRdoThreads) {
    float p[kRateRows];
#pragma unroll
    for (int k = 0; k < kRateRows; ++k) p[k] = sp[k * C + c];
    zb[c] = bits_regs(0.f, p[0] * d, p);
  }
  __syncthreads();
  const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const long lo = (long)ch * kRdoChunk;
  const long hi = lo + kRdoChunk < per_image ? lo + kRdoChunk : per_image;
  float s = 0.f;
  int bad = 0;
#pragma unroll 1
  for (long j = lo + tid; j < hi; j += kRdoThreads) {
    const int c = (int)(j % C);
    const long i = (long)b * per_image + j;
    const float t = y[i] / d;
    const float r = rintf(t);
    float q = r, bits = zb[c];
    if (!(r == r)) {
      bad |= ST_NAN;
    } else if (fabsf(r) > 32767.f) {
      bad |= ST_RANGE;
    } else if (r != 0.f) {
      float p[kRateRows];
#pragma unroll
      for (int k = 0; k < kRateRows; ++k) p[k] = sp[k * C + c];
      q = rdo_pick(t, r, p[0] * d, p, lw[c] * d * d, zb[c], &bits);
    }
    y_hat[i] = q;
    y_deq[i] = d * q;
    s += bits;
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
  if ((tid & 63) == 0 && bad) atomicOr(status, bad);
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < 4; ++w) t += (double)red[w];
    partial[(long)b * chunks + ch] = t;
  }
}

// One workgroup per (image, chunk), as rate_sweep_kernel. LDS: the rate floats, lam, the bits of
// level 0 per (step, channel) and the chunk of y, read from memory once. The step loop is the
// outer one and stays rolled (32 inlined copies of the model would not fit the instruction
// cache); a thread adds its elements' bits of one step in a register, in rate_bits' order, so no
// accumulator per (step, thread) is needed and the level-0 table fits beside the chunk.
// partial[b][s][chunk].
__global__ void __launch_bounds__(kRdoThreads) rate_sweep_rdo_kernel(
    const float* __restrict__ y, int C, long per_image, const float* __restrict__ rp, Steps st,
    int S, const float* __restrict__ lam, double* __restrict__ partial, int chunks) {
  extern __shared__ float lds[];
  __shared__ float red[4][kRdoMax];
  __shared__ float ds[kRdoMax];
  float* sp = lds;                       // [11][C]
  float* lw = lds + kRateRows * C;       // [C]
  float* zb = lw + C;                    // [S][C]
  float* yv = zb + S * C;                // [4096]
  const int tid = threadIdx.x;
  const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const long lo = (long)ch * kRdoChunk;
  const long hi = lo + kRdoChunk < per_image ? lo + kRdoChunk : per_image;
  const int n = (int)(hi - lo);
  for (int i = tid; i < kRateRows * C; i += kRdoThreads) sp[i] = rp[i];
  for (int i = tid; i < C; i += kRdoThreads) lw[i] = lam[i];
  for (int i = tid; i < n; i += kRdoThreads) yv[i] = y[(long)b * per_image + lo + i];
  if (tid == 0) {
#pragma unroll
    for (int s = 0; s < kRdoMax; ++s) ds[s] = st.d[s];   // constant indices: scalar loads
  }
  __syncthreads();
#pragma unroll 1
  for (int i = tid; i < S * C; i += kRdoThreads) {
    const int s = i / C, c = i - s * C;
    float p[kRateRows];
#pragma unroll
    for (int k = 0; k < kRateRows; ++k) p[k] = sp[k * C + c];
    zb[i] = bits_regs(0.f, p[0] * ds[s], p);
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const int c0 = (int)((lo + tid) % C);
#pragma unroll 1
  for (int s = 0; s < S; ++s) {
    const float d = ds[s];
    float acc = 0.f;
    int c = c0;
#pragma unroll 1
    for (int j = tid; j < n; j += kRdoThreads) {
      const float t = yv[j] / d;
      const float r = rintf(t);
      float bits = zb[s * C + c];
      if (r != 0.f) {
        float p[kRateRows];
#pragma unroll
        for (int k = 0; k < kRateRows; ++k) p[k] = sp[k * C + c];
        if (r == r && fabsf(r) <= 32767.f)
          rdo_pick(t, r, p[0] * d, p, lw[c] * d * d, zb[s * C + c], &bits);
        else
          bits = bits_regs(r, p[0] * d, p);   // what quantise_rdo refuses: rate_sweep's figure
      }
      acc += bits;
      c = (c + kRdoThreads) % C;
    }
    const float t = wave_sum(acc);
    if (lane == 0) red[wave][s] = t;
  }
  __syncthreads();
  if (tid < S) {
    double t = 0.0;
    for (int w = 0; w < 4; ++w) t += (double)red[w][tid];
    partial[((long)b * S + tid) * chunks + ch] = t;
  }
}

bool good_step(float d) { return isfinite(d) && d > 0.f; }

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
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "quantise_rdo: bad shape B=%d h=%d w=%d N=%d", B, h, w, N);
  ICLR17_REQUIRE(good_step(step), ICLR17_EINVAL,
                 "quantise_rdo: the step %g is not finite and positive", (double)step);
  const size_t shm = ((size_t)kRateRows + 2) * N * sizeof(float);
  ICLR17_REQUIRE(shm <= kLdsLimit - sizeof(float) * 4, ICLR17_EUNSUPPORTED,
                 "quantise_rdo: N=%d needs %zu bytes of LDS", N, shm);
  const int chunks = iclr17_rate_sweep_rdo_partials(h, w, N);
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks < (1L << 31), ICLR17_EUNSUPPORTED, "quantise_rdo: %ld workgroups", blocks);
  hipLaunchKernelGGL(quantise_rdo_kernel, dim3((unsigned)blocks), dim3(kRdoThreads), shm,
                     (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, step, lam, y_hat,
                     y_deq, partial, chunks, (int*)status);
  const int rc = check_launch("quantise_rdo");
  if (rc) return rc;
  // bits[b] = Σ_chunk partial[b][chunk], in reduce_partials' fixed order
  return iclr17_reduce_partials(partial, B, chunks, bits, nullptr, 1.0, stream);
}

int iclr17_rate_sweep_rdo(const float* y, int B, int h, int w, int N, const float* rate_packed,
                          const float* steps, int S, const float* lam, double* partial,
                          double* bits, void* stream) {
  ICLR17_REQUIRE(y && rate_packed && steps && lam && partial && bits, ICLR17_EINVAL,
                 "rate_sweep_rdo: null pointer");
  ICLR17_REQUIRE(B > 0 && h > 0 && w > 0 && N > 0, ICLR17_EINVAL,
                 "rate_sweep_rdo: bad shape B=%d h=%d w=%d N=%d", B, h, w, N);
  ICLR17_REQUIRE(S >= 1 && S <= kRdoMax, ICLR17_EINVAL, "rate_sweep_rdo: S=%d steps (1..%d)", S,
                 kRdoMax);
  Steps st;
  for (int s = 0; s < kRdoMax; ++s) st.d[s] = 1.0f;
  for (int s = 0; s < S; ++s) {
    ICLR17_REQUIRE(good_step(steps[s]), ICLR17_EINVAL,
                   "rate_sweep_rdo: step %d (%g) is not finite and positive", s, (double)steps[s]);
    st.d[s] = steps[s];
  }
  const size_t shm =
      (((size_t)kRateRows + 1 + S) * N + (size_t)kRdoChunk) * sizeof(float);
  ICLR17_REQUIRE(shm <= kLdsLimit - sizeof(float) * 5 * kRdoMax, ICLR17_EUNSUPPORTED,
                 "rate_sweep_rdo: N=%d and S=%d need %zu bytes of LDS", N, S, shm);
  const int chunks = iclr17_rate_sweep_rdo_partials(h, w, N);
  const long blocks = (long)B * chunks;
  ICLR17_REQUIRE(blocks * S < (1L << 31), ICLR17_EUNSUPPORTED,
                 "rate_sweep_rdo: %ld workgroups x %d steps", blocks, S);
  hipLaunchKernelGGL(rate_sweep_rdo_kernel, dim3((unsigned)blocks), dim3(kRdoThreads), shm,
                     (hipStream_t)stream, y, N, (long)N * h * w, rate_packed, st, S, lam, partial,
                     chunks);
  const int rc = check_launch("rate_sweep_rdo");
  if (rc) return rc;
  return iclr17_reduce_partials(partial, B * S, chunks, bits, nullptr, 1.0, stream);
}

}  // extern "C"
