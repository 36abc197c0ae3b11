// Centroid reconstruction: the decoder places a level at the mean of its bin under
// the rate model it already holds, not at the bin's centre. Decoder-only: no bit of a stream
// changes, and nothing here has to match the fp32 rate path.
//
//   recon_offsets          off[s][c][v + K] = strength · (the bin mean of level v of channel c at
//                          step s, minus v, in level units), one thread per entry (the zero bin
//                          only: per step and channel, on a zeroed table), float64
//   dequantise_recon       Δ·(ŷ + off[c][ŷ + K]) at one step; the [N][2K+1] table in LDS where it
//                          fits, else read from global memory
//   dequantise_recon_map   the same with a step and a table per block (slots, as the mapped
//                          coder's); the stacked tables are read from global memory
//
// With F the model's CDF and Δ the step, level v's bin is [Δ(v − ½), Δ(v + ½)], a = F(Δ(v − ½)),
// b = F(Δ(v + ½)), p = b − a. Integration by parts gives the bin mean in level units as
//   v + (½(a + b) − I)/p,   I = ∫_{−½}^{½} F(Δ(v + u)) du,
// which carries no factor |v|: no cancellation in the tails. I is composite Simpson with
// kReconSimpson sub-intervals, summed in the order k = 0..n. Entries with p < 2⁻²⁴ (the fp32
// epsilon of the CDF the coder's tables are built from) are 0; the offset is clamped to ±½.
#include "ladder.h"

using namespace iclr17;

namespace iclr17 {
namespace {

constexpr int kReconSimpson = 512;       // sub-intervals of a bin (how it was chosen)
constexpr double kReconMinP = 0x1p-24;
constexpr unsigned kReconBlocks = 512;   // dequantise_recon's grid limit: a table is staged per block

__global__ void __launch_bounds__(kThreads) recon_offsets_kernel(const float* __restrict__ rp,
                                                                 int N, int K, Steps st, int S,
                                                                 int mode, float strength,
                                                                 float* __restrict__ off) {
  __shared__ float sd[kLadder];
  stage_ladder(st, sd);
  const int L = 2 * K + 1;
  // every entry, or (the zero bin only) a thread per (step, channel) on a table zeroed before:
  // a wave then holds 64 bins to integrate, not one among 64 idle lanes
  const long j = (long)blockIdx.x * kThreads + threadIdx.x;
  const long i = mode == ICLR17_RECON_ZERO ? j * L + K : j;
  if (i >= (long)S * N * L) return;
  const int v = (int)(i % L) - K;
  const int c = (int)((i / L) % N);
  const int s = (int)(i / ((long)L * N));
  float o = 0.f;
  const double d = (double)sd[s];
  const double a = bitparm_cdf64(d * ((double)v - 0.5), rp, N, c);
  const double b = bitparm_cdf64(d * ((double)v + 0.5), rp, N, c);
  const double p = b - a;
  if (p >= kReconMinP) {
    constexpr int n = kReconSimpson;
    double acc = a;
    for (int k = 1; k < n; ++k) {
      const double u = (double)(k - n / 2) / (double)n;
      acc += ((k & 1) ? 4.0 : 2.0) * bitparm_cdf64(d * ((double)v + u), rp, N, c);
    }
    acc += b;
    double f = (0.5 * (a + b) - acc / (3.0 * n)) / p;
    f = f < -0.5 ? -0.5 : f > 0.5 ? 0.5 : f;
    o = (float)((double)strength * f);
  }
  off[i] = o;
}

// Where an element's step and table row come from. stage() runs once before the loop; slot(i) is
// element i's table set, step(sd, slot) its Δ and row(slot, c) the 2K+1 offsets of channel c.
struct OneTable {   // one step, one table: staged in the dynamic LDS when lds, else global
  float d;
  const float* __restrict__ off;
  int tab;     // N·(2K+1)
  bool lds;
  __device__ __forceinline__ void stage(float*, float* st) const {
    if (lds) {
      for (int i = threadIdx.x; i < tab; i += kThreads) st[i] = off[i];
      __syncthreads();
    }
  }
  __device__ __forceinline__ int slot(long) const { return 0; }
  __device__ __forceinline__ float step(const float*, int) const { return d; }
  __device__ __forceinline__ const float* row(const float* st, int, int c, int L) const {
    return (lds ? st : off) + (long)c * L;
  }
};

struct MapTables {   // a step and a table per block: steps[slot], off[slot][c]
  int C, S;
  MapGeo g;
  const unsigned char* __restrict__ slots;
  const float* __restrict__ off;
  Steps st;
  __device__ __forceinline__ void stage(float* sd, float*) const { stage_ladder(st, sd); }
  __device__ __forceinline__ int slot(long i) const {
    const int t = slots[map_entry(g, i / C)];
    return t < S ? t : S - 1;   // the caller checked the map; never read past the tables
  }
  __device__ __forceinline__ float step(const float* sd, int t) const { return sd[t]; }
  __device__ __forceinline__ const float* row(const float*, int t, int c, int L) const {
    return off + ((long)t * C + c) * L;
  }
};

// Δ ⊗ (ŷ ⊕ off): an index into a row is formed only for |ŷ| ≤ K; escapes, infinities and NaN
// take the offset 0
__device__ __forceinline__ float recon_element(float q, float d, const float* __restrict__ row,
                                               int K) {
  float o = 0.f;
  if (fabsf(q) <= (float)K) o = row[(int)q + K];
  return d * (q + o);
}

template <class Src>
__global__ void __launch_bounds__(kThreads) dequantise_recon_kernel(const float* __restrict__ y_hat,
                                                                    long n, int N, int K, Src src,
                                                                    float* __restrict__ y_deq) {
  __shared__ float sd[kLadder];
  extern __shared__ float stab[];
  src.stage(sd, stab);
  const int L = 2 * K + 1;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
    const int t = src.slot(i);
    const int c = (int)(i % N);
    y_deq[i] = recon_element(y_hat[i], src.step(sd, t), src.row(stab, t, c, L), K);
  }
}

int check_levels(const char* what, int K) {
  ICLR17_REQUIRE(K >= 1 && K <= 1024, ICLR17_EINVAL, "%s: K=%d (1..1024)", what, K);
  return 0;
}

}  // namespace
}  // namespace iclr17

extern "C" {

int iclr17_recon_offsets(const float* rate_packed, int N, int K, const float* steps, int S,
                         int mode, float strength, float* off, void* stream) {
  ICLR17_REQUIRE(rate_packed && steps && off, ICLR17_EINVAL, "recon_offsets: null pointer");
  ICLR17_REQUIRE(N > 0, ICLR17_EINVAL, "recon_offsets: bad shape N=%d", N);
  int rc = check_levels("recon_offsets", K);
  if (!rc) rc = check_count("recon_offsets", S);
  if (rc) return rc;
  ICLR17_REQUIRE(mode == ICLR17_RECON_CENTROID || mode == ICLR17_RECON_ZERO, ICLR17_EINVAL,
                 "recon_offsets: mode %d (0: every level, 1: the zero bin only)", mode);
  ICLR17_REQUIRE(isfinite(strength) && strength >= 0.f && strength <= 1.f, ICLR17_EINVAL,
                 "recon_offsets: strength %g is not in [0, 1]", (double)strength);
  Steps st;
  rc = fill_steps("recon_offsets", steps, S, st);
  if (rc) return rc;
  const long total = (long)S * N * (2 * K + 1);
  ICLR17_REQUIRE(total < (1L << 31), ICLR17_EUNSUPPORTED, "recon_offsets: %ld entries", total);
  long threads = total;
  if (mode == ICLR17_RECON_ZERO) {
    threads = (long)S * N;
    const hipError_t e = hipMemsetAsync(off, 0, (size_t)total * sizeof(float), (hipStream_t)stream);
    ICLR17_REQUIRE(e == hipSuccess, ICLR17_ELAUNCH, "recon_offsets: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(recon_offsets_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, (hipStream_t)stream, rate_packed, N, K, st, S, mode,
                     strength, off);
  return check_launch("recon_offsets");
}

int iclr17_dequantise_recon(const float* y_hat, int B, int h, int w, int N, float step,
                            const float* off, int K, float* y_deq, void* stream) {
  ICLR17_REQUIRE(y_hat && off && y_deq, ICLR17_EINVAL, "dequantise_recon: null pointer");
  int rc = check_latent("dequantise_recon", B, h, w, N);
  if (!rc) rc = check_levels("dequantise_recon", K);
  if (rc) return rc;
  ICLR17_REQUIRE(good_step(step), ICLR17_EINVAL,
                 "dequantise_recon: the step %g is not finite and positive", (double)step);
  const long tab = (long)N * (2 * K + 1);
  ICLR17_REQUIRE(tab < (1L << 31), ICLR17_EUNSUPPORTED, "dequantise_recon: %ld entries", tab);
  const bool lds = tab * sizeof(float) <= kStepLdsMax - 256;
  const long n = (long)B * h * w * N;
  unsigned blocks = elementwise_blocks(n);
  if (lds && blocks > kReconBlocks) blocks = kReconBlocks;
  hipLaunchKernelGGL(dequantise_recon_kernel<OneTable>, dim3(blocks), dim3(kThreads),
                     lds ? (size_t)tab * sizeof(float) : 0, (hipStream_t)stream, y_hat, n, N, K,
                     OneTable{step, off, (int)tab, lds}, y_deq);
  return check_launch("dequantise_recon");
}

int iclr17_dequantise_recon_map(const float* y_hat, int B, int h, int w, int N,
                                const uint8_t* slots, int log2_g, const float* steps,
                                const float* off, int S, int K, float* y_deq, void* stream) {
  ICLR17_REQUIRE(y_hat && slots && steps && off && y_deq, ICLR17_EINVAL,
                 "dequantise_recon_map: null pointer");
  int rc = check_latent("dequantise_recon_map", B, h, w, N);
  if (!rc) rc = check_block("dequantise_recon_map", log2_g);
  if (!rc) rc = check_levels("dequantise_recon_map", K);
  if (!rc) rc = check_count("dequantise_recon_map", S);
  if (rc) return rc;
  MapTables src;
  rc = fill_steps("dequantise_recon_map", steps, S, src.st);
  if (rc) return rc;
  ICLR17_REQUIRE((long)S * N * (2 * K + 1) < (1L << 31), ICLR17_EUNSUPPORTED,
                 "dequantise_recon_map: %ld entries", (long)S * N * (2 * K + 1));
  src.C = N;
  src.S = S;
  src.g = geo_of(h, w, log2_g);
  src.slots = slots;
  src.off = off;
  const long n = (long)B * h * w * N;
  hipLaunchKernelGGL(dequantise_recon_kernel<MapTables>, dim3(elementwise_blocks(n)),
                     dim3(kThreads), 0, (hipStream_t)stream, y_hat, n, N, K, src, y_deq);
  return check_launch("dequantise_recon_map");
}

}  // extern "C"
