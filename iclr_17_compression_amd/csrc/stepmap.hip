// A quantiser step per block of latent positions: region-of-interest coding.
//
// The latent of a canvas is h×w positions; a block is g×g of them (g = 2^lg, lg = 0..4) and the
// map is mh×mw = ⌈h/g⌉×⌈w/g⌉ per image, row-major, the last row and column ragged. Position (i, j)
// belongs to block (i >> lg, j >> lg); every channel of a position shares its block's step.
//
//   quantise_step_map    ŷ = rintf(y/Δ_e) and Δ_e·ŷ in one pass, e the block's ladder index (u8
//                        map): ladder.h's quantiser with MapSteps as its step source, so
//                        quantise_step with the step looked up per element
//   dequantise_step_map  Δ_e·ŷ alone (the decoder's half)
//
// The rate sweep with an offset per block, rate_sweep_offsets, is rate_sweep's kernel and lives
// beside it in ratectl.hip.
#include "ladder.h"

using namespace iclr17;

namespace {

// the shape, block-edge and ladder checks of both entry points, and their step source
int map_steps(const char* what, int B, int h, int w, int N, const uint8_t* indices, int log2_g,
              const float* steps, MapSteps& src) {
  int rc = check_latent(what, B, h, w, N);
  if (!rc) rc = check_block(what, log2_g);
  if (!rc) rc = fill_steps(what, steps, kLadder, src.st);
  if (rc) return rc;
  src.g = geo_of(h, w, log2_g);
  src.idx = indices;
  src.C = N;
  return 0;
}

}  // namespace

extern "C" {

int iclr17_quantise_step_map(const float* y, int B, int h, int w, int N, const uint8_t* indices,
                             int log2_g, const float* steps, float* y_hat, float* y_deq,
                             int32_t* status, void* stream) {
  ICLR17_REQUIRE(y && indices && steps && y_hat && y_deq && status, ICLR17_EINVAL,
                 "quantise_step_map: null pointer");
  MapSteps src;
  const int rc = map_steps("quantise_step_map", B, h, w, N, indices, log2_g, steps, src);
  if (rc) return rc;
  const long n = (long)B * h * w * N;
  hipLaunchKernelGGL(quantise_kernel<MapSteps>, dim3(elementwise_blocks(n)), dim3(kThreads), 0,
                     (hipStream_t)stream, y, n, src, y_hat, y_deq, (int*)status);
  return check_launch("quantise_step_map");
}

int iclr17_dequantise_step_map(const float* y_hat, int B, int h, int w, int N,
                               const uint8_t* indices, int log2_g, const float* steps,
                               float* y_deq, void* stream) {
  ICLR17_REQUIRE(y_hat && indices && steps && y_deq, ICLR17_EINVAL,
                 "dequantise_step_map: null pointer");
  MapSteps src;
  const int rc = map_steps("dequantise_step_map", B, h, w, N, indices, log2_g, steps, src);
  if (rc) return rc;
  const long n = (long)B * h * w * N;
  hipLaunchKernelGGL(dequantise_kernel<MapSteps>, dim3(elementwise_blocks(n)), dim3(kThreads), 0,
                     (hipStream_t)stream, y_hat, n, src, y_deq);
  return check_launch("dequantise_step_map");
}

}  // extern "C"
