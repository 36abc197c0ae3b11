// Image files in and out of the codec: 8-bit HWC RGB images of any size ↔ the padded fp32 NCHW
// batch the analysis transform reads and the synthesis transform writes.
//   ingest: out[b,c,i,j] = float(src_b[min(i,H_b−1)][min(j,W_b−1)][c]) / 255  (ToTensor's division;
//           the image at the top left of the Hc×Wc canvas, bottom and right edges replicated)
//   egress: dst_b[i][j][c] = (uint8) rintf(clamp(recon[b,c,i,j], 0, 1) · 255) for the image's own
//           H_b×W_b region, optionally Σ (dst − ref)² per image (int64) and a non-finite status
//   sse:    the egress's sums and status alone, no pixel written (the probe of a quality target)
// The reference has no such step (train.py feeds fp32 crops); tests/test_gpu_image_io.py holds the
// contract as torch expressions.
//
// Both kernels: a workgroup of 4 waves covers 4 canvas rows × 256 columns, one row per wave and 4
// columns (16 bytes per fp32 plane) per lane. The 8-bit side of a row segment (≤ 768 bytes from an
// arbitrary byte address) goes through LDS so that global memory sees aligned dwords: whole
// dwords inside the segment move as dwords, the ≤ 3 bytes at either end as bytes, and nothing
// outside the segment is touched.
#include "common.h"

namespace iclr17 {
namespace {

constexpr int kCols = 256;               // columns per workgroup (4 per lane)
constexpr int kRows = 4;                 // rows per workgroup (one per wave)
constexpr int kSegBytes = 3 * kCols;     // 8-bit bytes of a full row segment
constexpr int kStage = kSegBytes + 16;   // + up to 3 bytes of alignment shift, 16-byte multiple

// int64 descriptor row per image: byte offset in the packed uint8 buffer, H, W, 0
enum : int { D_OFF = 0, D_H, D_W, D_N = 4 };

// This wave: n bytes from p (any alignment) → lds[sh .. sh + n), sh = p & 3 (returned): the LDS
// image is aligned like global memory. Publish with a barrier before other lanes read it.
__device__ __forceinline__ int stage_bytes(const unsigned char* __restrict__ p, int n,
                                           unsigned char* lds, int lane) {
  const int sh = (int)((uintptr_t)p & 3);
  const unsigned char* a = p - sh;
  for (int k = lane; 4 * k < sh + n; k += 64) {
    if (4 * k >= sh && 4 * k + 4 <= sh + n) {
      ((unsigned*)lds)[k] = *(const unsigned*)(a + 4 * k);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int o = 4 * k + t;
        if (o >= sh && o < sh + n) lds[o] = a[o];
      }
    }
  }
  return sh;
}

// This wave: lds[0 .. n) → n bytes at p (any alignment), the inverse of stage_bytes from an
// UNshifted LDS image: global dword k takes LDS bytes [4k − sh, 4k − sh + 4).
__device__ __forceinline__ void unstage_bytes(unsigned char* __restrict__ p, int n,
                                              const unsigned char* lds, int lane) {
  const int sh = (int)((uintptr_t)p & 3);
  unsigned char* a = p - sh;
  const unsigned* l32 = (const unsigned*)lds;
  for (int k = lane; 4 * k < sh + n; k += 64) {
    if (4 * k >= sh && 4 * k + 4 <= sh + n) {
      const unsigned hi = l32[k], lo = k > 0 ? l32[k - 1] : 0u;
      const unsigned long long both = ((unsigned long long)hi << 32) | lo;
      *(unsigned*)(a + 4 * k) = (unsigned)(both >> (8 * (4 - sh)));
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int o = 4 * k + t - sh;
        if (o >= 0 && o < n) a[4 * k + t] = lds[o];
      }
    }
  }
}

__device__ __forceinline__ int clampi(long v, int lo, int hi) {
  return v < lo ? lo : (v > hi ? hi : (int)v);
}

__global__ void __launch_bounds__(64 * kRows) image_ingest_kernel(
    const unsigned char* __restrict__ src, const long* __restrict__ desc, int Hc, int Wc,
    float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) unsigned char stage[kRows][kStage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, i = blockIdx.y * kRows + wave, j0 = blockIdx.x * kCols;
  const long* d = desc + (long)b * D_N;
  const int H = clampi(d[D_H], 1, Hc), W = clampi(d[D_W], 1, Wc);
  // the source columns this segment shows: [c_lo, c_lo + ncols), at least the last one
  const int si = i < H ? i : H - 1;
  const int c_lo = j0 < W ? j0 : W - 1;
  const int ncols = (j0 + kCols < W ? j0 + kCols : W) - c_lo;
  const unsigned char* row = src + d[D_OFF] + ((long)si * W + c_lo) * 3;
  const int sh = stage_bytes(row, 3 * ncols, stage[wave], lane);
  __syncthreads();
  const int j = j0 + 4 * lane;
  if (j >= Wc) return;
  const unsigned char* s = stage[wave] + sh;
  const long plane = (long)Hc * Wc;
  float* o = out + (long)b * 3 * plane + (long)i * Wc + j;
  f4 v[3];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int jj = (j + q < W ? j + q : W - 1) - c_lo;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c][q] = (float)s[3 * jj + c] / 255.0f;   // ToTensor: uint8 / 255
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) *(f4*)(o + c * plane) = v[c];
}

// WRITE = false is image_sse: the same pixels and the same sums, dst never touched.
template <bool REF, bool WRITE = true>
__global__ void __launch_bounds__(64 * kRows) image_egress_kernel(
    const float* __restrict__ recon, const long* __restrict__ desc, int Hc, int Wc,
    unsigned char* __restrict__ dst, const unsigned char* __restrict__ ref,
    unsigned long long* __restrict__ sse, int* __restrict__ status) {
  __shared__ __attribute__((aligned(16))) unsigned char pix[kRows][kSegBytes];
  __shared__ __attribute__((aligned(16))) unsigned char stage[REF ? kRows : 1][kStage];
  __shared__ int wave_sse[kRows];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.z, i = blockIdx.y * kRows + wave, j0 = blockIdx.x * kCols;
  const long* d = desc + (long)b * D_N;
  const int H = clampi(d[D_H], 1, Hc), W = clampi(d[D_W], 1, Wc);
  const bool active = i < H && j0 < W;   // wave-uniform; the padding is never looked at
  const int ncols = active ? (j0 + kCols < W ? j0 + kCols : W) - j0 : 0;
  const long seg = d[D_OFF] + ((long)i * W + j0) * 3;
  const int j = j0 + 4 * lane;
  int sh = 0;
  bool bad = false;
  if (active) {
    if constexpr (REF) sh = stage_bytes(ref + seg, 3 * ncols, stage[wave], lane);
    if (j < W) {
      const long plane = (long)Hc * Wc;
      const float* r = recon + (long)b * 3 * plane + (long)i * Wc + j;
      unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const f4 x = *(const f4*)(r + c * plane);   // inside the canvas; columns ≥ W unused
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (j + q < W) {
            bad |= (__float_as_uint(x[q]) & 0x7f800000u) == 0x7f800000u;
            const float y = rintf(fminf(fmaxf(x[q], 0.0f), 1.0f) * 255.0f);   // half to even
            const int t = 3 * q + c;
            w[t >> 2] |= (unsigned)y << (8 * (t & 3));
          }
        }
      }
      unsigned* p32 = (unsigned*)pix[wave] + 3 * lane;
      p32[0] = w[0];
      p32[1] = w[1];
      p32[2] = w[2];
    }
  }
  __syncthreads();
  int acc = 0;
  if (active) {
    if constexpr (REF) {
      if (j < W) {
        const unsigned char* a = pix[wave] + 12 * lane;
        const unsigned char* r8 = stage[wave] + sh + 12 * lane;
#pragma unroll
        for (int t = 0; t < 12; ++t) {
          if (j + t / 3 < W) {
            const int e = (int)a[t] - (int)r8[t];
            acc += e * e;
          }
        }
      }
    }
    if constexpr (WRITE) unstage_bytes(dst + seg, 3 * ncols, pix[wave], lane);
  }
  if (__any(bad) && lane == 0) atomicOr(status, 1);
  if constexpr (REF) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) wave_sse[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      // integer sums are associative: the total is the same bits in any arrival order
      unsigned long long s = 0;
#pragma unroll
      for (int k = 0; k < kRows; ++k) s += (unsigned long long)wave_sse[k];
      if (s != 0) atomicAdd(sse + b, s);
    }
  }
}

int check_canvas(const char* what, int B, int Hc, int Wc) {
  if (int rc = check_image(B, Hc, Wc, 128)) return rc;
  ICLR17_REQUIRE(B <= 65535 && Hc / kRows <= 65535, ICLR17_EUNSUPPORTED,
                 "%s: B=%d or canvas height %d beyond the launch grid", what, B, Hc);
  return ICLR17_OK;
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

int iclr17_image_ingest_u8(const uint8_t* src, const int64_t* desc, int B, int Hc, int Wc,
                           float* out, void* stream) {
  ICLR17_REQUIRE(src && desc && out, ICLR17_EINVAL, "image_ingest: null pointer");
  if (int rc = check_canvas("image_ingest", B, Hc, Wc)) return rc;
  const dim3 grid((Wc + kCols - 1) / kCols, Hc / kRows, B);
  hipLaunchKernelGGL(image_ingest_kernel, grid, dim3(64 * kRows), 0, (hipStream_t)stream,
                     (const unsigned char*)src, (const long*)desc, Hc, Wc, out);
  return check_launch("image_ingest");
}

int iclr17_image_egress_u8(const float* recon, const int64_t* desc, int B, int Hc, int Wc,
                           uint8_t* dst, const uint8_t* ref, int64_t* sse, int32_t* status,
                           void* stream) {
  ICLR17_REQUIRE(recon && desc && dst && status, ICLR17_EINVAL, "image_egress: null pointer");
  ICLR17_REQUIRE(!ref || sse, ICLR17_EINVAL, "image_egress: sse required with ref");
  if (int rc = check_canvas("image_egress", B, Hc, Wc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e == hipSuccess && sse) e = hipMemsetAsync(sse, 0, (size_t)B * sizeof(int64_t), st);
  if (e != hipSuccess) {
    set_error(ICLR17_ELAUNCH, "image_egress: %s", hipGetErrorString(e));
    return ICLR17_ELAUNCH;
  }
  const dim3 grid((Wc + kCols - 1) / kCols, Hc / kRows, B);
  if (ref)
    hipLaunchKernelGGL(image_egress_kernel<true>, grid, dim3(64 * kRows), 0, st, recon,
                       (const long*)desc, Hc, Wc, (unsigned char*)dst, (const unsigned char*)ref,
                       (unsigned long long*)sse, (int*)status);
  else
    hipLaunchKernelGGL(image_egress_kernel<false>, grid, dim3(64 * kRows), 0, st, recon,
                       (const long*)desc, Hc, Wc, (unsigned char*)dst, (const unsigned char*)nullptr,
                       (unsigned long long*)nullptr, (int*)status);
  return check_launch("image_egress");
}

int iclr17_image_sse_u8(const float* recon, const int64_t* desc, int B, int Hc, int Wc,
                        const uint8_t* ref, int64_t* sse, int32_t* status, void* stream) {
  ICLR17_REQUIRE(recon && desc && ref && sse && status, ICLR17_EINVAL, "image_sse: null pointer");
  if (int rc = check_canvas("image_sse", B, Hc, Wc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(sse, 0, (size_t)B * sizeof(int64_t), st);
  if (e != hipSuccess) {
    set_error(ICLR17_ELAUNCH, "image_sse: %s", hipGetErrorString(e));
    return ICLR17_ELAUNCH;
  }
  const dim3 grid((Wc + kCols - 1) / kCols, Hc / kRows, B);
  hipLaunchKernelGGL((image_egress_kernel<true, false>), grid, dim3(64 * kRows), 0, st, recon,
                     (const long*)desc, Hc, Wc, (unsigned char*)nullptr,
                     (const unsigned char*)ref, (unsigned long long*)sse, (int*)status);
  return check_launch("image_sse");
}

}  // extern "C"
