// MS-SSIM on the GPU — models/ms_ssim_torch.py:5-196 as train.py:178 calls it
// (ms_ssim(clipped, x, data_range=1.0): 11-tap σ=1.5 Gaussian, 5 levels, weights
// 0.0448 0.2856 0.3001 0.2363 0.1333), per image.
//
// Per level one kernel does the whole SSIM: a 16×64 output tile of one image plane stages its
// 26×74 input window of X and Y in LDS (49 KB: 3 workgroups per CU; 32×64 tiles were 1.5 %
// slower at 2), runs the separable 'valid' filter (along W, then along
// H — the reference's order) on X, Y, X², Y² and XY, forms the cs and ssim maps and leaves one
// partial sum per tile. Both passes slide the window in registers (a W-pass thread filters 4
// consecutive columns of a row from 14 loaded values, an H-pass thread 4 consecutive rows of a
// column from 14), so each filtered value costs ~2 LDS reads instead of 11; every output keeps
// the reference's tap order. A second kernel does the 2×2 average pooling (one zero row/column
// of padding on odd sizes, counted in the average: avg_pool2d's defaults), and a last one, one
// workgroup per image, reduces the per-tile partials of all levels (fixed-order trees: results
// are bitwise reproducible) and forms
//   ms_ssim = Π_{l<4} (cs_l^w_l · ssim_4^w_4)
// exactly as ms_ssim_torch.py:189-190 does (the last level's ssim enters every factor; its cs is
// unused).
//
// The gradient path (the loss λ·(1 − MS-SSIM) + bpp; "Backward" below): saving variants of the
// level kernel also write the per-pixel derivative maps, and one backward kernel per level, from
// the coarsest up, turns them into dX / dY.
//
// iclr17_image_msssim_u8 (the probe of an MS-SSIM target) runs the same level,
// pooling and finish kernels over a canvas batch of the image codec: images of different true
// sizes, measured each over its own H×W on the 8-bit decode ("extent sources" below).
// iclr17_image_msssim_u8_fwd_saved / _bwd (the distortion gradient of latent refinement for
// MS-SSIM) run the gradient path over the same sources: the gradient on recon,
// straight through the 8-bit rounding, gated at the clamp, zero on the canvas padding.
#include <string.h>

#include "common.h"

namespace iclr17 {
namespace {

constexpr int WIN = 11, TOH = 16, TOW = 64;
constexpr int IH = TOH + WIN - 1, IW = TOW + WIN - 1;   // 26 × 74 input window at TOH = 16
constexpr int IWP = 76;                                 // LDS row stride: 16-byte rows
constexpr int RS = TOH / 4;                             // H-pass rows per thread (wave = strip)
constexpr int LEVELS = 5;
__constant__ float c_msssim_w[LEVELS] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
// The reference's fp32 window (ms_ssim_torch.py:5-18: exp(−c²/(2·1.5²)) normalised by its sum,
// evaluated by torch-CPU fp32), bit for bit (tests/test_library.py recomputes it from the oracle).
__constant__ float c_gauss[WIN] = {
    0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
    0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f};

struct Level {
  int H, W;         // input size of the level
  long off;         // offset of the level's planes in the pyramid buffer (floats; level 0: -1)
  int tiles;        // output tiles per plane
};

// What the finish kernel sums for image b at level l: n(l, b) partial pairs from first(l, b),
// divided by mean_over(l, b).
struct FinishPlan {
  long poff[LEVELS];     // first partial (doubles) of each level
  int tiles[LEVELS];     // tiles per plane
  double count[LEVELS];  // 3 · Ho · Wo
  __device__ __forceinline__ long n(int l, int) const { return 3L * tiles[l]; }
  __device__ __forceinline__ long first(int l, int b) const { return poff[l] + 2 * (long)b * n(l, b); }
  __device__ __forceinline__ double mean_over(int l, int) const { return count[l]; }
};

// g·v + acc: one fused multiply-add (the filter's rounding differs from the reference's
// torch-CPU convolution either way; MS-SSIM parity is a 1e-5 relative tolerance)
__device__ __forceinline__ float fmac(float g, float v, float acc) {
  return __builtin_fmaf(g, v, acc);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// F.avg_pool2d(kernel 2, stride 2, padding n % 2): the next level's size
__host__ __device__ inline int pooled(int n) { return (n + 2 * (n % 2) - 2) / 2 + 1; }

// ------------------------------------------------------------------------- extent sources
// The level, pooling and finish kernels are one body over an *extent source*, which says where a
// plane's size and pixels come from (as ladder.h's step sources do for Δ):
//   Uniform      every plane of the batch is H×W, dense fp32: iclr17_ms_ssim and the gradient path
//   ImageU8      a canvas batch of the image codec at level 0: plane 3b + c is image b's own
//                H_b×W_b (the descriptors) of the 8-bit decode of recon and of the packed uint8
//                original, converted as they are read; no level-0 plane exists in memory
//   ImagePlanes  the same batch at levels ≥ 1: image b's level size follows from its descriptor by
//                `pooled`, its planes lie dense (row stride = its own width) in a slot of the
//                canvas's level size
// view(plane) gives the plane: H, W, x(r, c, bad) and y(r, c). A ragged source (kRagged) is
// launched on the grid of the canvas; a workgroup beyond the image's own grid returns before any
// barrier, and an image's partials are indexed by its own tile grid in (plane, tile row, tile
// column) order from the first slot of the image, so that they are the partials, in the order,
// of that image as a Uniform batch of one.
//
// The gradient path adds: map_slot(Ho, Wo), the floats between the derivative maps of two planes
// (a ragged source: the canvas's map size at the level, an image's maps dense at its own size in
// the front of its slot, as its pyramid planes are), and for the backward at(r, c), where the
// gradient of pixel (r, c) goes, gate(r, c, d), what is stored for the gradient d there, and
// kFill: the view's output is a whole canvas plane, whose padding the backward zeroes.
struct PlaneView {
  static constexpr bool kFill = false;
  int H, W;
  const float* __restrict__ xp;
  const float* __restrict__ yp;
  long po;   // the plane's first float in a buffer laid out as the source's
  __device__ __forceinline__ float x(int r, int c, bool&) const { return xp[(long)r * W + c]; }
  __device__ __forceinline__ float y(int r, int c) const { return yp[(long)r * W + c]; }
  __device__ __forceinline__ long at(int r, int c) const { return po + (long)r * W + c; }
  __device__ __forceinline__ float gate(int, int, float d) const { return d; }
};

struct Uniform {
  static constexpr bool kRagged = false;
  const float* __restrict__ X;
  const float* __restrict__ Y;
  int H, W;
  __device__ __forceinline__ PlaneView view(int plane) const {
    const long po = (long)plane * H * W;
    return PlaneView{H, W, X + po, Y + po, po};
  }
  __device__ __forceinline__ void report(bool) const {}
  __device__ __forceinline__ long map_slot(int Ho, int Wo) const { return (long)Ho * Wo; }
};

// int64 descriptor row per image (imageio.hip): byte offset in the packed uint8 buffer, H, W, 0
constexpr int kDescOff = 0, kDescH = 1, kDescW = 2, kDescN = 4;

struct Extent {
  int H, W;
};

// image b's size at `level`, from its (host-checked) descriptor, kept inside the canvas
__device__ __forceinline__ Extent image_extent(const long* __restrict__ desc, int b, int Hc, int Wc,
                                               int level) {
  const long h = desc[(long)b * kDescN + kDescH], w = desc[(long)b * kDescN + kDescW];
  Extent e{h < 1 ? 1 : (h > Hc ? Hc : (int)h), w < 1 ? 1 : (w > Wc ? Wc : (int)w)};
  for (int l = 0; l < level; ++l) {
    e.H = pooled(e.H);
    e.W = pooled(e.W);
  }
  return e;
}

// X = the byte image_egress_u8 writes and Y = the original's byte, each times fl(1/255): the planes
// codec.evaluate_images feeds iclr17_ms_ssim (torch divides a device tensor by the scalar 255 as
// the product with the fp32 reciprocal, which is not the quotient for 126 of the 256 bytes), so
// that a value here is the value reported there. bad: a recon value that is not finite.
constexpr float kInv255 = 1.0f / 255.0f;

struct U8View {
  static constexpr bool kFill = true;
  int H, W, Wc;
  const float* __restrict__ rp;            // recon plane [Hc][Wc]
  const unsigned char* __restrict__ yp;    // the image's HWC bytes, from this channel's first
  long po;                                 // the plane's first float in a [B][3][Hc][Wc] buffer
  __device__ __forceinline__ float x(int r, int c, bool& bad) const {
    const float v = rp[(long)r * Wc + c];
    bad |= (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
    return rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f) * kInv255;
  }
  __device__ __forceinline__ float y(int r, int c) const {
    return (float)yp[((long)r * W + c) * 3] * kInv255;
  }
  __device__ __forceinline__ long at(int r, int c) const { return po + (long)r * Wc + c; }
  // straight through the rounding, gated at the clamp: a descent step along −d would only push a
  // clamped value further out
  __device__ __forceinline__ float gate(int r, int c, float d) const {
    const float v = rp[(long)r * Wc + c];
    return ((v < 0.0f && d > 0.0f) || (v > 1.0f && d < 0.0f)) ? 0.0f : d;
  }
};

struct ImageU8 {
  static constexpr bool kRagged = true;
  const float* __restrict__ recon;
  const long* __restrict__ desc;
  const unsigned char* __restrict__ ref;
  int Hc, Wc;
  int* __restrict__ status;
  long mslot = 0;   // the gradient path's: (Hc − 10)·(Wc − 10)
  __device__ __forceinline__ U8View view(int plane) const {
    const int b = plane / 3, c = plane - 3 * b;
    const Extent e = image_extent(desc, b, Hc, Wc, 0);
    const long po = (long)plane * Hc * Wc;
    return U8View{e.H, e.W, Wc, recon + po, ref + desc[(long)b * kDescN + kDescOff] + c, po};
  }
  __device__ __forceinline__ void report(bool bad) const {
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, 1);
  }
  __device__ __forceinline__ long map_slot(int, int) const { return mslot; }
};

struct ImagePlanes {
  static constexpr bool kRagged = true;
  const float* __restrict__ X;    // the level's X and Y slots: `slot` floats per plane
  const float* __restrict__ Y;
  long slot;
  const long* __restrict__ desc;
  int Hc, Wc, level;
  long mslot = 0;   // the gradient path's: the canvas's map size at the level
  __device__ __forceinline__ PlaneView view(int plane) const {
    const Extent e = image_extent(desc, plane / 3, Hc, Wc, level);
    const long po = (long)plane * slot;
    return PlaneView{e.H, e.W, X + po, Y + po, po};
  }
  __device__ __forceinline__ void report(bool) const {}
  __device__ __forceinline__ long map_slot(int, int) const { return mslot; }
};

// The finish of a canvas batch: `canvas` is the plan of the canvas (where an image's partials
// start); the image sums the 3·tiles of its own grid, as its Uniform batch of one would.
struct ImageFinish {
  FinishPlan canvas;
  const long* __restrict__ desc;
  int Hc, Wc;
  __device__ __forceinline__ Extent maps(int l, int b) const {   // Ho × Wo
    const Extent e = image_extent(desc, b, Hc, Wc, l);
    return Extent{e.H - (WIN - 1), e.W - (WIN - 1)};
  }
  __device__ __forceinline__ long n(int l, int b) const {
    const Extent o = maps(l, b);
    if (o.H <= 0 || o.W <= 0) return 0;   // too small for the level (the host wrapper rejects it)
    return 3L * ((o.W + TOW - 1) / TOW) * ((o.H + TOH - 1) / TOH);
  }
  __device__ __forceinline__ long first(int l, int b) const {
    return canvas.poff[l] + 2 * (long)b * 3 * canvas.tiles[l];
  }
  __device__ __forceinline__ double mean_over(int l, int b) const {
    const Extent o = maps(l, b);
    return 3.0 * o.H * o.W;
  }
};

// SAVE (the gradient path, see "Backward" below): bit 0 also writes the per-pixel derivatives of
// the cs map, bit 1 those of the ssim map, to dcs / dss as planes [map][plane][map_slot] with
// map 0 = ∂/∂mx, 1 = ∂/∂exx (= ∂/∂eyy), 2 = ∂/∂exy and, with want_dy, 3 = ∂/∂my. SAVE = 0 is the
// evaluation kernel; the partial sums and their arithmetic are the same in every variant.
template <int SAVE, class Ext>
__global__ void __launch_bounds__(256, 2) ssim_level_kernel(const Ext ext, float c1, float c2,
                                                            double* __restrict__ partial,
                                                            float* __restrict__ dcs,
                                                            float* __restrict__ dss, int want_dy) {
  __shared__ __attribute__((aligned(16))) float sx[IH * IWP], sy[IH * IWP];
  __shared__ __attribute__((aligned(16))) float h[5][IH][TOW];
  __shared__ double red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = blockIdx.z;
  const auto pv = ext.view(plane);
  const int H = pv.H, W = pv.W;
  const int Ho = H - (WIN - 1), Wo = W - (WIN - 1);
  // the plane's own tile grid and its first partial
  int tgx = gridDim.x, tgy = gridDim.y;
  long tile0 = (long)plane * gridDim.y * gridDim.x;
  if constexpr (Ext::kRagged) {
    tgx = (Wo + TOW - 1) / TOW;
    tgy = (Ho + TOH - 1) / TOH;
    if ((int)blockIdx.x >= tgx || (int)blockIdx.y >= tgy) return;   // uniform over the workgroup
    const int img = plane / 3;
    tile0 = 3L * img * gridDim.y * gridDim.x + (long)(plane - 3 * img) * tgy * tgx;
  }
  const int r0 = blockIdx.y * TOH, c0 = blockIdx.x * TOW;
  float g[WIN];
#pragma unroll
  for (int k = 0; k < WIN; ++k) g[k] = c_gauss[k];

  bool bad = false;
  for (int i = tid; i < IH * IW; i += 256) {
    const int r = i / IW, c = i - r * IW;
    const int gr = r0 + r, gc = c0 + c;
    const bool ok = gr < H && gc < W;
    sx[r * IWP + c] = ok ? pv.x(gr, gc, bad) : 0.f;
    sy[r * IWP + c] = ok ? pv.y(gr, gc) : 0.f;
  }
  ext.report(bad);
  __syncthreads();
  // along W: 42 rows × 16 column quads; a thread filters columns cq .. cq+3 of row r
  for (int task = tid; task < IH * (TOW / 4); task += 256) {
    const int r = task >> 4, cq = (task & 15) * 4;
    float xv[16], yv[16];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const f4 a = *(const f4*)(sx + r * IWP + cq + 4 * v);
      const f4 b = *(const f4*)(sy + r * IWP + cq + 4 * v);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xv[4 * v + e] = a[e];
        yv[4 * v + e] = b[e];
      }
    }
    f4 o[5];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float ax = 0.f, ay = 0.f, axx = 0.f, ayy = 0.f, axy = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) {
        const float xk = xv[j + k], yk = yv[j + k];
        ax = fmac(g[k], xk, ax);
        ay = fmac(g[k], yk, ay);
        axx = fmac(g[k], xk * xk, axx);
        ayy = fmac(g[k], yk * yk, ayy);
        axy = fmac(g[k], xk * yk, axy);
      }
      o[0][j] = ax;
      o[1][j] = ay;
      o[2][j] = axx;
      o[3][j] = ayy;
      o[4][j] = axy;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) *(f4*)(&h[q][r][cq]) = o[q];
  }
  __syncthreads();
  // along H: wave w filters rows RS·w .. RS·w + RS − 1 of column lane, then the maps
  // (ms_ssim_torch.py:59-73)
  const int rs = wave * RS;
  float m[5][RS];
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    float v[RS + WIN - 1];
#pragma unroll
    for (int i = 0; i < RS + WIN - 1; ++i) v[i] = h[q][rs + i][lane];
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) acc = fmac(g[k], v[j + k], acc);
      m[q][j] = acc;
    }
  }
  double s_ssim = 0.0, s_cs = 0.0;
  if (c0 + lane < Wo) {
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      if (r0 + rs + j >= Ho) break;
      const float mx = m[0][j], my = m[1][j];
      const float mxx = mx * mx, myy = my * my, mxy = mx * my;
      const float vx = 1.0f * (m[2][j] - mxx), vy = 1.0f * (m[3][j] - myy),
                  cxy = 1.0f * (m[4][j] - mxy);
      const float cs = (2.0f * cxy + c2) / (vx + vy + c2);
      const float ssim = ((2.0f * mxy + c1) / (mxx + myy + c1)) * cs;
      s_ssim += (double)ssim;
      s_cs += (double)cs;
      if constexpr (SAVE != 0) {
        const float D = vx + vy + c2, E = mxx + myy + c1;
        const float L = (2.0f * mxy + c1) / E;
        const float c_exy = 2.0f / D, c_exx = -cs / D;
        const float c_mx = (2.0f * cs * mx - 2.0f * my) / D;
        const float c_my = (2.0f * cs * my - 2.0f * mx) / D;
        const long slot = ext.map_slot(Ho, Wo);
        const long ms = (long)gridDim.z * slot;   // one map of every plane
        const long at = (long)plane * slot + (long)(r0 + rs + j) * Wo + (c0 + lane);
        if constexpr ((SAVE & 1) != 0) {
          dcs[at] = c_mx;
          dcs[ms + at] = c_exx;
          dcs[2 * ms + at] = c_exy;
          if (want_dy) dcs[3 * ms + at] = c_my;
        }
        if constexpr ((SAVE & 2) != 0) {
          dss[at] = cs * (2.0f * my - 2.0f * L * mx) / E + L * c_mx;
          dss[ms + at] = L * c_exx;
          dss[2 * ms + at] = L * c_exy;
          if (want_dy) dss[3 * ms + at] = cs * (2.0f * mx - 2.0f * L * my) / E + L * c_my;
        }
      }
    }
  }
  s_ssim = wave_sum_d(s_ssim);
  s_cs = wave_sum_d(s_cs);
  if (lane == 0) {
    red[0][wave] = s_ssim;
    red[1][wave] = s_cs;
  }
  __syncthreads();
  if (tid == 0) {
    const long tile = tile0 + (long)blockIdx.y * tgx + blockIdx.x;
    partial[2 * tile] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    partial[2 * tile + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// F.avg_pool2d(kernel 2, stride 2, padding (H % 2, W % 2)), count_include_pad: /4 always.
// grid (⌈Wo/256⌉, Ho, 2P): output row oy of plane z % P of X (z < P) or Y. The output planes are
// dense (row stride Wo), `out_plane` floats apart: Ho·Wo, or a ragged source's next slot, on whose
// canvas grid a row or column beyond the image's own output returns.
template <class Ext>
__global__ void __launch_bounds__(256) avgpool2_kernel(const Ext ext, int P, long out_plane,
                                                       float* __restrict__ outx,
                                                       float* __restrict__ outy) {
  const int z = blockIdx.z;
  const int p = z < P ? z : z - P;
  const auto pv = ext.view(p);
  const int H = pv.H, W = pv.W;
  const int ph = H % 2, pw = W % 2;
  const int Ho = pooled(H), Wo = pooled(W);
  const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
  if (ox >= Wo || oy >= Ho) return;
  float s = 0.f;
  bool bad = false;   // the level kernel of the source's level reports it
  for (int dy = 0; dy < 2; ++dy)
    for (int dx = 0; dx < 2; ++dx) {
      const int iy = 2 * oy - ph + dy, ix = 2 * ox - pw + dx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) s += z < P ? pv.x(iy, ix, bad) : pv.y(iy, ix);
    }
  (z < P ? outx : outy)[(long)p * out_plane + (long)oy * Wo + ox] = s / 4.0f;
}

// One workgroup per image: the per-level means (Σ over the 3 planes × tiles, a fixed-order
// strided sum + tree, / (3·Ho·Wo)) and the MS-SSIM product.
template <class Plan>
__global__ void __launch_bounds__(256) msssim_finish_kernel(const double* __restrict__ partial,
                                                            const Plan pl, int B,
                                                            double* __restrict__ means /* [L][B][2] */,
                                                            float* __restrict__ out) {
  __shared__ double red[2][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int l = 0; l < LEVELS; ++l) {
    const long n = pl.n(l, b);
    const double* p = partial + pl.first(l, b);
    const double count = pl.mean_over(l, b);
    double a = 0.0, c = 0.0;
    for (long t = tid; t < n; t += 256) {
      a += p[2 * t];
      c += p[2 * t + 1];
    }
    red[0][tid] = a;
    red[1][tid] = c;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        red[0][tid] += red[0][tid + s];
        red[1][tid] += red[1][tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      means[((long)l * B + b) * 2] = red[0][0] / count;
      means[((long)l * B + b) * 2 + 1] = red[1][0] / count;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float ssim_last = (float)means[((long)(LEVELS - 1) * B + b) * 2];
    float prod = 1.0f;
    for (int l = 0; l < LEVELS - 1; ++l) {
      const float cs = (float)means[((long)l * B + b) * 2 + 1];
      prod = prod * (powf(cs, c_msssim_w[l]) * powf(ssim_last, c_msssim_w[LEVELS - 1]));
    }
    out[b] = prod;
  }
}

// Single-scale SSIM (ms_ssim_torch.py:86-120 → _ssim :36-83 with size_average=False, full=True):
// per image the means of the ssim and cs maps over C·Ho·Wo, the same fixed-order sums as above.
__global__ void __launch_bounds__(256) ssim_finish_kernel(const double* __restrict__ partial,
                                                          long tiles3, double count,
                                                          float* __restrict__ out_ssim,
                                                          float* __restrict__ out_cs) {
  __shared__ double red[2][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* p = partial + 2 * (long)b * tiles3;
  double a = 0.0, c = 0.0;
  for (long t = tid; t < tiles3; t += 256) {
    a += p[2 * t];
    c += p[2 * t + 1];
  }
  red[0][tid] = a;
  red[1][tid] = c;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) {
      red[0][tid] += red[0][tid + s];
      red[1][tid] += red[1][tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out_ssim[b] = (float)(red[0][0] / count);
    if (out_cs) out_cs[b] = (float)(red[1][0] / count);
  }
}

// ------------------------------------------------------------------------------- Backward
// The saving forward (ssim_level_kernel<SAVE>) leaves, per level, the per-pixel derivatives of the
// map whose mean enters the result (cs for levels 0-3, ssim for level 4; both for single-scale
// SSIM). The upstream gradient on a map is one scalar per image (coef), so
//   dX(q) = (Gᵀ d_mx)(q) + 2·X(q)·(Gᵀ d_exx)(q) + Y(q)·(Gᵀ d_exy)(q)         (dY: x ↔ y, d_eyy = d_exx)
// with Gᵀ the 'full' separable correlation of the Ho×Wo map (zero outside) into H×W; the window is
// symmetric, so it is the forward's 'valid' filter over the zero-padded map. Nothing is scattered:
// every sum has a fixed order and the gradients are bitwise reproducible.

// coef[l][b] = g[b] · ∂M/∂mean_l / (3·Ho_l·Wo_l) for M = Π_{l<4} (C_l^{w_l} · S_4^{w_4}), chained
// as torch differentiates prod (M / t_l), mul and pow (w·v^{w−1}), in double from the fp32 means
// the forward used. Nothing is clamped: a non-positive mean gives NaN, as in the reference.
// Plan: the finish kernel's, for its mean_over (an image of a canvas batch: its own counts).
template <class Plan>
__global__ void msssim_coef_kernel(const double* __restrict__ means /* [L][B][2] */,
                                   const float* __restrict__ g, const Plan pl, int B,
                                   float* __restrict__ coef /* [L][B] */) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double w4 = (double)c_msssim_w[LEVELS - 1];
  const double s = (double)(float)means[((long)(LEVELS - 1) * B + b) * 2];
  const double sp = pow(s, w4);
  double a[LEVELS - 1], t[LEVELS - 1], M = 1.0;
  for (int l = 0; l < LEVELS - 1; ++l) {
    a[l] = pow((double)(float)means[((long)l * B + b) * 2 + 1], (double)c_msssim_w[l]);
    t[l] = a[l] * sp;
    M *= t[l];
  }
  const double gb = (double)g[b];
  double dsp = 0.0;
  for (int l = 0; l < LEVELS - 1; ++l) {
    const double gt = gb * (M / t[l]);
    const double cs = (double)(float)means[((long)l * B + b) * 2 + 1], w = (double)c_msssim_w[l];
    coef[(long)l * B + b] = (float)(gt * sp * (w * pow(cs, w - 1.0)) / pl.mean_over(l, b));
    dsp += gt * a[l];
  }
  coef[(long)(LEVELS - 1) * B + b] =
      (float)(dsp * (w4 * pow(s, w4 - 1.0)) / pl.mean_over(LEVELS - 1, b));
}

// Single-scale: coef[0][b] = g_ssim[b] / count, coef[1][b] = g_cs[b] / count (a null g: unused).
__global__ void ssim_coef_kernel(const float* __restrict__ g_ssim, const float* __restrict__ g_cs,
                                 double count, int B, float* __restrict__ coef /* [2][B] */) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (g_ssim) coef[b] = (float)((double)g_ssim[b] / count);
  if (g_cs) coef[B + b] = (float)((double)g_cs[b] / count);
}

// One level of the backward: a workgroup owns a 16×64 tile of dX (and dY) of one plane. Per map it
// stages the 26×74 window of the derivative map (tile + 10 rows above / columns left, zero outside
// the map), scaled by the image's coefficient (two sets, DA·ca + DB·cb, when single-scale SSIM
// has gradients on both ssim and cs), runs the forward's two register-sliding filter passes, and
// keeps the 4 filtered values per thread; then the pointwise combination with X and Y and the
// average pooling's backward from the level below,
//   0.25 · d_{l+1}[(iy + H%2)/2][(ix + W%2)/2]   (every pixel lies in exactly one pooling window).
// grid (⌈W/64⌉, ⌈H/16⌉, planes). dX / dY null: not wanted.
//
// One body over the extent source, as the forward: X and Y come from the plane's view (at level 0
// of a canvas batch they are recomputed from recon and the original's bytes), the maps of plane p
// start at p·map_slot, and the level below is the plane's own pooled size in slots of `pool_slot`
// floats. A ragged source is launched on the canvas's grid: a workgroup beyond the image's own
// H×W returns, after zeroing its tile where the output is the canvas itself (kFill), as does a
// thread beyond the image inside a workgroup that covers its edge.
template <class Ext>
__global__ void __launch_bounds__(256, 2) ssim_level_bwd_kernel(
    const Ext ext, const float* __restrict__ DA, const float* __restrict__ coefA,
    const float* __restrict__ DB, const float* __restrict__ coefB,
    const float* __restrict__ poolX, const float* __restrict__ poolY, long pool_slot,
    float* __restrict__ dX, float* __restrict__ dY) {
  __shared__ __attribute__((aligned(16))) float sd[IH * IWP];
  __shared__ __attribute__((aligned(16))) float h[IH][TOW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int plane = blockIdx.z, img = plane / 3;
  const auto pv = ext.view(plane);
  constexpr bool kFill = decltype(pv)::kFill;
  const int H = pv.H, W = pv.W;
  const int Ho = H - (WIN - 1), Wo = W - (WIN - 1);
  const int r0 = blockIdx.y * TOH, c0 = blockIdx.x * TOW;
  const int rs = wave * RS;
  if constexpr (Ext::kRagged) {
    if (r0 >= H || c0 >= W) {   // uniform over the workgroup
      if constexpr (kFill) {
        const int col = c0 + lane;
#pragma unroll
        for (int j = 0; j < RS; ++j) {
          const int row = r0 + rs + j;
          if (row < ext.Hc && col < ext.Wc) {
            if (dX) dX[pv.at(row, col)] = 0.f;
            if (dY) dY[pv.at(row, col)] = 0.f;
          }
        }
      }
      return;
    }
  }
  const long slot = ext.map_slot(Ho, Wo);
  const long ms = (long)gridDim.z * slot;
  const float ca = coefA[img], cb = DB ? coefB[img] : 0.f;
  float g[WIN];
#pragma unroll
  for (int k = 0; k < WIN; ++k) g[k] = c_gauss[k];
  float m[4][RS];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int j = 0; j < RS; ++j) m[q][j] = 0.f;
    if ((q == 0 && !dX) || (q == 3 && !dY)) continue;   // uniform over the grid
    const float* da = DA + q * ms + (long)plane * slot;
    const float* db = DB ? DB + q * ms + (long)plane * slot : nullptr;
    // (sd is free: the barrier before the previous map's H pass followed its W pass)
    for (int i = tid; i < IH * IW; i += 256) {
      const int r = i / IW, c = i - r * IW;
      const int gr = r0 - (WIN - 1) + r, gc = c0 - (WIN - 1) + c;
      float v = 0.f;
      if (gr >= 0 && gr < Ho && gc >= 0 && gc < Wo) {
        v = ca * da[(long)gr * Wo + gc];
        if (db) v += cb * db[(long)gr * Wo + gc];
      }
      sd[r * IWP + c] = v;
    }
    __syncthreads();   // also: the previous map's H pass has read h
    for (int task = tid; task < IH * (TOW / 4); task += 256) {
      const int r = task >> 4, cq = (task & 15) * 4;
      float v[16];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f4 a = *(const f4*)(sd + r * IWP + cq + 4 * u);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * u + e] = a[e];
      }
      f4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) acc = fmac(g[k], v[j + k], acc);
        o[j] = acc;
      }
      *(f4*)(&h[r][cq]) = o;
    }
    __syncthreads();
    float v[RS + WIN - 1];
#pragma unroll
    for (int i = 0; i < RS + WIN - 1; ++i) v[i] = h[rs + i][lane];
#pragma unroll
    for (int j = 0; j < RS; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < WIN; ++k) acc = fmac(g[k], v[j + k], acc);
      m[q][j] = acc;
    }
  }
  const int col = c0 + lane;
  const int ph = H % 2, pw = W % 2;
  const int Wn = pooled(W);
#pragma unroll
  for (int j = 0; j < RS; ++j) {
    const int row = r0 + rs + j;
    if (row < H && col < W) {
      const long at = pv.at(row, col);
      const long pat = (long)plane * pool_slot + (long)((row + ph) / 2) * Wn + (col + pw) / 2;
      bool bad = false;   // the forward reported it
      const float x = pv.x(row, col, bad), y = pv.y(row, col);
      if (dX) {
        float d = (m[0][j] + 2.0f * x * m[1][j]) + y * m[2][j];
        if (poolX) d += 0.25f * poolX[pat];
        dX[at] = pv.gate(row, col, d);
      }
      if (dY) {
        float d = (m[3][j] + 2.0f * y * m[1][j]) + x * m[2][j];
        if (poolY) d += 0.25f * poolY[pat];
        dY[at] = d;
      }
    } else if constexpr (kFill) {
      if (row < ext.Hc && col < ext.Wc) {
        if (dX) dX[pv.at(row, col)] = 0.f;
        if (dY) dY[pv.at(row, col)] = 0.f;
      }
    }
  }
}

int level_plan(int H, int W, Level* lv, int B, long* pyr_floats, long* partial_doubles,
               int levels = LEVELS) {
  long off = 0, part = 0;
  for (int l = 0; l < levels; ++l) {
    if (H < WIN || W < WIN) return -1;
    lv[l].H = H;
    lv[l].W = W;
    lv[l].off = l == 0 ? -1 : off;
    if (l > 0) off += 2L * B * 3 * H * W;   // X and Y planes of this level
    lv[l].tiles = ((W - WIN + 1 + TOW - 1) / TOW) * ((H - WIN + 1 + TOH - 1) / TOH);
    part += 2L * B * 3 * lv[l].tiles;
    H = pooled(H);
    W = pooled(W);
  }
  *pyr_floats = off;
  *partial_doubles = part;
  return 0;
}

// Workspace of the gradient path, from its 256-byte aligned base:
//   partial doubles | means [levels][B][2] doubles | pyramid of X, Y (levels ≥ 1) | pyramid of
//   dX, dY (levels ≥ 1, the backward's) | derivative maps | coef floats
// The maps of level l: MS-SSIM one set of nmaps (3, with dY 4) planes-of-every-image; single-scale
// two sets (ssim, then cs).
struct GradPlan {
  Level lv[LEVELS];
  int levels, nmaps;
  long pyr, part;
  long maps[LEVELS];   // first float of the level's maps
  size_t off_means, off_pyr, off_gpyr, off_maps, off_coef, bytes;
};

int grad_plan(int B, int H, int W, int want_dy, int multiscale, GradPlan* gp) {
  gp->levels = multiscale ? LEVELS : 1;
  gp->nmaps = want_dy ? 4 : 3;
  if (B <= 0 || level_plan(H, W, gp->lv, B, &gp->pyr, &gp->part, gp->levels) != 0) return -1;
  long maps = 0;
  for (int l = 0; l < gp->levels; ++l) {
    gp->maps[l] = maps;
    maps += (multiscale ? 1L : 2L) * gp->nmaps * B * 3 * (gp->lv[l].H - WIN + 1) *
            (gp->lv[l].W - WIN + 1);
  }
  gp->off_means = (size_t)gp->part * 8;
  gp->off_pyr = gp->off_means + (size_t)gp->levels * B * 2 * 8;
  gp->off_gpyr = gp->off_pyr + (size_t)gp->pyr * 4;
  gp->off_maps = gp->off_gpyr + (size_t)gp->pyr * 4;
  gp->off_coef = gp->off_maps + (size_t)maps * 4;
  gp->bytes = gp->off_coef + (size_t)(multiscale ? LEVELS : 2) * B * 4 + 256;
  return 0;
}

char* aligned_base(void* workspace) {
  return (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
}

// The forward of a canvas batch, for iclr17_image_msssim_u8 and its saving twin: the same
// launches on the same partials in the same order. The pyramid, the partials and the means are
// laid out for B images of the canvas's size (lv); an image uses the front of each of its slots.
// maps (null: the evaluation kernels): the level's derivative maps go to maps + map_off[l].
int image_msssim_levels(const char* what, const float* recon, const long* d, int B, int Hc, int Wc,
                        const unsigned char* ref, const Level* lv, double* partial, double* means,
                        float* pyrbuf, float* maps, const long* map_off, float* out,
                        int32_t* status, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
  if (e != hipSuccess) {
    set_error(ICLR17_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return ICLR17_ELAUNCH;
  }
  const float data_range = 1.0f;
  const float c1 = (0.01f * data_range) * (0.01f * data_range);
  const float c2 = (0.03f * data_range) * (0.03f * data_range);
  double* pl = partial;
  ImageFinish fin{{}, d, Hc, Wc};
  for (int l = 0; l < LEVELS; ++l) {
    const int Hl = lv[l].H, Wl = lv[l].W;   // of the canvas: the launch grids and the slots
    const int Ho = Hl - WIN + 1, Wo = Wl - WIN + 1;
    const long slot = (long)Hl * Wl, mslot = (long)Ho * Wo;
    float* Xl = l ? pyrbuf + lv[l].off : nullptr;
    float* Yl = l ? Xl + (long)B * 3 * slot : nullptr;
    const ImageU8 level0{recon, d, ref, Hc, Wc, (int*)status, mslot};
    const ImagePlanes here{Xl, Yl, slot, d, Hc, Wc, l, mslot};
    const dim3 pool_grid((Wl + 255) / 256, Hl, 2 * B * 3);
    if (l == 1)
      hipLaunchKernelGGL(avgpool2_kernel<ImageU8>, pool_grid, dim3(256), 0, st, level0, B * 3, slot,
                         Xl, Yl);
    if (l > 1) {
      const long up = (long)lv[l - 1].H * lv[l - 1].W;
      const float* Xu = pyrbuf + lv[l - 1].off;
      hipLaunchKernelGGL(avgpool2_kernel<ImagePlanes>, pool_grid, dim3(256), 0, st,
                         ImagePlanes{Xu, Xu + (long)B * 3 * up, up, d, Hc, Wc, l - 1}, B * 3, slot,
                         Xl, Yl);
    }
    const dim3 grid((Wo + TOW - 1) / TOW, (Ho + TOH - 1) / TOH, B * 3);
    float* D = maps ? maps + map_off[l] : nullptr;
    float* none = nullptr;
    if (!maps && l == 0)
      hipLaunchKernelGGL((ssim_level_kernel<0, ImageU8>), grid, dim3(256), 0, st, level0, c1, c2, pl,
                         none, none, 0);
    else if (!maps)
      hipLaunchKernelGGL((ssim_level_kernel<0, ImagePlanes>), grid, dim3(256), 0, st, here, c1, c2,
                         pl, none, none, 0);
    else if (l == 0)
      hipLaunchKernelGGL((ssim_level_kernel<1, ImageU8>), grid, dim3(256), 0, st, level0, c1, c2, pl,
                         D, none, 0);
    else if (l < LEVELS - 1)
      hipLaunchKernelGGL((ssim_level_kernel<1, ImagePlanes>), grid, dim3(256), 0, st, here, c1, c2,
                         pl, D, none, 0);
    else
      hipLaunchKernelGGL((ssim_level_kernel<2, ImagePlanes>), grid, dim3(256), 0, st, here, c1, c2,
                         pl, none, D, 0);
    fin.canvas.poff[l] = pl - partial;
    fin.canvas.tiles[l] = lv[l].tiles;
    fin.canvas.count[l] = 3.0 * Ho * Wo;
    pl += 2L * B * 3 * lv[l].tiles;
  }
  hipLaunchKernelGGL(msssim_finish_kernel<ImageFinish>, dim3(B), dim3(256), 0, st, partial, fin, B,
                     means, out);
  return check_launch(what);
}

}  // namespace
}  // namespace iclr17

using namespace iclr17;

extern "C" {

size_t iclr17_ms_ssim_workspace_size(int B, int H, int W) {
  Level lv[LEVELS];
  long pyr = 0, part = 0;
  if (B <= 0 || level_plan(H, W, lv, B, &pyr, &part) != 0) return 0;
  // pyramid floats | partial doubles | per-level means [L][B][2] doubles (+ alignment slack)
  return (size_t)pyr * 4 + (size_t)part * 8 + (size_t)LEVELS * B * 2 * 8 + 256;
}

int iclr17_ms_ssim(const float* x, const float* y, int B, int H, int W, float data_range,
                   void* workspace, size_t workspace_bytes, float* out, void* stream) {
  ICLR17_REQUIRE(x && y && workspace && out && B > 0, ICLR17_EINVAL, "ms_ssim: null pointer");
  ICLR17_REQUIRE(B <= 10000 && H <= 65535 * 2, ICLR17_EINVAL, "ms_ssim: B=%d H=%d exceed the grid", B, H);
  Level lv[LEVELS];
  long pyr = 0, part = 0;
  ICLR17_REQUIRE(level_plan(H, W, lv, B, &pyr, &part) == 0, ICLR17_EINVAL,
                 "ms_ssim: %dx%d is too small for 5 levels of an 11-tap window", H, W);
  ICLR17_REQUIRE(workspace_bytes >= iclr17_ms_ssim_workspace_size(B, H, W), ICLR17_EINVAL,
                 "ms_ssim: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* pyrbuf = (float*)ws;
  double* partial = (double*)(ws + pyr * 4);
  double* means = partial + part;
  const float c1 = (0.01f * data_range) * (0.01f * data_range);
  const float c2 = (0.03f * data_range) * (0.03f * data_range);
  const float* X = x;
  const float* Y = y;
  double* pl = partial;
  FinishPlan fp;
  for (int l = 0; l < LEVELS; ++l) {
    const int Hl = lv[l].H, Wl = lv[l].W;
    if (l > 0) {
      float* Xn = pyrbuf + lv[l].off;
      float* Yn = Xn + (long)B * 3 * Hl * Wl;
      const int Hp = lv[l - 1].H, Wp = lv[l - 1].W;
      hipLaunchKernelGGL(avgpool2_kernel<Uniform>, dim3((Wl + 255) / 256, Hl, 2 * B * 3),
                         dim3(256), 0, st, Uniform{X, Y, Hp, Wp}, B * 3, (long)Hl * Wl, Xn, Yn);
      X = Xn;
      Y = Yn;
    }
    const int Ho = Hl - WIN + 1, Wo = Wl - WIN + 1;
    dim3 grid((Wo + TOW - 1) / TOW, (Ho + TOH - 1) / TOH, B * 3);
    hipLaunchKernelGGL((ssim_level_kernel<0, Uniform>), grid, dim3(256), 0, st,
                       Uniform{X, Y, Hl, Wl}, c1, c2, pl, (float*)nullptr, (float*)nullptr, 0);
    fp.poff[l] = pl - partial;
    fp.tiles[l] = lv[l].tiles;
    fp.count[l] = 3.0 * Ho * Wo;
    pl += 2L * B * 3 * lv[l].tiles;
  }
  hipLaunchKernelGGL(msssim_finish_kernel<FinishPlan>, dim3(B), dim3(256), 0, st, partial, fp, B, means, out);
  return check_launch("ms_ssim");
}

// The pyramid, the partials and the means of a canvas batch are laid out for B images of the
// canvas's size; an image uses the front of each of its slots.
size_t iclr17_image_msssim_workspace_size(int B, int Hc, int Wc) {
  return iclr17_ms_ssim_workspace_size(B, Hc, Wc);
}

int iclr17_image_msssim_u8(const float* recon, const int64_t* desc, int B, int Hc, int Wc,
                           const uint8_t* ref, void* workspace, size_t workspace_bytes, float* out,
                           int32_t* status, void* stream) {
  ICLR17_REQUIRE(recon && desc && ref && workspace && out && status, ICLR17_EINVAL,
                 "image_msssim: null pointer");
  if (int rc = check_image(B, Hc, Wc, 128)) return rc;
  ICLR17_REQUIRE(B <= 10000 && Hc <= 65535 * 2, ICLR17_EUNSUPPORTED,
                 "image_msssim: B=%d or canvas height %d beyond the launch grid", B, Hc);
  Level lv[LEVELS];
  long pyr = 0, part = 0;
  ICLR17_REQUIRE(level_plan(Hc, Wc, lv, B, &pyr, &part) == 0, ICLR17_EINVAL,
                 "image_msssim: the canvas %dx%d is too small for 5 levels of an 11-tap window", Hc,
                 Wc);
  ICLR17_REQUIRE(workspace_bytes >= iclr17_image_msssim_workspace_size(B, Hc, Wc), ICLR17_EINVAL,
                 "image_msssim: workspace too small");
  char* ws = aligned_base(workspace);
  double* partial = (double*)(ws + pyr * 4);
  return image_msssim_levels("image_msssim", recon, (const long*)desc, B, Hc, Wc,
                             (const unsigned char*)ref, lv, partial, partial + part, (float*)ws,
                             nullptr, nullptr, out, status, (hipStream_t)stream);
}

size_t iclr17_ssim_workspace_size(int B, int H, int W) {
  Level lv[1];
  long pyr = 0, part = 0;
  if (B <= 0 || level_plan(H, W, lv, B, &pyr, &part, 1) != 0) return 0;
  return (size_t)part * 8 + 256;
}

int iclr17_ssim(const float* x, const float* y, int B, int H, int W, float data_range,
                void* workspace, size_t workspace_bytes, float* out_ssim, float* out_cs,
                void* stream) {
  ICLR17_REQUIRE(x && y && workspace && out_ssim && B > 0, ICLR17_EINVAL, "ssim: null pointer");
  ICLR17_REQUIRE(B <= 10000 && H <= 65535 * 2, ICLR17_EINVAL, "ssim: B=%d H=%d exceed the grid", B, H);
  Level lv[1];
  long pyr = 0, part = 0;
  ICLR17_REQUIRE(level_plan(H, W, lv, B, &pyr, &part, 1) == 0, ICLR17_EINVAL,
                 "ssim: %dx%d is smaller than the 11-tap window", H, W);
  ICLR17_REQUIRE(workspace_bytes >= iclr17_ssim_workspace_size(B, H, W), ICLR17_EINVAL,
                 "ssim: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  double* partial = (double*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const float c1 = (0.01f * data_range) * (0.01f * data_range);
  const float c2 = (0.03f * data_range) * (0.03f * data_range);
  const int Ho = H - WIN + 1, Wo = W - WIN + 1;
  dim3 grid((Wo + TOW - 1) / TOW, (Ho + TOH - 1) / TOH, B * 3);
  hipLaunchKernelGGL((ssim_level_kernel<0, Uniform>), grid, dim3(256), 0, st, Uniform{x, y, H, W},
                     c1, c2, partial, (float*)nullptr, (float*)nullptr, 0);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(B), dim3(256), 0, st, partial, 3L * lv[0].tiles,
                     3.0 * Ho * Wo, out_ssim, out_cs);
  return check_launch("ssim");
}

// ------------------------------------------------------------------------ gradient path
size_t iclr17_ssim_grad_workspace_size(int B, int H, int W, int want_dy, int multiscale) {
  GradPlan gp;
  return grad_plan(B, H, W, want_dy, multiscale, &gp) == 0 ? gp.bytes : 0;
}

int iclr17_ms_ssim_fwd_saved(const float* x, const float* y, int B, int H, int W, float data_range,
                             int want_dy, void* workspace, size_t workspace_bytes, float* out,
                             void* stream) {
  ICLR17_REQUIRE(x && y && workspace && out && B > 0, ICLR17_EINVAL,
                 "ms_ssim_fwd_saved: null pointer");
  ICLR17_REQUIRE(B <= 10000 && H <= 65535 * 2, ICLR17_EINVAL,
                 "ms_ssim_fwd_saved: B=%d H=%d exceed the grid", B, H);
  GradPlan gp;
  ICLR17_REQUIRE(grad_plan(B, H, W, want_dy, 1, &gp) == 0, ICLR17_EINVAL,
                 "ms_ssim_fwd_saved: %dx%d is too small for 5 levels of an 11-tap window", H, W);
  ICLR17_REQUIRE(workspace_bytes >= gp.bytes, ICLR17_EINVAL,
                 "ms_ssim_fwd_saved: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = aligned_base(workspace);
  double* partial = (double*)ws;
  double* means = (double*)(ws + gp.off_means);
  float* pyrbuf = (float*)(ws + gp.off_pyr);
  float* maps = (float*)(ws + gp.off_maps);
  const float c1 = (0.01f * data_range) * (0.01f * data_range);
  const float c2 = (0.03f * data_range) * (0.03f * data_range);
  const float* X = x;
  const float* Y = y;
  double* pl = partial;
  FinishPlan fp;
  for (int l = 0; l < LEVELS; ++l) {
    const int Hl = gp.lv[l].H, Wl = gp.lv[l].W;
    if (l > 0) {
      float* Xn = pyrbuf + gp.lv[l].off;
      float* Yn = Xn + (long)B * 3 * Hl * Wl;
      hipLaunchKernelGGL(avgpool2_kernel<Uniform>, dim3((Wl + 255) / 256, Hl, 2 * B * 3),
                         dim3(256), 0, st, Uniform{X, Y, gp.lv[l - 1].H, gp.lv[l - 1].W}, B * 3,
                         (long)Hl * Wl, Xn, Yn);
      X = Xn;
      Y = Yn;
    }
    const int Ho = Hl - WIN + 1, Wo = Wl - WIN + 1;
    dim3 grid((Wo + TOW - 1) / TOW, (Ho + TOH - 1) / TOH, B * 3);
    float* d = maps + gp.maps[l];
    if (l < LEVELS - 1)
      hipLaunchKernelGGL((ssim_level_kernel<1, Uniform>), grid, dim3(256), 0, st,
                         Uniform{X, Y, Hl, Wl}, c1, c2, pl, d, (float*)nullptr, want_dy);
    else
      hipLaunchKernelGGL((ssim_level_kernel<2, Uniform>), grid, dim3(256), 0, st,
                         Uniform{X, Y, Hl, Wl}, c1, c2, pl, (float*)nullptr, d, want_dy);
    fp.poff[l] = pl - partial;
    fp.tiles[l] = gp.lv[l].tiles;
    fp.count[l] = 3.0 * Ho * Wo;
    pl += 2L * B * 3 * gp.lv[l].tiles;
  }
  hipLaunchKernelGGL(msssim_finish_kernel<FinishPlan>, dim3(B), dim3(256), 0, st, partial, fp, B, means, out);
  return check_launch("ms_ssim_fwd_saved");
}

int iclr17_ms_ssim_bwd(const float* x, const float* y, int B, int H, int W, int saved_dy,
                       void* workspace, size_t workspace_bytes, const float* g, float* dx,
                       float* dy, void* stream) {
  ICLR17_REQUIRE(x && y && workspace && g && (dx || dy) && B > 0, ICLR17_EINVAL,
                 "ms_ssim_bwd: null pointer");
  ICLR17_REQUIRE(!dy || saved_dy, ICLR17_EINVAL,
                 "ms_ssim_bwd: dy asked of a forward that saved no dY maps");
  ICLR17_REQUIRE(B <= 10000 && H <= 65535 * 2, ICLR17_EINVAL,
                 "ms_ssim_bwd: B=%d H=%d exceed the grid", B, H);
  GradPlan gp;
  ICLR17_REQUIRE(grad_plan(B, H, W, saved_dy, 1, &gp) == 0, ICLR17_EINVAL,
                 "ms_ssim_bwd: %dx%d is too small for 5 levels of an 11-tap window", H, W);
  ICLR17_REQUIRE(workspace_bytes >= gp.bytes, ICLR17_EINVAL, "ms_ssim_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = aligned_base(workspace);
  const double* means = (const double*)(ws + gp.off_means);
  const float* pyrbuf = (const float*)(ws + gp.off_pyr);
  float* gpyr = (float*)(ws + gp.off_gpyr);
  const float* maps = (const float*)(ws + gp.off_maps);
  float* coef = (float*)(ws + gp.off_coef);
  FinishPlan fp;
  for (int l = 0; l < LEVELS; ++l)
    fp.count[l] = 3.0 * (gp.lv[l].H - WIN + 1) * (gp.lv[l].W - WIN + 1);
  hipLaunchKernelGGL(msssim_coef_kernel<FinishPlan>, dim3((B + 63) / 64), dim3(64), 0, st, means,
                     g, fp, B, coef);
  for (int l = LEVELS - 1; l >= 0; --l) {
    const int Hl = gp.lv[l].H, Wl = gp.lv[l].W;
    const long n = (long)B * 3 * Hl * Wl;
    const float* X = l ? pyrbuf + gp.lv[l].off : x;
    const float* Y = l ? pyrbuf + gp.lv[l].off + n : y;
    float* oX = dx ? (l ? gpyr + gp.lv[l].off : dx) : nullptr;
    float* oY = dy ? (l ? gpyr + gp.lv[l].off + n : dy) : nullptr;
    const float *pX = nullptr, *pY = nullptr;
    long below = 0;
    if (l < LEVELS - 1) {
      below = (long)gp.lv[l + 1].H * gp.lv[l + 1].W;
      pX = dx ? gpyr + gp.lv[l + 1].off : nullptr;
      pY = dy ? gpyr + gp.lv[l + 1].off + (long)B * 3 * below : nullptr;
    }
    dim3 grid((Wl + TOW - 1) / TOW, (Hl + TOH - 1) / TOH, B * 3);
    hipLaunchKernelGGL(ssim_level_bwd_kernel<Uniform>, grid, dim3(256), 0, st,
                       Uniform{X, Y, Hl, Wl}, maps + gp.maps[l], coef + (long)l * B,
                       (const float*)nullptr, (const float*)nullptr, pX, pY, below, oX, oY);
  }
  return check_launch("ms_ssim_bwd");
}

// ------------------------------------------------- gradient path of a canvas batch
// The workspace is grad_plan's for B images of the canvas's size without dY maps; an image uses
// the front of each of its slots (partials, pyramid planes, gradient planes, maps).
size_t iclr17_image_msssim_grad_workspace_size(int B, int Hc, int Wc) {
  GradPlan gp;
  return grad_plan(B, Hc, Wc, 0, 1, &gp) == 0 ? gp.bytes : 0;
}

int iclr17_image_msssim_u8_fwd_saved(const float* recon, const int64_t* desc, int B, int Hc, int Wc,
                                     const uint8_t* ref, void* workspace, size_t workspace_bytes,
                                     float* out, int32_t* status, void* stream) {
  ICLR17_REQUIRE(recon && desc && ref && workspace && out && status, ICLR17_EINVAL,
                 "image_msssim_fwd_saved: null pointer");
  if (int rc = check_image(B, Hc, Wc, 128)) return rc;
  ICLR17_REQUIRE(B <= 10000 && Hc <= 65535 * 2, ICLR17_EUNSUPPORTED,
                 "image_msssim_fwd_saved: B=%d or canvas height %d beyond the launch grid", B, Hc);
  GradPlan gp;
  ICLR17_REQUIRE(grad_plan(B, Hc, Wc, 0, 1, &gp) == 0, ICLR17_EINVAL,
                 "image_msssim_fwd_saved: the canvas %dx%d is too small for 5 levels of an 11-tap "
                 "window", Hc, Wc);
  ICLR17_REQUIRE(workspace_bytes >= gp.bytes, ICLR17_EINVAL,
                 "image_msssim_fwd_saved: workspace too small");
  char* ws = aligned_base(workspace);
  return image_msssim_levels("image_msssim_fwd_saved", recon, (const long*)desc, B, Hc, Wc,
                             (const unsigned char*)ref, gp.lv, (double*)ws,
                             (double*)(ws + gp.off_means), (float*)(ws + gp.off_pyr),
                             (float*)(ws + gp.off_maps), gp.maps, out, status,
                             (hipStream_t)stream);
}

int iclr17_image_msssim_u8_bwd(const float* recon, const int64_t* desc, int B, int Hc, int Wc,
                               const uint8_t* ref, void* workspace, size_t workspace_bytes,
                               const float* g, float* d_recon, void* stream) {
  ICLR17_REQUIRE(recon && desc && ref && workspace && g && d_recon, ICLR17_EINVAL,
                 "image_msssim_bwd: null pointer");
  if (int rc = check_image(B, Hc, Wc, 128)) return rc;
  ICLR17_REQUIRE(B <= 10000 && Hc <= 65535 * 2, ICLR17_EUNSUPPORTED,
                 "image_msssim_bwd: B=%d or canvas height %d beyond the launch grid", B, Hc);
  GradPlan gp;
  ICLR17_REQUIRE(grad_plan(B, Hc, Wc, 0, 1, &gp) == 0, ICLR17_EINVAL,
                 "image_msssim_bwd: the canvas %dx%d is too small for 5 levels of an 11-tap window",
                 Hc, Wc);
  ICLR17_REQUIRE(workspace_bytes >= gp.bytes, ICLR17_EINVAL, "image_msssim_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = aligned_base(workspace);
  const double* means = (const double*)(ws + gp.off_means);
  const float* pyrbuf = (const float*)(ws + gp.off_pyr);
  float* gpyr = (float*)(ws + gp.off_gpyr);
  const float* maps = (const float*)(ws + gp.off_maps);
  float* coef = (float*)(ws + gp.off_coef);
  const long* d = (const long*)desc;
  hipLaunchKernelGGL(msssim_coef_kernel<ImageFinish>, dim3((B + 63) / 64), dim3(64), 0, st, means,
                     g, ImageFinish{{}, d, Hc, Wc}, B, coef);
  for (int l = LEVELS - 1; l >= 0; --l) {
    const int Hl = gp.lv[l].H, Wl = gp.lv[l].W;   // of the canvas: the launch grid and the slots
    const long slot = (long)Hl * Wl, mslot = (long)(Hl - WIN + 1) * (Wl - WIN + 1);
    const float* pX = nullptr;
    long below = 0;
    if (l < LEVELS - 1) {
      below = (long)gp.lv[l + 1].H * gp.lv[l + 1].W;
      pX = gpyr + gp.lv[l + 1].off;
    }
    const float* D = maps + gp.maps[l];
    const float* c = coef + (long)l * B;
    const dim3 grid((Wl + TOW - 1) / TOW, (Hl + TOH - 1) / TOH, B * 3);
    if (l == 0) {
      hipLaunchKernelGGL(ssim_level_bwd_kernel<ImageU8>, grid, dim3(256), 0, st,
                         ImageU8{recon, d, (const unsigned char*)ref, Hc, Wc, nullptr, mslot}, D, c,
                         (const float*)nullptr, (const float*)nullptr, pX, (const float*)nullptr,
                         below, d_recon, (float*)nullptr);
    } else {
      const float* Xl = pyrbuf + gp.lv[l].off;
      hipLaunchKernelGGL(ssim_level_bwd_kernel<ImagePlanes>, grid, dim3(256), 0, st,
                         ImagePlanes{Xl, Xl + (long)B * 3 * slot, slot, d, Hc, Wc, l, mslot}, D, c,
                         (const float*)nullptr, (const float*)nullptr, pX, (const float*)nullptr,
                         below, gpyr + gp.lv[l].off, (float*)nullptr);
    }
  }
  return check_launch("image_msssim_bwd");
}

int iclr17_ssim_fwd_saved(const float* x, const float* y, int B, int H, int W, float data_range,
                          int want_dy, void* workspace, size_t workspace_bytes, float* out_ssim,
                          float* out_cs, void* stream) {
  ICLR17_REQUIRE(x && y && workspace && out_ssim && out_cs && B > 0, ICLR17_EINVAL,
                 "ssim_fwd_saved: null pointer");
  ICLR17_REQUIRE(B <= 10000 && H <= 65535 * 2, ICLR17_EINVAL,
                 "ssim_fwd_saved: B=%d H=%d exceed the grid", B, H);
  GradPlan gp;
  ICLR17_REQUIRE(grad_plan(B, H, W, want_dy, 0, &gp) == 0, ICLR17_EINVAL,
                 "ssim_fwd_saved: %dx%d is smaller than the 11-tap window", H, W);
  ICLR17_REQUIRE(workspace_bytes >= gp.bytes, ICLR17_EINVAL, "ssim_fwd_saved: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = aligned_base(workspace);
  double* partial = (double*)ws;
  float* maps = (float*)(ws + gp.off_maps);
  const float c1 = (0.01f * data_range) * (0.01f * data_range);
  const float c2 = (0.03f * data_range) * (0.03f * data_range);
  const int Ho = H - WIN + 1, Wo = W - WIN + 1;
  const long set = (long)gp.nmaps * B * 3 * Ho * Wo;
  dim3 grid((Wo + TOW - 1) / TOW, (Ho + TOH - 1) / TOH, B * 3);
  hipLaunchKernelGGL((ssim_level_kernel<3, Uniform>), grid, dim3(256), 0, st, Uniform{x, y, H, W},
                     c1, c2, partial, maps + set, maps, want_dy);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(B), dim3(256), 0, st, partial, 3L * gp.lv[0].tiles,
                     3.0 * Ho * Wo, out_ssim, out_cs);
  return check_launch("ssim_fwd_saved");
}

int iclr17_ssim_bwd(const float* x, const float* y, int B, int H, int W, int saved_dy,
                    void* workspace, size_t workspace_bytes, const float* g_ssim,
                    const float* g_cs, float* dx, float* dy, void* stream) {
  ICLR17_REQUIRE(x && y && workspace && (g_ssim || g_cs) && (dx || dy) && B > 0, ICLR17_EINVAL,
                 "ssim_bwd: null pointer");
  ICLR17_REQUIRE(!dy || saved_dy, ICLR17_EINVAL,
                 "ssim_bwd: dy asked of a forward that saved no dY maps");
  ICLR17_REQUIRE(B <= 10000 && H <= 65535 * 2, ICLR17_EINVAL,
                 "ssim_bwd: B=%d H=%d exceed the grid", B, H);
  GradPlan gp;
  ICLR17_REQUIRE(grad_plan(B, H, W, saved_dy, 0, &gp) == 0, ICLR17_EINVAL,
                 "ssim_bwd: %dx%d is smaller than the 11-tap window", H, W);
  ICLR17_REQUIRE(workspace_bytes >= gp.bytes, ICLR17_EINVAL, "ssim_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = aligned_base(workspace);
  const float* maps = (const float*)(ws + gp.off_maps);
  float* coef = (float*)(ws + gp.off_coef);
  const int Ho = H - WIN + 1, Wo = W - WIN + 1;
  const long set = (long)gp.nmaps * B * 3 * Ho * Wo;
  hipLaunchKernelGGL(ssim_coef_kernel, dim3((B + 63) / 64), dim3(64), 0, st, g_ssim, g_cs,
                     3.0 * Ho * Wo, B, coef);
  // set A: the ssim maps when g_ssim is given, else the cs maps; set B: the cs maps when both are
  const float* DA = g_ssim ? maps : maps + set;
  const float* cA = g_ssim ? coef : coef + B;
  const float* DB = g_ssim && g_cs ? maps + set : nullptr;
  dim3 grid((W + TOW - 1) / TOW, (H + TOH - 1) / TOH, B * 3);
  hipLaunchKernelGGL(ssim_level_bwd_kernel<Uniform>, grid, dim3(256), 0, st, Uniform{x, y, H, W},
                     DA, cA, DB, (const float*)(coef + B), (const float*)nullptr,
                     (const float*)nullptr, 0L, dx, dy);
  return check_launch("ssim_bwd");
}

}  // extern "C"
