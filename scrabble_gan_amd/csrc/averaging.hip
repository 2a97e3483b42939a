// Averaged generator: the exponential moving average of a network's flat parameter buffer, the in-place exchange that
// puts the average under the model's parameter views (and takes it out again), and the uint8 sample sheet.
// All three are HBM-bound sweeps: 16 bytes per lane, grid capped by sg_grid_for with a grid-stride loop, as k_adam.
//   ema update : 12 B of HBM traffic per weight (read ema, read p, write ema)
//   swap       : 16 B per weight
//   sheet      : 4 B read per image pixel, 1 B written per sheet pixel
#include "sg_common.h"

#define F4(p) (*reinterpret_cast<float4*>(p))
#define CF4(p) (*reinterpret_cast<const float4*>(p))

static inline bool sg_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ema += a (p - ema), a = 1 - decay rounded once on the host.  COPY: a == 1, where ema + (p - ema) is not p in floating point
template <bool COPY>
__global__ __launch_bounds__(256) void k_ema(float* ema, const float* p, long n, float a) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += stride) {
    const float4 pv = CF4(p + 4 * e);
    if (COPY) {
      F4(ema + 4 * e) = pv;
    } else {
      float4 ev = CF4(ema + 4 * e);
      ev.x += a * (pv.x - ev.x); ev.y += a * (pv.y - ev.y);
      ev.z += a * (pv.z - ev.z); ev.w += a * (pv.w - ev.w);
      F4(ema + 4 * e) = ev;
    }
  }
  for (long e = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const float pv = p[e];
    ema[e] = COPY ? pv : ema[e] + a * (pv - ema[e]);
  }
}

extern "C" int sg_ema_update(float* ema, const float* p, long n, float one_minus_decay, void* stream) {
  if (n < 0 || !sg_aligned16(ema) || !sg_aligned16(p)) return SG_ERR_ARG;
  if (!(one_minus_decay >= 0.f && one_minus_decay <= 1.f)) return SG_ERR_ARG;      // (also rejects NaN)
  if (n == 0) return SG_OK;                                                         // (an empty buffer may have no address)
  if (!ema || !p) return SG_ERR_ARG;
  if (one_minus_decay == 0.f) return SG_OK;                                         // nothing moves: ema stays bitwise what it was
  const dim3 grid(sg_grid_for((n + 3) / 4, 256));
  if (one_minus_decay == 1.f)
    SG_KERNEL(k_ema<true>, grid, dim3(256), 0, (hipStream_t)stream, ema, p, n, 1.f);
  else
    SG_KERNEL(k_ema<false>, grid, dim3(256), 0, (hipStream_t)stream, ema, p, n, one_minus_decay);
  return sg_launch_status();
}

__global__ __launch_bounds__(256) void k_swap(float* a, float* b, long n) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += stride) {
    const float4 av = CF4(a + 4 * e), bv = CF4(b + 4 * e);
    F4(a + 4 * e) = bv; F4(b + 4 * e) = av;
  }
  for (long e = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const float av = a[e];
    a[e] = b[e]; b[e] = av;
  }
}

// a <-> b, n floats each.  The buffers must be the same one (nothing to do) or disjoint: every element is read and written by ONE lane
extern "C" int sg_swap_f32(float* a, float* b, long n, void* stream) {
  if (n < 0 || !sg_aligned16(a) || !sg_aligned16(b)) return SG_ERR_ARG;
  if (n == 0) return SG_OK;
  if (!a || !b) return SG_ERR_ARG;
  if (a == b) return SG_OK;
  const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
  if ((ua < ub ? ub - ua : ua - ub) < (uintptr_t)n * sizeof(float)) return SG_ERR_ARG;
  SG_KERNEL(k_swap, dim3(sg_grid_for((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, a, b, n);
  return sg_launch_status();
}

// One sheet byte: the image pixel under it as round(clip((x + 1) / 2, 0, 1) * 255) -- the float32 numpy expression of
// run_inference.generate / save_grid, same operations in the same order, nothing contracted, round-half-even -- or `fill` in a
// gutter / an unused cell of the last row.
__device__ __forceinline__ unsigned sheet_byte(const float* imgs, int o, int N, int H, int W, int cols, int pad, int SW, unsigned fill) {
#pragma clang fp contract(off)
  const int sy = o / SW, sx = o - sy * SW;
  const int r = sy / (H + pad), y = sy - r * (H + pad);
  const int c = sx / (W + pad), x = sx - c * (W + pad);
  const int i = r * cols + c;
  if (y >= H || x >= W || i >= N) return fill;
  float v = (imgs[(i * H + y) * W + x] + 1.0f) / 2.0f;
  v = fminf(fmaxf(v, 0.0f), 1.0f);
  return (unsigned)rintf(v * 255.0f);
}

// four consecutive sheet bytes per lane, one 32-bit store; the last, partial group is written byte by byte
__global__ __launch_bounds__(256) void k_image_sheet(const float* __restrict__ imgs, unsigned char* __restrict__ sheet, int total, int N, int H,
                                                     int W, int cols, int pad, int SW, unsigned fill) {
  const int groups = (total >> 2) + ((total & 3) ? 1 : 0);
  for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {   // (grid * block <= 2^20: no overflow)
    const int o = 4 * g;
    if (total - o >= 4) {
      unsigned w = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) w |= sheet_byte(imgs, o + k, N, H, W, cols, pad, SW, fill) << (8 * k);
      *reinterpret_cast<unsigned*>(sheet + o) = w;
    } else {
      for (int k = o; k < total; ++k) sheet[k] = (unsigned char)sheet_byte(imgs, k, N, H, W, cols, pad, SW, fill);
    }
  }
}

// imgs [N,H,W,1] fp32 in [-1,1] -> sheet uint8 [rows*(H+pad)-pad, cols*(W+pad)-pad], rows = ceil(N/cols), image i at (i / cols, i % cols)
extern "C" int sg_image_sheet_u8(const float* imgs, unsigned char* sheet, int N, int H, int W, int cols, int pad, int fill, void* stream) {
  if (!imgs || !sheet || N < 1 || H < 1 || W < 1 || cols < 1 || pad < 0 || fill < 0 || fill > 255) return SG_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(sheet) & 3) return SG_ERR_ARG;
  const long rows = ((long)N + cols - 1) / cols;
  const long SH = rows * ((long)H + pad) - pad, SW = (long)cols * ((long)W + pad) - pad;
  if (SH > 0x7fffffffL || SW > 0x7fffffffL || SH * SW > 0x7fffffffL) return SG_ERR_ARG;   // the kernel indexes with 32-bit integers
  const int total = (int)(SH * SW);
  SG_KERNEL(k_image_sheet, dim3(sg_grid_for((SH * SW + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, imgs, sheet, total, N, H, W, cols, pad,
            (int)SW, (unsigned)fill);
  return sg_launch_status();
}
