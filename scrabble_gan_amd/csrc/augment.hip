// Differentiable augmentation of the discriminator's inputs (DiffAugment, Zhao et al. 2020; scrabble_gan_amd/augment.py draws the
// parameter rows): per sample a contrast / brightness map about the sample's mean, a bilinear affine resampling with constant
// padding, and a rectangular cutout -- forward and exact adjoint.  Not in the reference.
//
//   params [B,12] : c beta | a00 a01 a02 a10 a11 a12 | x0 y0 x1 y1
//   mu_b          = mean of x_b over H W C (fp64 accumulation)
//   t(v)          = c v + (1 - c) mu_b + beta
//   y[b,i,j,:]    = pad                                              inside the half-open cutout rectangle
//                 = sum over the four taps around (sx, sy) of w * (tap inside ? t(x[tap]) : pad)   elsewhere,
//   sx = a00 j + a01 i + a02, sy = a10 j + a11 i + a12; a tap of weight exactly 0 is skipped and not read.
//
// Both kernels are HBM sweeps of one read and one write per element: a workgroup stages its sample (at most 32 x 368 floats =
// 46 KiB in the shapes this project trains on) in LDS, takes the mean (forward) or the mean's gradient (backward) from there and
// then resamples from LDS, so the 4 (forward) or 9 (backward) reads per element never leave the CU.  A sample that does not fit
// (> AUG_STAGE_MAX floats) is read from global memory twice instead (the second time from L2).
//
// Backward = a GATHER, one adder per dx address, so dx is bitwise reproducible in every mode: input pixel (x, y) visits the
// output pixels (i, j) whose sample point lies within one pixel of it and re-derives their tap weights with the forward pass's
// own expressions (aug_coord / aug_axis: the same roundings, hence the same weights, and the same "skip w == 0" rule).
// Search window, from the limits augment.DiffAugment.check enforces (a10 == 0, 0.9 <= a00, a11 <= 1.1, |a01| <= 0.3,
// |a02|, |a12| <= 2^16):
//   rows   : sy = a11 i + a12 and |sy - y| < 1  =>  |i - i*| < 1 / a11 <= 1.112 with i* = (y - a12) / a11.  The kernel takes
//            ic = rint(i* computed in fp32): |ic - i*| <= 0.5 + err, err < 2^-24 (2^16 + H) / 0.9 + 2^-24 |i*| < 0.01, so
//            |i - ic| < 1.63 and i, ic being integers |i - ic| <= 1: THREE candidate rows ic - 1 .. ic + 1.
//   columns: for each candidate row i, sx = a00 j + (a01 i + a02) and |sx - x| < 1  =>  |j - j*| < 1 / a00 <= 1.112 with
//            j* = (x - a02 - a01 i) / a00; the same argument gives THREE candidate columns jc - 1 .. jc + 1.
// The window only has to be a superset: every candidate is tested with the forward expressions before it contributes.
//
// Addressing: every index is formed from a value that was range-tested first (aug_axis returns index 0 with ok = false for a tap
// outside the image; candidates outside [0,H) x [0,W) are dropped before dy is addressed).  The sample base is b * HWC in 64-bit;
// inside a sample 32-bit indices suffice because the entry points reject H W C > 2^31 - 1.
#include "sg_common.h"

#define AUG_THREADS 512
#define AUG_RED_BYTES 128                                    // 8 wave partials (fp64) in front of the staged sample: keeps it 16-byte aligned
#define AUG_STAGE_MAX ((65536 - AUG_RED_BYTES) / 4)          // floats of one sample that fit the 64 KiB a workgroup gets without opting in

struct AugRow {
  float c, beta, a00, a01, a02, a10, a11, a12, cx0, cy0, cx1, cy1;
};

__device__ __forceinline__ AugRow aug_row(const float* __restrict__ params, long b) {
  const float* p = params + b * 12;
  AugRow r;
  r.c = p[0]; r.beta = p[1];
  r.a00 = p[2]; r.a01 = p[3]; r.a02 = p[4]; r.a10 = p[5]; r.a11 = p[6]; r.a12 = p[7];
  r.cx0 = p[8]; r.cy0 = p[9]; r.cx1 = p[10]; r.cy1 = p[11];
  return r;
}

// the sample point of output pixel (row i, column j): two fused multiply-adds per coordinate, exact for integer translations
__device__ __forceinline__ void aug_coord(const AugRow& r, int i, int j, float& sx, float& sy) {
  sx = fmaf(r.a00, (float)j, fmaf(r.a01, (float)i, r.a02));
  sy = fmaf(r.a10, (float)j, fmaf(r.a11, (float)i, r.a12));
}

__device__ __forceinline__ bool aug_cut(const AugRow& r, int i, int j) {
  return (float)j >= r.cx0 && (float)j < r.cx1 && (float)i >= r.cy0 && (float)i < r.cy1;
}

// the two taps of one axis of length n around coordinate s: weights, and for each tap whether it lies inside and, if so, its index
// (0 otherwise: the index is in range whatever s is, NaN and +-huge included)
__device__ __forceinline__ void aug_axis(float s, int n, int& i0, int& i1, bool& ok0, bool& ok1, float& w0, float& w1) {
  const float f = floorf(s);
  w1 = s - f;
  w0 = 1.f - w1;
  ok0 = f >= 0.f && f <= (float)(n - 1);
  ok1 = f >= -1.f && f <= (float)(n - 2);
  i0 = ok0 ? (int)f : 0;
  i1 = ok1 ? (int)f + 1 : 0;
}

// sum of `v` over the workgroup in fp64, the same value in every thread; fixed order (lane butterflies, then waves 0..n-1)
__device__ __forceinline__ double aug_block_sum(double v, double* red) {
  v = sg_wave_sum_d(v);
  __syncthreads();                                           // (red may still be read from the previous use)
  if ((threadIdx.x & (SG_WAVE - 1)) == 0) red[threadIdx.x / SG_WAVE] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < AUG_THREADS / SG_WAVE; ++w) s += red[w];
  return s;
}

// global sample -> LDS (STAGE) with its fp64 sum, or the sum alone.  16 bytes per lane where the sample's base allows it
template <bool STAGE>
__device__ __forceinline__ double aug_load(const float* __restrict__ g, float* lds, int n, bool vec) {
  double acc = 0.0;
  if (vec) {
    for (int q = threadIdx.x; q < (n >> 2); q += AUG_THREADS) {
      const float4 v = *reinterpret_cast<const float4*>(g + 4 * q);
      if (STAGE) *reinterpret_cast<float4*>(lds + 4 * q) = v;
      acc += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
  } else {
    for (int e = threadIdx.x; e < n; e += AUG_THREADS) {
      const float v = g[e];
      if (STAGE) lds[e] = v;
      acc += (double)v;
    }
  }
  return acc;
}

template <bool STAGE>
__global__ __launch_bounds__(AUG_THREADS) void k_augment_fwd(const float* __restrict__ x, const float* __restrict__ params, float* __restrict__ y,
                                                             float* __restrict__ mean_out, int B, int H, int W, int C, float pad, bool vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char aug_smem[];
  double* red = reinterpret_cast<double*>(aug_smem);
  float* lds = reinterpret_cast<float*>(aug_smem + AUG_RED_BYTES);
  const int n = H * W * C;
  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    const float* xb = x + b * n;
    float* yb = y + b * n;
    const AugRow r = aug_row(params, b);
    __syncthreads();                                         // (the previous sample's readers are done with lds)
    const double sum = aug_block_sum(aug_load<STAGE>(xb, lds, n, vec), red);      // (its barriers also publish lds)
    const double mu = sum / (double)n;
    if (threadIdx.x == 0) mean_out[b] = (float)mu;
    const float off = (float)((double)(1.f - r.c) * mu + (double)r.beta);         // t(v) = c v + off
    const float* src = STAGE ? lds : xb;
    for (int e = threadIdx.x; e < n; e += AUG_THREADS) {
      const int pix = e / C, ch = e - pix * C;
      const int i = pix / W, j = pix - i * W;
      float out = pad;
      if (!aug_cut(r, i, j)) {
        float sx, sy, wx[2], wy[2];
        int ix[2], iy[2];
        bool okx[2], oky[2];
        aug_coord(r, i, j, sx, sy);
        aug_axis(sx, W, ix[0], ix[1], okx[0], okx[1], wx[0], wx[1]);
        aug_axis(sy, H, iy[0], iy[1], oky[0], oky[1], wy[0], wy[1]);
        out = 0.f;
#pragma unroll
        for (int ty = 0; ty < 2; ++ty)
#pragma unroll
          for (int tx = 0; tx < 2; ++tx) {
            const float w = wx[tx] * wy[ty];
            if (w != 0.f) {
              const bool in = okx[tx] && oky[ty];
              const float v = in ? fmaf(r.c, src[(iy[ty] * W + ix[tx]) * C + ch], off) : pad;
              out = fmaf(w, v, out);
            }
          }
      }
      yb[e] = out;
    }
  }
}

template <bool STAGE>
__global__ __launch_bounds__(AUG_THREADS) void k_augment_bwd(const float* __restrict__ dy, const float* __restrict__ params, float* __restrict__ dx,
                                                             int B, int H, int W, int C, bool vec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char aug_smem[];
  double* red = reinterpret_cast<double*>(aug_smem);
  float* lds = reinterpret_cast<float*>(aug_smem + AUG_RED_BYTES);
  const int n = H * W * C;
  for (long b = blockIdx.x; b < B; b += gridDim.x) {
    const float* gb = dy + b * n;
    float* dxb = dx + b * n;
    const AugRow r = aug_row(params, b);
    __syncthreads();
    if (STAGE) {
      aug_load<true>(gb, lds, n, vec);
      __syncthreads();
    }
    const float* src = STAGE ? lds : gb;

    // gradient of the mean: (1 - c) * sum over non-cut output pixels of dy * (weight of their inside taps), spread over the sample
    float gm = 0.f;
    if (r.c != 1.f) {                                        // (block-uniform: one row per sample)
      double acc = 0.0;
      for (int e = threadIdx.x; e < n; e += AUG_THREADS) {
        const int pix = e / C;
        const int i = pix / W, j = pix - i * W;
        if (aug_cut(r, i, j)) continue;
        float sx, sy, wx[2], wy[2];
        int ix[2], iy[2];
        bool okx[2], oky[2];
        aug_coord(r, i, j, sx, sy);
        aug_axis(sx, W, ix[0], ix[1], okx[0], okx[1], wx[0], wx[1]);
        aug_axis(sy, H, iy[0], iy[1], oky[0], oky[1], wy[0], wy[1]);
        float win = 0.f;
#pragma unroll
        for (int ty = 0; ty < 2; ++ty)
#pragma unroll
          for (int tx = 0; tx < 2; ++tx) {
            const float w = wx[tx] * wy[ty];
            if (w != 0.f && okx[tx] && oky[ty]) win += w;
          }
        acc += (double)(win * src[e]);
      }
      gm = (float)((double)(1.f - r.c) * aug_block_sum(acc, red) / (double)n);
    }

    for (int e = threadIdx.x; e < n; e += AUG_THREADS) {
      const int pix = e / C, ch = e - pix * C;
      const int yy = pix / W, xx = pix - yy * W;
      // centre row of the window (header comment); clamped BEFORE the conversion, so ic is in [-2, H + 1] whatever the row holds
      const int ic = (int)rintf(fminf(fmaxf(((float)yy - r.a12) / r.a11, -2.f), (float)H + 1.f));
      float s = 0.f;
      for (int i = ic - 1; i <= ic + 1; ++i) {
        if (i < 0 || i >= H) continue;
        const float jr = ((float)xx - fmaf(r.a01, (float)i, r.a02)) / r.a00;
        const int jc = (int)rintf(fminf(fmaxf(jr, -2.f), (float)W + 1.f));
        for (int j = jc - 1; j <= jc + 1; ++j) {
          if (j < 0 || j >= W) continue;
          if (aug_cut(r, i, j)) continue;
          float sx, sy, wx0, wx1, wy0, wy1;
          int ix0, ix1, iy0, iy1;
          bool okx0, okx1, oky0, oky1;
          aug_coord(r, i, j, sx, sy);
          aug_axis(sx, W, ix0, ix1, okx0, okx1, wx0, wx1);
          aug_axis(sy, H, iy0, iy1, oky0, oky1, wy0, wy1);
          // which of (i, j)'s taps, if any, is this input pixel
          const float wxe = (okx0 && ix0 == xx) ? wx0 : ((okx1 && ix1 == xx) ? wx1 : 0.f);
          const float wye = (oky0 && iy0 == yy) ? wy0 : ((oky1 && iy1 == yy) ? wy1 : 0.f);
          const float w = wxe * wye;
          if (w != 0.f) s = fmaf(w, src[(i * W + j) * C + ch], s);
        }
      }
      dxb[e] = fmaf(r.c, s, gm);
    }
  }
}

static inline bool aug_args_ok(const void* a, const void* p, const void* o, int B, int H, int W, int C) {
  if (!a || !p || !o || a == o || B < 1 || H < 1 || W < 1 || C < 1) return false;
  if (H > (1 << 24) || W > (1 << 24)) return false;                               // (float)(n - 1) in aug_axis is exact
  return (long)H * W * C <= 0x7fffffffL;                                            // 32-bit indices inside one sample
}

// x, y [B,H,W,C] fp32 (distinct buffers), params [B,12], mean_out [B]
extern "C" int sg_augment_fwd(const float* x, const float* params, float* y, float* mean_out, int B, int H, int W, int C, float pad, void* stream) {
  if (!aug_args_ok(x, params, y, B, H, W, C) || !mean_out) return SG_ERR_ARG;
  const long n = (long)H * W * C;
  const bool stage = n <= AUG_STAGE_MAX;
  const bool vec = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const size_t lds = AUG_RED_BYTES + (stage ? (size_t)((n + 3) / 4) * 16 : 0);
  const dim3 grid(B < sg_grid_cap() ? B : sg_grid_cap());
  if (stage)
    SG_KERNEL(k_augment_fwd<true>, grid, dim3(AUG_THREADS), lds, (hipStream_t)stream, x, params, y, mean_out, B, H, W, C, pad, vec);
  else
    SG_KERNEL(k_augment_fwd<false>, grid, dim3(AUG_THREADS), lds, (hipStream_t)stream, x, params, y, mean_out, B, H, W, C, pad, vec);
  return sg_launch_status();
}

// dy, dx [B,H,W,C] fp32 (distinct buffers); dx is overwritten
extern "C" int sg_augment_bwd(const float* dy, const float* params, float* dx, int B, int H, int W, int C, void* stream) {
  if (!aug_args_ok(dy, params, dx, B, H, W, C)) return SG_ERR_ARG;
  const long n = (long)H * W * C;
  const bool stage = n <= AUG_STAGE_MAX;
  const bool vec = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0;
  const size_t lds = AUG_RED_BYTES + (stage ? (size_t)((n + 3) / 4) * 16 : 0);
  const dim3 grid(B < sg_grid_cap() ? B : sg_grid_cap());
  if (stage)
    SG_KERNEL(k_augment_bwd<true>, grid, dim3(AUG_THREADS), lds, (hipStream_t)stream, dy, params, dx, B, H, W, C, vec);
  else
    SG_KERNEL(k_augment_bwd<false>, grid, dim3(AUG_THREADS), lds, (hipStream_t)stream, dy, params, dx, B, H, W, C, vec);
  return sg_launch_status();
}
