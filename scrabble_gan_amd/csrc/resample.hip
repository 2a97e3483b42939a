// Resampling of a ragged batch of grey uint8 images in one launch (the converter of scrabble_gan_amd/dinterface.py, the raw-corpus
// reader and the style-image loader of data_io.py; the reference resizes with cv2.resize on the host, iam_handwriting_db.py:73,
// data_utils.py:144,179).  desc [n_img, 8] long, one row per image:
//   src_off sh sw src_stride | dst_off dh dw canvas_w
// Output row r of an image starts at dst_off + r * canvas_w; columns < min(dw, canvas_w) are the resampled image, columns in
// [dw, canvas_w) are `fill`, columns >= canvas_w of a wider resample are never computed (the crop of data_utils.py:147-148).
//
// Sampling (per axis, s source and d output pixels; the contract is tests/resample_refs.py).  Tap positions and weights are formed
// from INTEGER quotients and remainders, the weight is one fp64 quotient of two exact integers rounded to fp32 once:
//   LINEAR  x = ((2i+1) s - d) / (2d) = q + r / (2d);  taps q, q+1 (clamped to [0, s-1]), weights (2d - r) / 2d and r / 2d
//   CUBIC   the same q, r; taps q-1 .. q+2 (clamped), Keys weights with A = -0.75 evaluated in fp64 at f = r / 2d
//   AREA, both axes shrink or keep (sh >= dh and sw >= dw): exact box integration.  In units of 1/d of a source pixel output i
//           covers [i s, (i+1) s) and source pixel t covers [t d, (t+1) d): weight = overlap / s (interior taps: d / s)
//   AREA, either axis grows: both axes take two taps sx = floor(i s / d), sx + 1 with fx = ((i+1) s - (sx+1) d) / s reduced to its
//           fractional part (0 when not positive, and sx = s-1, fx = 0 at the end): weights (s - r) / s and r / s
// Products and sums are fp32 fused multiply-adds in ascending tap order, rows first and then columns: one fixed order, so a result
// does not depend on the grid, on how a source is cut into passes, or on the other images of the batch.
//
// Layout.  A workgroup owns a tile of RS_RB output rows x RS_CB output columns of one image (grid.x walks the images, grid.y the
// tiles of an image; the descriptors live on the device, so the grid cannot depend on them).  It builds the tile's row and column
// tap tables once (LDS), then for every RS_CW-wide slice of the source columns its columns need:
//   vertical pass   each thread takes 16 source columns of one output row: one aligned 16-byte load per tap row (what the 16-byte
//                   rule for src_off / src_stride is for), 16 fp32 accumulators, the finished fp32 row segment goes to LDS;
//   horizontal pass each thread takes output pixels of the tile and adds its taps that fall into the slice from LDS to the
//                   pixel's accumulator (LDS as well: the same thread owns a pixel in every slice).
// A source of any height is streamed by the vertical pass (an output row reads only its own tap rows), a source wider than RS_CW
// by the slices; 46 KiB of LDS whatever the shape.  The bytes between sw and src_stride are loaded with their 16-byte group but no
// tap index reaches them (every index is clamped to [0, sw-1] before it addresses the staged row).
//
// Addressing: a descriptor row outside the documented ranges (1 <= sh, sw <= 32768, 1 <= dh, dw, canvas_w <= 4096, stride >= sw,
// offsets >= 0) is skipped by its workgroups; the buffers' extents are the caller's contract (ops.resample_u8 checks them on the host).
#include "sg_common.h"

#define RS_THREADS 256
#define RS_RB 8                     // output rows of a tile
#define RS_CB 256                   // output columns of a tile
#define RS_CW 1024                  // source columns staged per pass (a multiple of 16)
#define RS_LINEAR 0
#define RS_AREA 1
#define RS_CUBIC 2
#define RS_OUT_U8 0
#define RS_OUT_F32 1
#define RS_OUT_F32_QUANT 2

struct RsTap {                      // taps t0 .. t0 + n - 1 of one output index; box: w = {first, interior, last}, else w[k] of tap k
  int t0, n;
  float w[4];
};

__device__ __forceinline__ double rs_keys_near(double x) { return ((-0.75 + 2.0) * x - (-0.75 + 3.0)) * x * x + 1.0; }                  // |x| <= 1
__device__ __forceinline__ double rs_keys_far(double x) { return ((-0.75 * x - 5.0 * -0.75) * x + 8.0 * -0.75) * x - 4.0 * -0.75; }      // 1 < |x| < 2

__device__ RsTap rs_tap(int mode, bool two_tap_area, long i, long s, long d) {
  RsTap t;
  t.w[0] = t.w[1] = t.w[2] = t.w[3] = 0.f;
  if (mode == RS_AREA && !two_tap_area) {
    const long lo = i * s, hi = (i + 1) * s;
    const long first = lo / d, last = (hi + d - 1) / d - 1;
    const long ov0 = (hi < (first + 1) * d ? hi : (first + 1) * d) - lo;
    const long ov1 = hi - (lo > last * d ? lo : last * d);
    t.t0 = (int)first;
    t.n = (int)(last - first + 1);
    t.w[0] = (float)((double)ov0 / (double)s);
    t.w[1] = (float)((double)d / (double)s);
    t.w[2] = (float)((double)ov1 / (double)s);
  } else if (mode == RS_AREA) {
    long sx = (i * s) / d;
    long r = 0;
    if (sx >= s - 1) {
      sx = s - 1;
    } else {
      const long num = (i + 1) * s - (sx + 1) * d;
      r = num <= 0 ? 0 : num % s;
    }
    t.t0 = (int)sx;
    t.n = 2;
    t.w[0] = (float)((double)(s - r) / (double)s);
    t.w[1] = (float)((double)r / (double)s);
  } else {
    const long num = (2 * i + 1) * s - d, den = 2 * d;
    long q = num / den;
    if (num < 0 && q * den != num) --q;                      // floor
    const long r = num - q * den;
    if (mode == RS_LINEAR) {
      t.t0 = (int)q;
      t.n = 2;
      t.w[0] = (float)((double)(den - r) / (double)den);
      t.w[1] = (float)((double)r / (double)den);
    } else {
      const double f = (double)r / (double)den;
      t.t0 = (int)q - 1;
      t.n = 4;
      t.w[0] = (float)rs_keys_far(1.0 + f);
      t.w[1] = (float)rs_keys_near(f);
      t.w[2] = (float)rs_keys_near(1.0 - f);
      t.w[3] = (float)rs_keys_far(2.0 - f);
    }
  }
  return t;
}

__device__ __forceinline__ float rs_weight(const RsTap* t, int k, int n, bool box) {
  if (!box) return t->w[k];
  return k == 0 ? t->w[0] : (k == n - 1 ? t->w[2] : t->w[1]);
}

__device__ __forceinline__ int rs_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

template <int OUT>
__device__ __forceinline__ void rs_store(void* out, long at, float v) {
  if (OUT == RS_OUT_F32) {
    reinterpret_cast<float*>(out)[at] = (v - 127.5f) / 127.5f;
    return;
  }
  const float q = rintf(fminf(fmaxf(v, 0.f), 255.f));        // saturate, round half to even
  if (OUT == RS_OUT_U8)
    reinterpret_cast<unsigned char*>(out)[at] = (unsigned char)q;
  else
    reinterpret_cast<float*>(out)[at] = (q - 127.5f) / 127.5f;                   // sg_normalize_u8's two operations
}

template <int OUT>
__global__ __launch_bounds__(RS_THREADS) void k_resample_u8(const unsigned char* __restrict__ src, const long* __restrict__ desc, int n_img,
                                                            int mode, void* __restrict__ out, float fill) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
  float* stage = reinterpret_cast<float*>(rs_smem);                              // [RS_RB][RS_CW]
  float* acc = stage + RS_RB * RS_CW;                                            // [rows of the tile][computed columns of the tile]
  RsTap* ctap = reinterpret_cast<RsTap*>(acc + RS_RB * RS_CB);                   // [RS_CB]
  RsTap* rtap = ctap + RS_CB;                                                    // [RS_RB]
  const int tid = threadIdx.x;

  for (int img = blockIdx.x; img < n_img; img += gridDim.x) {
    const long* dr = desc + 8L * img;
    const long src_off = dr[0], sh_l = dr[1], sw_l = dr[2], stride = dr[3], dst_off = dr[4], dh_l = dr[5], dw_l = dr[6], cw_l = dr[7];
    if (src_off < 0 || dst_off < 0 || sh_l < 1 || sw_l < 1 || sh_l > 32768 || sw_l > 32768 || stride < sw_l || (stride & 15) || (src_off & 15) ||
        dh_l < 1 || dw_l < 1 || cw_l < 1 || dh_l > 4096 || dw_l > 4096 || cw_l > 4096)
      continue;                                              // (block-uniform)
    const int sh = (int)sh_l, sw = (int)sw_l, dh = (int)dh_l, dw = (int)dw_l, cw = (int)cw_l;
    const bool two_tap_area = mode == RS_AREA && (sh < dh || sw < dw);
    const bool box = mode == RS_AREA && !two_tap_area;
    const int ncomp = dw < cw ? dw : cw;
    const int nct = (cw + RS_CB - 1) / RS_CB;
    const int ntiles = ((dh + RS_RB - 1) / RS_RB) * nct;
    const unsigned char* simg = src + src_off;

    for (int tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
      const int r0 = (tile / nct) * RS_RB, c0 = (tile % nct) * RS_CB;
      const int nr = dh - r0 < RS_RB ? dh - r0 : RS_RB;
      const int nc = cw - c0 < RS_CB ? cw - c0 : RS_CB;
      const int ncc = ncomp - c0 < 0 ? 0 : (ncomp - c0 < nc ? ncomp - c0 : nc);  // columns of the tile that are resampled, the rest is fill
      __syncthreads();                                       // (the previous tile's readers are done with the tables and acc)
      if (tid < nr) rtap[tid] = rs_tap(mode, two_tap_area, r0 + tid, sh, dh);
      for (int j = tid; j < ncc; j += RS_THREADS) ctap[j] = rs_tap(mode, two_tap_area, c0 + j, sw, dw);
      for (int e = tid; e < nr * ncc; e += RS_THREADS) acc[e] = 0.f;
      __syncthreads();

      if (ncc > 0) {
        const int xlo = rs_clamp(ctap[0].t0, sw - 1);
        const int xhi = rs_clamp(ctap[ncc - 1].t0 + ctap[ncc - 1].n - 1, sw - 1);
        for (int x0 = xlo & ~15; x0 <= xhi; x0 += RS_CW) {
          const int x1 = x0 + RS_CW < xhi + 1 ? x0 + RS_CW : xhi + 1;            // source columns [x0, x1) in this pass
          const int ng = (x1 - x0 + 15) >> 4;

          // vertical pass: 16 source columns of one output row per thread
          for (int e = tid; e < nr * ng; e += RS_THREADS) {
            const int r = e / ng, g = e - r * ng;
            const RsTap* rt = rtap + r;
            const int t0 = rt->t0, n = rt->n;
            const unsigned char* p = simg + x0 + 16 * g;
            float a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = 0.f;
#pragma unroll 2
            for (int k = 0; k < n; ++k) {
              const int y = rs_clamp(t0 + k, sh - 1);
              const float w = rs_weight(rt, k, n, box);
              const uint4 v = *reinterpret_cast<const uint4*>(p + (long)y * stride);
              const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                a[4 * q + 0] = fmaf(w, (float)(u[q] & 0xffu), a[4 * q + 0]);
                a[4 * q + 1] = fmaf(w, (float)((u[q] >> 8) & 0xffu), a[4 * q + 1]);
                a[4 * q + 2] = fmaf(w, (float)((u[q] >> 16) & 0xffu), a[4 * q + 2]);
                a[4 * q + 3] = fmaf(w, (float)(u[q] >> 24), a[4 * q + 3]);
              }
            }
            float4* so = reinterpret_cast<float4*>(stage + r * RS_CW + 16 * g);
#pragma unroll
            for (int q = 0; q < 4; ++q) so[q] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
          }
          __syncthreads();

          // horizontal pass: the taps of every output pixel that fall into [x0, x1), in ascending order
          for (int e = tid; e < nr * ncc; e += RS_THREADS) {
            const int r = e / ncc, j = e - r * ncc;
            const RsTap* ct = ctap + j;
            const int t0 = ct->t0, n = ct->n;
            int k0 = 0, k1 = n;
            if (box) {                                       // (box taps are never clamped: index = t0 + k)
              k0 = x0 - t0 > 0 ? x0 - t0 : 0;
              k1 = x1 - t0 < n ? x1 - t0 : n;
            }
            const float* srow = stage + r * RS_CW - x0;
            float s = acc[e];
            for (int k = k0; k < k1; ++k) {
              const int x = rs_clamp(t0 + k, sw - 1);
              if (x >= x0 && x < x1) s = fmaf(rs_weight(ct, k, n, box), srow[x], s);
            }
            acc[e] = s;
          }
          __syncthreads();                                   // (stage is rewritten by the next pass; acc is read by other threads below)
        }
      }

      for (int e = tid; e < nr * nc; e += RS_THREADS) {
        const int r = e / nc, j = e - r * nc;
        const float v = j < ncc ? acc[r * ncc + j] : fill;
        rs_store<OUT>(out, dst_off + (long)(r0 + r) * cw + c0 + j, v);
      }
    }
  }
}

// src: packed grey images (device, 16-byte aligned); desc [n_img, 8] long (device); out: uint8 (OUT_U8) or fp32; fill 0..255
extern "C" int sg_resample_u8(const unsigned char* src, const long* desc, int n_img, int mode, int out_kind, void* out, int fill, void* stream) {
  if (n_img < 0 || mode < RS_LINEAR || mode > RS_CUBIC || out_kind < RS_OUT_U8 || out_kind > RS_OUT_F32_QUANT || fill < 0 || fill > 255)
    return SG_ERR_ARG;
  if (n_img == 0) return SG_OK;
  if (!src || !desc || !out) return SG_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(src) & 15) || (reinterpret_cast<uintptr_t>(desc) & 7) || (reinterpret_cast<uintptr_t>(out) & 3)) return SG_ERR_ARG;
  const size_t lds = (size_t)RS_RB * RS_CW * 4 + (size_t)RS_RB * RS_CB * 4 + (size_t)(RS_CB + RS_RB) * sizeof(RsTap);
  int gy = 1024 / n_img;                                     // tiles of one image taken side by side: 4 cover a 32-row word image
  gy = gy < 4 ? 4 : (gy > 64 ? 64 : gy);
  const dim3 grid(n_img < sg_grid_cap() ? n_img : sg_grid_cap(), gy);
  const float f = (float)fill;
  if (out_kind == RS_OUT_U8)
    SG_KERNEL(k_resample_u8<RS_OUT_U8>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, src, desc, n_img, mode, out, f);
  else if (out_kind == RS_OUT_F32)
    SG_KERNEL(k_resample_u8<RS_OUT_F32>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, src, desc, n_img, mode, out, f);
  else
    SG_KERNEL(k_resample_u8<RS_OUT_F32_QUANT>, grid, dim3(RS_THREADS), lds, (hipStream_t)stream, src, desc, n_img, mode, out, f);
  return sg_launch_status();
}
