// Fidelity statistics of feature rows (scrabble_gan_amd/fidelity.py): streaming fp64 first / second moments for the Frechet
// distance and the polynomial-kernel Gram sums of the kernel distance (KID), both on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64).  The operands are fp32 features; they stay fp32 in LDS and are widened on the read into the
// fragment.  A product of two fp32 values is exact in fp64, so the only rounding is the order of the additions -- and that
// order is fixed: no floating-point atomics, one workgroup per output tile, partial sums added in index order.
//
// One 256-thread workgroup owns a 64x64 tile C = P Q^T; wave w owns the 32x32 quadrant (w >> 1, w & 1) as 2x2 MFMA tiles.
// Fragment maps of the f64 instruction (NOT those of the f32 forms): A[lane & 15][k = lane >> 4], B[k = lane >> 4][lane & 15],
// C/D col = lane & 15, row = (lane >> 4) + 4 * reg.
#include "sg_common.h"

typedef double fd_d4 __attribute__((ext_vector_type(4)));

#define FD_TILE 64
#define FD_KT 16     // contraction steps per LDS stage (4 MFMA k-steps)
#define FD_LD 80     // floats between two k-rows of a staged operand: the four k-groups of a fragment read fall 16 banks apart
#define FD_MAX_D 4096

// ---- operand loaders: element [r][k] of a 64-row operand, zero outside the matrix.  load() takes this thread's 4 elements of
// the stage that starts at contraction index k0 into registers, store() puts them into the stage buffer s[k][FD_LD].
// Contraction over the ROWS of x (moments): [r][k] = x[k, c0 + r], coalesced along r
struct FdLoadCols {
  const float* x;
  long ld;
  int c0, ncols, nrows;
  __device__ __forceinline__ void load(float (&v)[4], int k0) const {
    const int r = threadIdx.x & 63, c = c0 + r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + (threadIdx.x >> 6) + 4 * j;
      v[j] = (c < ncols && k < nrows) ? x[(long)k * ld + c] : 0.f;
    }
  }
  __device__ __forceinline__ void store(float* s, const float (&v)[4]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[((threadIdx.x >> 6) + 4 * j) * FD_LD + (threadIdx.x & 63)] = v[j];
  }
};
// Contraction over the COLUMNS of gathered rows (kernel sums): [r][k] = x[rows[r], k], coalesced along k; rows[r] < 0: masked
struct FdLoadRows {
  const float* x;
  long ld;
  const int* rows;      // LDS, 64 entries
  int ncols;
  __device__ __forceinline__ void load(float (&v)[4], int k0) const {
    const int k = k0 + (threadIdx.x & 15);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rows[(threadIdx.x >> 4) + 16 * j];
      v[j] = (row >= 0 && k < ncols) ? x[(long)row * ld + k] : 0.f;
    }
  }
  __device__ __forceinline__ void store(float* s, const float (&v)[4]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[(threadIdx.x & 15) * FD_LD + (threadIdx.x >> 4) + 16 * j] = v[j];
  }
};

// acc (this wave's 2x2 MFMA tiles of the 64x64 tile) += P Q^T over K contraction steps.  The next stage's global loads are in
// flight while the matrix cores work on the current one.
template <class LP, class LQ>
__device__ __forceinline__ void fd_tile_product(const LP& lp, const LQ& lq, int K, float* sP, float* sQ, fd_d4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, wr = (threadIdx.x >> 6) >> 1, wc = (threadIdx.x >> 6) & 1;
  const int kq = lane >> 4, e = lane & 15;
  float rp[4], rq[4];
  lp.load(rp, 0);
  lq.load(rq, 0);
  for (int k0 = 0; k0 < K; k0 += FD_KT) {
    __syncthreads();                       // the previous stage has been read
    lp.store(sP, rp);
    lq.store(sQ, rq);
    __syncthreads();
    if (k0 + FD_KT < K) {
      lp.load(rp, k0 + FD_KT);
      lq.load(rq, k0 + FD_KT);
    }
#pragma unroll
    for (int kk = 0; kk < FD_KT; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = (double)sP[(kk + kq) * FD_LD + 32 * wr + 16 * i + e];
        b[i] = (double)sQ[(kk + kq) * FD_LD + 32 * wc + 16 * i + e];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
  }
}

// index b of the upper triangle of a T x T tile grid (row-major, ti <= tj) -> (ti, tj)
__device__ __forceinline__ void fd_upper_pair(int b, int T, int& ti, int& tj) {
  ti = 0;
  while (b >= T - ti) {
    b -= T - ti;
    ++ti;
  }
  tj = ti + b;
}

// ---- moments ------------------------------------------------------------------------------------------------------------
// sum[a] += sum_i x[i, a]: one lane per column, rows in order
__global__ __launch_bounds__(256) void k_feature_sum(const float* __restrict__ x, long ldx, int n, int D, double* __restrict__ sum) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= D) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += (double)x[(long)i * ldx + a];
  sum[a] += s;
}

// outer += x^T x: one workgroup per tile pair (ti <= tj); it adds into its tile and stores the same values into the mirrored
// tile, so outer stays bitwise symmetric.  On a diagonal tile the lanes of the upper triangle do both stores.
__global__ __launch_bounds__(256) void k_feature_outer(const float* __restrict__ x, long ldx, int n, int D, double* __restrict__ outer) {
  __shared__ float sP[FD_KT * FD_LD], sQ[FD_KT * FD_LD];
  int ti, tj;
  fd_upper_pair(blockIdx.x, (D + FD_TILE - 1) / FD_TILE, ti, tj);
  fd_d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = fd_d4{0.0, 0.0, 0.0, 0.0};
  const FdLoadCols lp{x, ldx, FD_TILE * ti, D, n}, lq{x, ldx, FD_TILE * tj, D, n};
  fd_tile_product(lp, lq, n, sP, sQ, acc);
  const int lane = threadIdx.x & 63, wr = (threadIdx.x >> 6) >> 1, wc = (threadIdx.x >> 6) & 1;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int a = FD_TILE * ti + 32 * wr + 16 * mi + (lane >> 4) + 4 * reg;
        const int b = FD_TILE * tj + 32 * wc + 16 * ni + (lane & 15);
        if (a < D && b < D && a <= b) {
          const double v = outer[(long)a * D + b] + acc[mi][ni][reg];
          outer[(long)a * D + b] = v;
          if (a != b) outer[(long)b * D + a] = v;
        }
      }
}

extern "C" int sg_feature_moments(const float* x, long ldx, int n, int D, double* sum, double* outer, void* stream) {
  if (!x || !sum || !outer || n < 1 || D < 1 || D > FD_MAX_D || ldx < D) return SG_ERR_ARG;
  const int T = (D + FD_TILE - 1) / FD_TILE;
  SG_KERNEL(k_feature_sum, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, ldx, n, D, sum);
  SG_KERNEL(k_feature_outer, dim3(T * (T + 1) / 2), dim3(256), 0, (hipStream_t)stream, x, ldx, n, D, outer);
  return sg_launch_status();
}

// mean = sum / count ; cov = (outer - count mean mean^T) / (count - 1)
__global__ __launch_bounds__(256) void k_feature_cov(const double* __restrict__ sum, const double* __restrict__ outer, double count,
                                                     double* __restrict__ mean, double* __restrict__ cov, int D) {
  const long total = (long)D * D;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const int a = (int)(e / D), b = (int)(e - (long)a * D);
    const double ma = sum[a] / count, mb = sum[b] / count;
    cov[e] = (outer[e] - count * ma * mb) / (count - 1.0);
    if (a == 0) mean[b] = mb;
  }
}

extern "C" int sg_feature_cov(const double* sum, const double* outer, double count, double* mean, double* cov, int D, void* stream) {
  if (!sum || !outer || !mean || !cov || D < 1 || D > FD_MAX_D || !(count >= 2.0)) return SG_ERR_ARG;
  SG_KERNEL(k_feature_cov, dim3(sg_grid_for((long)D * D, 256)), dim3(256), 0, (hipStream_t)stream, sum, outer, count, mean, cov, D);
  return sg_launch_status();
}

// ---- polynomial-kernel Gram sums ------------------------------------------------------------------------------------------
// tiles of one subset: [0, P) XX upper triangle, [P, 2P) YY upper triangle, [2P, 2P + Tm^2) XY; P = Tm (Tm + 1) / 2
static inline long fd_mmd_tiles(int m) {
  const long Tm = (m + FD_TILE - 1) / FD_TILE;
  return Tm * (Tm + 1) + Tm * Tm;
}

extern "C" long sg_poly_mmd_workspace_doubles(int S, int m) {
  if (S < 1 || m < 1) return -1;
  return (long)S * fd_mmd_tiles(m);
}

// workspace[blockIdx.x] = this tile's sum of k(P_i, Q_j) = (gamma P_i . Q_j + coef0)^3 over the valid (i, j); XX / YY tiles above the
// diagonal count twice (their mirror is not computed), tiles on it skip i == j
__global__ __launch_bounds__(256) void k_poly_mmd_tiles(const float* __restrict__ x, long ldx, const float* __restrict__ y, long ldy,
                                                        const int* __restrict__ ix, const int* __restrict__ iy, int m, int D, double gamma,
                                                        double coef0, int Tm, int NT, double* __restrict__ workspace) {
  __shared__ float sP[FD_KT * FD_LD], sQ[FD_KT * FD_LD];
  __shared__ int rowsP[FD_TILE], rowsQ[FD_TILE];
  __shared__ double red[4];
  const int s = blockIdx.x / NT, P = Tm * (Tm + 1) / 2;
  int t = blockIdx.x - s * NT, kind, ti, tj;
  if (t < 2 * P) {
    kind = t < P ? 0 : 1;
    fd_upper_pair(t - kind * P, Tm, ti, tj);
  } else {
    kind = 2;
    t -= 2 * P;
    ti = t / Tm;
    tj = t - ti * Tm;
  }
  const float* pp = kind == 1 ? y : x;
  const float* pq = kind == 0 ? x : y;
  const long ldp = kind == 1 ? ldy : ldx, ldq = kind == 0 ? ldx : ldy;
  const int* ip = kind == 1 ? iy : ix;
  const int* iq = kind == 0 ? ix : iy;
  if (threadIdx.x < FD_TILE) {
    const int i = FD_TILE * ti + threadIdx.x;
    rowsP[threadIdx.x] = i < m ? (ip ? ip[(long)s * m + i] : i) : -1;
  } else if (threadIdx.x < 2 * FD_TILE) {
    const int j = FD_TILE * tj + threadIdx.x - FD_TILE;
    rowsQ[threadIdx.x - FD_TILE] = j < m ? (iq ? iq[(long)s * m + j] : j) : -1;
  }
  __syncthreads();
  fd_d4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = fd_d4{0.0, 0.0, 0.0, 0.0};
  const FdLoadRows lp{pp, ldp, rowsP, D}, lq{pq, ldq, rowsQ, D};
  fd_tile_product(lp, lq, D, sP, sQ, acc);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1;
  const bool diag = kind < 2 && ti == tj;
  double part = 0.0;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = FD_TILE * ti + 32 * wr + 16 * mi + (lane >> 4) + 4 * reg;
        const int j = FD_TILE * tj + 32 * wc + 16 * ni + (lane & 15);
        if (i < m && j < m && !(diag && i == j)) {
          const double k = gamma * acc[mi][ni][reg] + coef0;
          part += k * k * k;
        }
      }
  part = sg_wave_sum_d(part);
  if (lane == 0) red[w] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double tot = ((red[0] + red[1]) + red[2]) + red[3];
    workspace[blockIdx.x] = (kind < 2 && ti < tj) ? 2.0 * tot : tot;
  }
}

// sums[s, kind] = the partial sums of (s, kind) added in index order
__global__ __launch_bounds__(64) void k_poly_mmd_reduce(const double* __restrict__ workspace, int S, int Tm, int NT, double* __restrict__ sums) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= 3 * S) return;
  const int s = e / 3, kind = e - 3 * s, P = Tm * (Tm + 1) / 2;
  const int lo = kind * P, hi = kind == 2 ? NT : lo + P;
  double tot = 0.0;
  for (int t = lo; t < hi; ++t) tot += workspace[(long)s * NT + t];
  sums[e] = tot;
}

extern "C" int sg_poly_mmd_sums(const float* x, long ldx, const float* y, long ldy, const int* ix, const int* iy, int S, int m, int D,
                                double gamma, double coef0, double* workspace, double* sums, void* stream) {
  if (!x || !y || !workspace || !sums || S < 1 || m < 1 || D < 1 || D > FD_MAX_D || ldx < D || ldy < D) return SG_ERR_ARG;
  const long NT = fd_mmd_tiles(m);
  if (NT > 0x7fffffffL || (long)S * NT > 0x7fffffffL) return SG_ERR_ARG;        // one workgroup per tile, 32-bit tile indices
  const int Tm = (m + FD_TILE - 1) / FD_TILE;
  SG_KERNEL(k_poly_mmd_tiles, dim3((unsigned)(S * NT)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, ix, iy, m, D, gamma, coef0, Tm,
            (int)NT, workspace);
  SG_KERNEL(k_poly_mmd_reduce, dim3((3 * S + 63) / 64), dim3(64), 0, (hipStream_t)stream, workspace, S, Tm, (int)NT, sums);
  return sg_launch_status();
}
