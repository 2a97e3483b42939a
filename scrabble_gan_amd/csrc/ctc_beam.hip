// CTC prefix beam search with an optional dense character n-gram LM: the third way to read the recognizer, between the best
// path (k_ctc_greedy) and the closed-lexicon read (k_ctc_score_words).  Contract: include/scrabble_hip.h, sg_ctc_beam_decode.
//
// One workgroup of 256 threads per sample, the whole search in LDS.  A beam entry is a prefix (a byte row, labels < 64) with
// pb / pnb (log-mass of its alignments ending in blank / non-blank), acc (LM + length credit), its length, its last two labels
// and two 64-bit rolling hashes (of the prefix and of the prefix without its last label).  Two generations of the beam are
// kept; a frame reads one and writes the other.  Per frame, n = live entries (<= beam), candidate k = i * C + c is "entry i
// extended by c" for c < C-1 and "entry i stays" for c = C-1:
//   A  merge   n^2 (j, i) pairs: is entry i the prefix of entry j without j's last label?  (length, hash, then the bytes.)  Then
//              the extension (i, last(j)) IS the string of entry j: its mass goes into j's stay candidate and the candidate is
//              struck (bit last(j) of kill[i]).  Identity is string equality, never "same parent slot".
//   B  stay    per entry: tot = lse(pb, pnb), the stay candidate's pb' = tot + lp[blank] and pnb' = pnb + lp[last] (+) merged mass
//   C  keys    every thread scores its 16 candidates into registers: (order-preserving bits of the score) << 32 | ~k, so that a
//              plain unsigned maximum takes the higher score and, on a tie, the lower k; 0 = no candidate
//   D  cut     up to `beam` rounds of workgroup maximum (wave shuffles, then 4 values through LDS, one barrier per round); the
//              winner's owner clears that key and rescans its 16
//   E  build   one wavefront per new entry: the lanes copy the parent's row as 32-bit words (a row has at most 64 of them), the
//              lane that owns the appended position patches the new label in; lane 0 writes the scalars
// Frame row t + 1 is fetched into a register at the top of frame t and parked in LDS at its end; every row is read from memory
// once.  A (+) has at most two terms (a string is reached by staying and by ONE extension: l + c = l' + c' forces l = l'), and
// lse2 is symmetric, so there is no summation order to fix; no float atomics anywhere (the one LDS atomic is an integer OR).
#include "ctc_common.h"

#define BM_THREADS 256
#define BM_MAX_BEAM 64
#define BM_MAX_C 64
#define BM_MAX_T 256
#define BM_KEYS (BM_MAX_BEAM * BM_MAX_C / BM_THREADS)      // candidates per thread
#define BM_HASH_MUL 0x9E3779B97F4A7C15ull

typedef unsigned long long bm_u64;

struct BmBeam {                      // one generation, structure of arrays
  float pb[BM_MAX_BEAM], pnb[BM_MAX_BEAM], acc[BM_MAX_BEAM];
  int len[BM_MAX_BEAM];
  int last[BM_MAX_BEAM], last2[BM_MAX_BEAM];       // the final two labels; C-1 (the blank, which is no label) where the prefix is shorter
  bm_u64 hash[BM_MAX_BEAM], phash[BM_MAX_BEAM];    // of the prefix / of the prefix without its last label
};

// floats -> unsigned ints of the same order (-inf lowest, still above 0)
__device__ __forceinline__ unsigned bm_ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ bm_u64 bm_key(float score, int k) { return ((bm_u64)bm_ord(score) << 32) | (bm_u64)(0xFFFFFFFFu - (unsigned)k); }

__device__ __forceinline__ bm_u64 bm_wave_max(bm_u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64), lo = __shfl_xor((unsigned)v, o, 64);
    const bm_u64 u = ((bm_u64)hi << 32) | lo;
    v = u > v ? u : v;
  }
  return v;
}

// pnb contribution of "entry (last, pb, tot) extended by c": a repeated label needs a blank in between
__device__ __forceinline__ float bm_ext(float lpc, int c, int last, float pb, float tot) { return lpc + (c == last ? pb : tot); }

// len_bonus + lm_weight * lm[ctx, c]; ctx = the last order-1 labels, oldest first, base C, C-1 at a missing position
__device__ __forceinline__ float bm_credit(const float* lm, int lm_order, float lm_weight, float len_bonus, int C, int last, int last2, int c) {
  if (!lm) return len_bonus;
  const int ctx = lm_order == 1 ? 0 : (lm_order == 2 ? last : last2 * C + last);
  return len_bonus + lm_weight * lm[(size_t)ctx * C + c];
}

__global__ __launch_bounds__(BM_THREADS) void k_ctc_beam(const float* lp_all, const float* lm, int* out_labels, int* out_len,
                                                         float* out_score, int T, int C, int L, int W, int lm_order, float lm_weight,
                                                         float len_bonus, int nbest, int out_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bm_rows[];       // [2][W][Lp] prefixes
  __shared__ BmBeam st[2];
  __shared__ float row[2][BM_MAX_C];                                            // lp[t], lp[t+1]
  __shared__ float tot[BM_MAX_BEAM], spb[BM_MAX_BEAM], spnb[BM_MAX_BEAM];       // per entry: lse(pb, pnb); the stay candidate's pb', pnb'
  __shared__ int par[BM_MAX_BEAM];                                              // slot of the entry's prefix-without-last, or -1
  __shared__ bm_u64 kill[BM_MAX_BEAM];                                          // bit c: extension (entry, c) merged into an entry
  __shared__ bm_u64 wbest[2][BM_THREADS / 64];
  __shared__ int sel[BM_MAX_BEAM];
  __shared__ float fscore[BM_MAX_BEAM];
  __shared__ int src[BM_MAX_BEAM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blank = C - 1;
  const int Lp = (L + 3) & ~3;                                                  // row stride: whole 32-bit words
  const float* lp = lp_all + (size_t)blockIdx.x * T * C;

  if (tid < BM_MAX_BEAM) {
    par[tid] = -1;
    kill[tid] = 0ull;
  }
  if (tid == 0) {
    st[0].pb[0] = 0.f; st[0].pnb[0] = -INFINITY; st[0].acc[0] = 0.f;
    st[0].len[0] = 0; st[0].last[0] = blank; st[0].last2[0] = blank;
    st[0].hash[0] = 0ull; st[0].phash[0] = 0ull;
  }
  if (tid < C) row[0][tid] = lp[tid];
  __syncthreads();

  int n = 1, cur = 0;
  for (int t = 0; t < L; ++t) {
    const BmBeam& S = st[cur];
    BmBeam& N = st[cur ^ 1];
    const unsigned char* pre = bm_rows + (size_t)cur * W * Lp;
    unsigned char* nxt = bm_rows + (size_t)(cur ^ 1) * W * Lp;
    const float* r = row[t & 1];
    float ahead = 0.f;
    if (t + 1 < L && tid < C) ahead = lp[(size_t)(t + 1) * C + tid];            // lands while the frame is worked on

    // A: which extension is already an entry
    for (int p = tid; p < n * n; p += BM_THREADS) {
      const int j = p / n, i = p - j * n;
      const int li = S.len[i];
      if (li + 1 != S.len[j] || S.hash[i] != S.phash[j]) continue;
      const unsigned* a = reinterpret_cast<const unsigned*>(pre + (size_t)i * Lp);
      const unsigned* b = reinterpret_cast<const unsigned*>(pre + (size_t)j * Lp);
      bool same = true;
      for (int w = 0; w < (li >> 2); ++w) same = same && a[w] == b[w];
      for (int q = li & ~3; q < li; ++q) same = same && pre[(size_t)i * Lp + q] == pre[(size_t)j * Lp + q];
      if (same) {
        par[j] = i;                                                             // (strings are unique: one i per j)
        atomicOr(&kill[i], 1ull << S.last[j]);
      }
    }
    __syncthreads();

    // B: the stay candidates
    if (tid < n) {
      const float tt = dec_lse2(S.pb[tid], S.pnb[tid]);
      float s = S.len[tid] > 0 ? S.pnb[tid] + r[S.last[tid]] : -INFINITY;
      const int i = par[tid];
      if (i >= 0) {
        const int c = S.last[tid];
        s = dec_lse2(s, bm_ext(r[c], c, S.last[i], S.pb[i], dec_lse2(S.pb[i], S.pnb[i])));
      }
      tot[tid] = tt;
      spb[tid] = tt + r[blank];
      spnb[tid] = s;
    }
    __syncthreads();

    // C: keys
    bm_u64 key[BM_KEYS];
    bm_u64 best = 0ull;
    const int ncand = n * C;
#pragma unroll
    for (int q = 0; q < BM_KEYS; ++q) {
      const int k = tid + BM_THREADS * q;
      bm_u64 kk = 0ull;
      if (k < ncand) {
        const int i = k / C, c = k - i * C;
        if (c == blank) {
          kk = bm_key(dec_lse2(spb[i], spnb[i]) + S.acc[i], k);
        } else if (!((kill[i] >> c) & 1ull)) {
          const float pnb = bm_ext(r[c], c, S.last[i], S.pb[i], tot[i]);
          kk = bm_key(pnb + (S.acc[i] + bm_credit(lm, lm_order, lm_weight, len_bonus, C, S.last[i], S.last2[i], c)), k);
        }
      }
      key[q] = kk;
      best = kk > best ? kk : best;
    }

    // D: the cut
    const int rounds = min(W, ncand);
    int nn = 0;
    for (int rd = 0; rd < rounds; ++rd) {
      const bm_u64 v = bm_wave_max(best);
      if (lane == 0) wbest[rd & 1][wave] = v;
      __syncthreads();
      bm_u64 g = wbest[rd & 1][0];
#pragma unroll
      for (int w = 1; w < BM_THREADS / 64; ++w) g = wbest[rd & 1][w] > g ? wbest[rd & 1][w] : g;
      if (g == 0ull) break;                                                     // (the same g in every thread)
      if (tid == 0) sel[rd] = (int)(0xFFFFFFFFu - (unsigned)g);
      nn = rd + 1;
      if (best == g) {                                                          // keys are unique: the owner alone
        best = 0ull;
#pragma unroll
        for (int q = 0; q < BM_KEYS; ++q) {
          if (key[q] == g) key[q] = 0ull;
          best = key[q] > best ? key[q] : best;
        }
      }
    }
    __syncthreads();

    // E: the next generation
    for (int e = wave; e < nn; e += BM_THREADS / 64) {                          // wave-uniform
      const int k = sel[e];
      const int i = k / C, c = k - i * C;
      const int li = S.len[i];                                                  // li <= t, so li + 1 <= L <= Lp
      const unsigned* from = reinterpret_cast<const unsigned*>(pre + (size_t)i * Lp);
      unsigned* to = reinterpret_cast<unsigned*>(nxt + (size_t)e * Lp);
      if (lane < ((li + 4) >> 2)) {                                             // the words that hold bytes [0, li]: at most Lp / 4 <= 64
        unsigned w = from[lane];
        if (c != blank && lane == (li >> 2)) {
          const int sh = (li & 3) * 8;
          w = (w & ~(0xFFu << sh)) | ((unsigned)c << sh);
        }
        to[lane] = w;
      }
      if (lane == 0) {
        if (c == blank) {
          N.pb[e] = spb[i]; N.pnb[e] = spnb[i]; N.acc[e] = S.acc[i];
          N.len[e] = li; N.last[e] = S.last[i]; N.last2[e] = S.last2[i];
          N.hash[e] = S.hash[i]; N.phash[e] = S.phash[i];
        } else {
          N.pb[e] = -INFINITY;
          N.pnb[e] = bm_ext(r[c], c, S.last[i], S.pb[i], tot[i]);
          N.acc[e] = S.acc[i] + bm_credit(lm, lm_order, lm_weight, len_bonus, C, S.last[i], S.last2[i], c);
          N.len[e] = li + 1; N.last[e] = c; N.last2[e] = S.last[i];
          N.hash[e] = (S.hash[i] + (bm_u64)(c + 1)) * BM_HASH_MUL; N.phash[e] = S.hash[i];
        }
      }
    }
    if (tid < BM_MAX_BEAM) {
      par[tid] = -1;
      kill[tid] = 0ull;
    }
    if (t + 1 < L && tid < C) row[(t + 1) & 1][tid] = ahead;
    __syncthreads();
    n = nn;
    cur ^= 1;
  }

  // survivors, best first by the final score (+ end-of-word term); slots past them: length 0, -inf
  const BmBeam& S = st[cur];
  const unsigned char* pre = bm_rows + (size_t)cur * W * Lp;
  if (tid < n) {
    float s = dec_lse2(S.pb[tid], S.pnb[tid]) + S.acc[tid];
    if (lm) {
      const int ctx = lm_order == 1 ? 0 : (lm_order == 2 ? S.last[tid] : S.last2[tid] * C + S.last[tid]);
      s += lm_weight * lm[(size_t)ctx * C + blank];
    }
    fscore[tid] = s;
  }
  __syncthreads();
  const size_t o0 = (size_t)blockIdx.x * nbest;
  if (tid < n) {
    const unsigned mine = bm_ord(fscore[tid]);
    int rank = 0;
    for (int q = 0; q < n; ++q) {
      const unsigned u = bm_ord(fscore[q]);
      rank += (u > mine || (u == mine && q < tid)) ? 1 : 0;                     // a strict order: the ranks are a permutation of [0, n)
    }
    src[rank] = tid;
    if (rank < nbest) {
      out_len[o0 + rank] = S.len[tid];
      out_score[o0 + rank] = fscore[tid];
    }
  } else if (tid < nbest) {
    out_len[o0 + tid] = 0;
    out_score[o0 + tid] = -INFINITY;
  }
  __syncthreads();
  for (int e = wave; e < nbest; e += BM_THREADS / 64) {
    const int s = e < n ? src[e] : 0;
    const int len = e < n ? S.len[s] : 0;
    int* out = out_labels + (o0 + e) * out_stride;
    for (int pos = lane; pos < out_stride; pos += 64) out[pos] = pos < len ? (int)pre[(size_t)s * Lp + pos] : -1;
  }
}

extern "C" long sg_ctc_beam_workspace_bytes(int B, int input_length, int beam) {
  if (B < 1 || input_length < 1 || input_length > BM_MAX_T || beam < 1 || beam > BM_MAX_BEAM) return -1;
  return 0;                                   // the search lives in LDS
}

extern "C" int sg_ctc_beam_decode(const float* lp, int B, int T, int C, int input_length, int beam, const float* lm, int lm_order,
                                  float lm_weight, float len_bonus, int* out_labels, int* out_len, float* out_score, int nbest,
                                  int out_stride, void* workspace, void* stream) {
  (void)workspace;
  if (!lp || !out_labels || !out_len || !out_score || B < 1 || C < 2 || C > BM_MAX_C || beam < 1 || beam > BM_MAX_BEAM || nbest < 1 ||
      nbest > beam || input_length < 1 || input_length > T || out_stride < input_length || (lm && (lm_order < 1 || lm_order > 3)))
    return SG_ERR_ARG;
  if (input_length > BM_MAX_T) return SG_ERR_UNSUPPORTED;
  const size_t lds = (size_t)2 * beam * ((input_length + 3) & ~3);              // <= 32 KiB beside ~9 KiB of static state
  SG_KERNEL(k_ctc_beam, dim3(B), dim3(BM_THREADS), lds, (hipStream_t)stream, lp, lm, out_labels, out_len, out_score, T, C, input_length,
            beam, lm_order, lm_weight, len_bonus, nbest, out_stride);
  return sg_launch_status();
}
