// Reading the recognizer: what ctc.hip trains, these kernels decode and score.
//   k_ctc_log_probs     per-frame lp = log_softmax(log(softmax(logits) + 1e-7)) -- phase A of k_softmax_ctc, written out
//   k_ctc_greedy        best-path decoding: per-frame argmax, merge equal neighbours, drop blanks
//   k_ctc_score_words   CTC negative log-likelihood of W candidate words (mixed lengths) per sample: the alpha recursion of
//                       k_softmax_ctc on the precomputed lp, one wavefront per (sample, word)
//   k_edit_distance     Levenshtein distance, one DP row across the lanes
//   k_legibility_sums   fp64 {sum dist, sum ref_len, #(dist != 0), B}
// Blank = last class.  Wave-shaped like ctc.hip: lanes are classes (C <= 64), frames (64 per chunk), extended-label states
// (2 len + 1 <= 64) or reference positions (ref_len <= 63); neighbours come from __shfl, flags from __ballot.
#include "ctc_common.h"      // dec_lse2 / dec_lse3

// One frame, lanes = classes; `a` is the lane's logit (-inf for lane >= C).  The same operations in the same order as phase A
// of k_softmax_ctc, so a score computed from this lp equals the training loss of the same word.
__device__ __forceinline__ float dec_frame_lp(float a, int lane, int C) {
  const float mx = sg_wave_max(a);
  const float e = lane < C ? expf(a - mx) : 0.f;
  const float p = e / sg_wave_sum(e);
  const float yv = lane < C ? logf(p + 1e-7f) : -INFINITY;
  const float my = sg_wave_max(yv);
  const float ey = lane < C ? expf(yv - my) : 0.f;
  const float ls = my + logf(sg_wave_sum(ey));
  return yv - ls;
}

// one wavefront per frame row, 4 rows per workgroup
__global__ __launch_bounds__(256) void k_ctc_log_probs(const float* logits, float* lp, long rows, int C) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {      // wave-uniform
    const float a = lane < C ? logits[r * C + lane] : -INFINITY;
    const float v = dec_frame_lp(a, lane, C);
    if (lane < C) lp[r * C + lane] = v;
  }
}

// One wavefront per sample.  Per frame the lanes are classes (argmax, lp of the winner); per chunk of 64 frames the lanes are
// frames: lane t & 63 keeps frame t's winner, keep-flags go through __ballot and a kept symbol lands at
// count + popcount(flags of the lower lanes).  `carry` (the previous chunk's last winner) and `count` cross the chunks.
__global__ __launch_bounds__(64) void k_ctc_greedy(const float* logits, int* out_labels, int* out_len, float* out_logp, int T,
                                                   int C, int T_in, int out_stride) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int blank = C - 1;
  const float* lg = logits + (size_t)b * T * C;
  int* out = out_labels + (size_t)b * out_stride;
  int carry = -1, count = 0;                       // -1: no previous frame (equals no class)
  float logp = 0.f;
  for (int t0 = 0; t0 < T_in; t0 += 64) {
    const int n = min(64, T_in - t0);
    int sym = -1;
    for (int k = 0; k < n; ++k) {
      const float a = lane < C ? lg[(size_t)(t0 + k) * C + lane] : -INFINITY;
      const float lpv = dec_frame_lp(a, lane, C);
      const float mx = sg_wave_max(a);
      const unsigned long long top = __ballot(lane < C && a == mx);
      const int win = top ? __ffsll(top) - 1 : blank;              // lowest index among the tied classes (numpy.argmax); a frame of NaNs reads as blank
      logp += __shfl(lpv, win, 64);
      if (lane == k) sym = win;
    }
    int prev = __shfl_up(sym, 1, 64);
    if (lane == 0) prev = carry;
    const bool keep = lane < n && sym != blank && sym != prev;
    const unsigned long long flags = __ballot(keep);
    if (keep) out[count + __popcll(flags & ((1ull << lane) - 1ull))] = sym;       // count + kept <= T_in <= out_stride
    count += __popcll(flags);
    carry = __shfl(sym, n - 1, 64);
  }
  for (int j = count + lane; j < out_stride; j += 64) out[j] = -1;
  if (lane == 0) {
    out_len[b] = count;
    if (out_logp) out_logp[b] = logp;
  }
}

#define DEC_WAVES 4            // wavefronts per workgroup of k_ctc_score_words
#define DEC_WORDS_PER_WG 32    // words that share one staging of a sample's lp rows

// grid (word groups, B).  The sample's lp rows [T_in][C] are staged in LDS once per workgroup; then every wavefront walks its
// words alone (no further barrier): lanes are the extended-label states blank, w0, blank, w1, ..., blank of ONE word.
__global__ __launch_bounds__(64 * DEC_WAVES) void k_ctc_score_words(const float* lp_all, const int* words, const int* word_len,
                                                                    int word_stride, float* nll, int T, int C, int T_in, int W) {
  extern __shared__ __attribute__((aligned(16))) float lp[];        // [T_in][C]
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blank = C - 1;
  const float* src = lp_all + (size_t)b * T * C;
  for (int e = threadIdx.x; e < T_in * C; e += 64 * DEC_WAVES) lp[e] = src[e];
  __syncthreads();
  const int max_len = min(word_stride, 31);
  for (int w = blockIdx.x * DEC_WAVES + wave; w < W; w += gridDim.x * DEC_WAVES) {            // wave-uniform
    float* dst = nll + (size_t)b * W + w;
    const int len = word_len[w];
    if (len < 1 || len > max_len) {                 // poisoned like a bad label in k_softmax_ctc: +inf, never a clamped word
      if (lane == 0) *dst = INFINITY;
      continue;
    }
    const int S = 2 * len + 1;
    int lab = blank;
    bool bad = false;
    if (lane < S && (lane & 1)) {
      lab = words[(size_t)w * word_stride + (lane >> 1)];
      bad = lab < 0 || lab >= blank;
      lab = bad ? 0 : lab;
    }
    if (__ballot(bad) != 0ull) {
      if (lane == 0) *dst = INFINITY;
      continue;
    }
    const int lab_m2 = __shfl_up(lab, 2, 64);
    const bool skip_in = lane >= 2 && lane < S && lab != blank && lab != lab_m2;        // s-2 -> s allowed
    float a_cur = lane < 2 ? lp[lab] : -INFINITY;                                        // (S >= 3)
    for (int t = 1; t < T_in; ++t) {
      float a1 = __shfl_up(a_cur, 1, 64), a2 = __shfl_up(a_cur, 2, 64);
      if (lane < 1) a1 = -INFINITY;
      if (!skip_in) a2 = -INFINITY;
      const float v = dec_lse3(a_cur, a1, a2);
      a_cur = lane < S ? v + lp[t * C + lab] : -INFINITY;
    }
    const float aT1 = __shfl(a_cur, S - 1, 64), aT2 = __shfl(a_cur, S - 2, 64);
    if (lane == 0) *dst = -dec_lse2(aT1, aT2);      // a word that needs more frames than T_in: -(-inf) = +inf
  }
}

// One wavefront per sample; lane j holds D[i][j], the distance between the first i hypothesis and the first j reference
// characters.  A new row takes the two lane-local candidates tmp[j] = min(D[i-1][j] + 1, D[i-1][j-1] + (h_i != r_j)); the in-row
// candidate D[i][j-1] + 1 unrolls to D[i][j] = j + min_{k <= j} (tmp[k] - k), an inclusive min-scan over the lanes (6 shuffles).
__global__ __launch_bounds__(64) void k_edit_distance(const int* hyp, const int* hyp_len, int hyp_stride, const int* ref,
                                                      const int* ref_len, int ref_stride, int* dist) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int hl = hyp_len[b], rl = ref_len[b];
  if (hl < 0 || hl > hyp_stride || rl < 0 || rl > ref_stride) {      // lengths that do not fit their rows: -1, never a clamped read
    if (lane == 0) dist[b] = -1;
    return;
  }
  const int r = (lane >= 1 && lane <= rl) ? ref[(size_t)b * ref_stride + lane - 1] : -2;
  int row = lane;                                                   // D[0][j] = j
  for (int i0 = 0; i0 < hl; i0 += 64) {
    const int n = min(64, hl - i0);
    const int mine = lane < n ? hyp[(size_t)b * hyp_stride + i0 + lane] : -3;
    for (int k = 0; k < n; ++k) {
      const int h = __shfl(mine, k, 64);
      int diag = __shfl_up(row, 1, 64);
      int tmp = min(row + 1, diag + (h != r ? 1 : 0));
      if (lane == 0) tmp = i0 + k + 1;                              // D[i][0] = i
      int s = tmp - lane;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(s, o, 64);
        if (lane >= o) s = min(s, u);
      }
      row = s + lane;
    }
  }
  const int d = __shfl(row, rl, 64);                                // (lanes above rl hold values nobody reads)
  if (lane == 0) dist[b] = d;
}

__global__ __launch_bounds__(256) void k_legibility_sums(const int* dist, const int* ref_len, int B, double* sums) {
  __shared__ double part[4][3];
  double sd = 0.0, sr = 0.0, sw = 0.0;
  for (int b = threadIdx.x; b < B; b += 256) {
    sd += (double)dist[b];
    sr += (double)ref_len[b];
    sw += dist[b] != 0 ? 1.0 : 0.0;
  }
  sd = sg_wave_sum_d(sd); sr = sg_wave_sum_d(sr); sw = sg_wave_sum_d(sw);
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = sd; part[threadIdx.x >> 6][1] = sr; part[threadIdx.x >> 6][2] = sw;
  }
  __syncthreads();
  if (threadIdx.x == 0) {                            // one adder per address; calls on one stream are ordered
    for (int i = 0; i < 3; ++i) sums[i] += part[0][i] + part[1][i] + part[2][i] + part[3][i];
    sums[3] += (double)B;
  }
}

extern "C" int sg_ctc_log_probs(const float* logits, float* lp, int B, int T, int C, void* stream) {
  if (!logits || !lp || B < 1 || T < 1 || C < 2 || C > 64) return SG_ERR_ARG;
  const long rows = (long)B * T;
  SG_KERNEL(k_ctc_log_probs, dim3(sg_grid_for(rows, 4)), dim3(256), 0, (hipStream_t)stream, logits, lp, rows, C);
  return sg_launch_status();
}

extern "C" int sg_ctc_greedy_decode(const float* logits, int* out_labels, int* out_len, float* out_logp, int B, int T, int C,
                                    int input_length, int out_stride, void* stream) {
  if (!logits || !out_labels || !out_len || B < 1 || C < 2 || C > 64 || input_length < 1 || input_length > T ||
      out_stride < input_length)
    return SG_ERR_ARG;
  SG_KERNEL(k_ctc_greedy, dim3(B), dim3(64), 0, (hipStream_t)stream, logits, out_labels, out_len, out_logp, T, C, input_length,
            out_stride);
  return sg_launch_status();
}

extern "C" int sg_ctc_score_words(const float* lp, const int* words, const int* word_len, int word_stride, float* nll, int B, int T,
                                  int C, int input_length, int W, void* stream) {
  if (!lp || !words || !word_len || !nll || B < 1 || B > 65535 || W < 1 || word_stride < 1 || C < 2 || C > 64 || input_length < 1 ||
      input_length > T)
    return SG_ERR_ARG;
  const size_t lds = (size_t)input_length * C * sizeof(float);
  if (lds > 64 * 1024) return SG_ERR_UNSUPPORTED;
  SG_KERNEL(k_ctc_score_words, dim3(sg_cdiv(W, DEC_WORDS_PER_WG), B), dim3(64 * DEC_WAVES), lds, (hipStream_t)stream, lp, words,
            word_len, word_stride, nll, T, C, input_length, W);
  return sg_launch_status();
}

extern "C" int sg_edit_distance(const int* hyp, const int* hyp_len, int hyp_stride, const int* ref, const int* ref_len,
                                int ref_stride, int* dist, int B, void* stream) {
  if (!hyp || !hyp_len || !ref || !ref_len || !dist || B < 1 || hyp_stride < 1 || ref_stride < 1) return SG_ERR_ARG;
  if (ref_stride > 63) return SG_ERR_UNSUPPORTED;
  SG_KERNEL(k_edit_distance, dim3(B), dim3(64), 0, (hipStream_t)stream, hyp, hyp_len, hyp_stride, ref, ref_len, ref_stride, dist);
  return sg_launch_status();
}

extern "C" int sg_legibility_sums(const int* dist, const int* ref_len, int B, double* sums, void* stream) {
  if (!dist || !ref_len || !sums || B < 1) return SG_ERR_ARG;
  SG_KERNEL(k_legibility_sums, dim3(1), dim3(256), 0, (hipStream_t)stream, dist, ref_len, B, sums);
  return sg_launch_status();
}
