// Score of a given translation on the first-pass text decoder (fairseq's SequenceScorer, --score-reference): per logits row the
// log-probability of the row's target token, the arg-max and its log-probability, and the target's rank -- one read of the row.
// The plain log_softmax of get_normalized_probs: no pad / unk masking, no unk penalty, no temperature (the search's
// beam_prefix_score_kernel applies those and reads the row three times; it stays as it is).
#include "elementwise.hpp"

namespace ss {

// One logits row per 256-thread workgroup, thread t owns columns t, t + 256, ...  PER > 0: N <= 256 * PER, the row is read from
// global memory once (coalesced) and stays in registers across the two passes.  PER == 0: any N, the second pass reads the row again.
// Arithmetic of log_softmax_kernel (elementwise.hip) step for step -- f32 max; per-thread sums of accurate expf(x - mx) over the
// thread's columns ascending; wave_sum; (s0 + s1) + (s2 + s3); one logf; (x - mx) - lse -- so stat[] holds the bits that kernel
// writes at the target and at the arg-max column, whichever form runs.  Arg-max: the lowest index that holds the maximum
// (torch.max, launch_masked_argmax).  Rank: #{n: x[n] > x[tk]} + #{n < tk: x[n] == x[tk]}, integer work on the float32 logits.
// A NaN or +inf column or an all -inf row makes the sum NaN (fmaxf skips a NaN, expf(NaN) does not; inf - inf): NaN, NaN, -1, -1.
// A -inf column adds expf(-inf) = 0; a -inf target answers -inf and its rank.  tk outside [0, N): nothing is written.
// Every reduction in a fixed order: a row's answers depend on the row's bits alone, never on M or on the row's place.
template <int PER>
__global__ __launch_bounds__(256) void mt_token_score_kernel(const float* __restrict__ logits, int ld, int N,
                                                             const int* __restrict__ target, float* __restrict__ stat,
                                                             int* __restrict__ idx) {
  __shared__ float sm[4], ss[4];
  __shared__ int si[4], sr[4];
  __shared__ float s_xt;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t row = blockIdx.x;
  const int tk = target[row];
  if (tk < 0 || tk >= N) return;                               // the same for the whole workgroup
  const float* r = logits + row * ld;
  float v[PER > 0 ? PER : 1];
  float mx = -INFINITY;
  if constexpr (PER > 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int n = t + 256 * i;
      v[i] = n < N ? r[n] : -INFINITY;                         // past the row: a column that changes nothing (below)
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      mx = fmaxf(mx, v[i]);
      if (t + 256 * i == tk) s_xt = v[i];                      // one thread of the workgroup owns the target
    }
  } else {
    for (int n = t; n < N; n += 256) {
      const float x = r[n];
      mx = fmaxf(mx, x);
      if (n == tk) s_xt = x;
    }
  }
  mx = wave_max(mx);
  if (lane == 0) sm[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  const float xt = s_xt;
  float sum = 0.f;
  int bi = 0x7fffffff, rank = 0;
  auto visit = [&](int n, float x) {                           // n ascends per thread
    sum += expf(x - mx);
    if (x == mx) bi = min(bi, n);
    rank += (x > xt || (x == xt && n < tk)) ? 1 : 0;
  };
  if constexpr (PER > 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) visit(t + 256 * i, v[i]);    // a -inf past the row adds +0 to the sum, is no maximum of a good
                                                               // row and counts for no rank (it is never above xt, and n > tk)
  } else {
    for (int n = t; n < N; n += 256) visit(n, r[n]);
  }
  sum = wave_sum(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bi = min(bi, __shfl_xor(bi, o, 64));
    rank += __shfl_xor(rank, o, 64);
  }
  if (lane == 0) { ss[wave] = sum; si[wave] = bi; sr[wave] = rank; }
  __syncthreads();
  if (t == 0) {
    const float tot = (ss[0] + ss[1]) + (ss[2] + ss[3]);
    const float lse = logf(tot);
    const bool bad = tot != tot;
    stat[2 * row] = bad ? __builtin_nanf("") : (xt - mx) - lse;
    stat[2 * row + 1] = bad ? __builtin_nanf("") : (mx - mx) - lse;
    idx[2 * row] = bad ? -1 : min(min(si[0], si[1]), min(si[2], si[3]));
    idx[2 * row + 1] = bad ? -1 : (sr[0] + sr[1]) + (sr[2] + sr[3]);
  }
}

int launch_mt_token_scores(const float* logits, int ld, int M, int N, const int* target, float* stat, int* idx, hipStream_t stream,
                           int form) {
  if (!logits || !target || !stat || !idx || M <= 0 || N <= 0 || ld < N || M > MT_SCORE_MAX_ROWS) return SS_ERR_ARG;
#define SS_MTS(PER) \
  hipLaunchKernelGGL(mt_token_score_kernel<PER>, dim3(M), dim3(256), 0, stream, logits, ld, N, target, stat, idx)
  if (form == 1) SS_MTS(0);
  else if (N <= 2048) SS_MTS(8);
  else if (N <= 4096) SS_MTS(16);
  else if (N <= 6144) SS_MTS(24);
  else if (N <= MT_SCORE_MAX_REG_N) SS_MTS(32);
  else SS_MTS(0);
#undef SS_MTS
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss
