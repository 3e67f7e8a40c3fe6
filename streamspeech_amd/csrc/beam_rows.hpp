// The row phase of the search's step kernels, once: beam_topk_body, sample_step_kernel and beam_prefix_score_body call these, so a
// row's masked log-probabilities are the same bits in all three (sampling at k = 1 and the prefix scores are pinned against the
// beam path).  One workgroup of 256 threads per row.  Log-softmax numerics of log_softmax_kernel (elementwise.hip).
#pragma once
#include "beam.hpp"

namespace ss {

// dynamic LDS of a row kernel: the row, and with a ban the row's history [Lc] and the V-bit map behind it
inline size_t topk_lds_bytes(int V, int ngram, int Lc) {
  return (size_t)V * sizeof(float) + (ngram >= 2 ? ((size_t)Lc + (size_t)(V + 31) / 32) * sizeof(int) : 0);
}

// The reference's no-repeat ban (fairseq/fairseq/ngram_repeat_block.py::_no_repeat_ngram) with ngram = n >= 2.  The row's step + 1
// tokens are staged in LDS behind vals -- the forced ones from the utterance's prefix-pass tokens, the fed ones through the ancestry
// table -- the step + 2 - n windows are compared one per thread, and a match sets the bit of the token behind the window.
// -> the map [ceil(V / 32)], bit n: token n is banned at this step.
__device__ __forceinline__ unsigned* row_ban_map(const TopkOpts& o, float* vals, int V, int row, int b, int step, int np) {
  const int t = threadIdx.x;
  int* hist = reinterpret_cast<int*>(vals + V);      // [Lc] tokens[0 .. step] of the row
  unsigned* banned = reinterpret_cast<unsigned*>(hist + o.Lc);
  const int n1 = o.ngram - 1, nwin = step + 1 - n1;
  for (int p = t; p <= step; p += 256) {
    int tk = -1;
    if (p < np) tk = o.ptok[o.row0[b] + p];
    else {
      const int u = p - np, slot = o.anc[(size_t)row * o.Lc + o.c0 + u];
      if ((unsigned)slot < (unsigned)o.R) tk = o.tok[(size_t)u * o.R + slot];
    }
    hist[p] = tk;
  }
  for (int w = t; w < (V + 31) / 32; w += 256) banned[w] = 0u;
  __syncthreads();
  for (int i = t; i < nwin; i += 256) {              // window i against the last n - 1 tokens, tokens[nwin .. step]
    bool same = true;
    for (int j = 0; j < n1 && same; ++j) same = hist[i + j] == hist[nwin + j];
    const int tk = hist[i + n1];
    if (same && (unsigned)tk < (unsigned)V) atomicOr(&banned[tk >> 5], 1u << (tk & 31));
  }
  __syncthreads();
  return banned;
}

// The row maximum, and the four waves' sums of exp(logit - max) left in sa [4] behind a barrier: two passes over logit(n), which
// carries the temperature divide where there is one.
template <class Logit>
__device__ __forceinline__ float row_max_sums(Logit logit, int V, float* sa) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float mx = -INFINITY;
  for (int n = t; n < V; n += 256) mx = fmaxf(mx, logit(n));
  mx = wave_max(mx);
  if (lane == 0) sa[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sa[0], sa[1]), fmaxf(sa[2], sa[3]));
  __syncthreads();
  float sum = 0.f;
  for (int n = t; n < V; n += 256) sum += expf(logit(n) - mx);
  sum = wave_sum(sum);
  if (lane == 0) sa[wave] = sum;
  __syncthreads();
  return mx;
}

// the log-sum-exp of the row from those sums, in the one fixed order
__device__ __forceinline__ float row_lse(const float* sa) { return logf((sa[0] + sa[1]) + (sa[2] + sa[3])); }

// The masks in the reference's order (unity/sequence_generator.py:290-327): NaN -> -inf, pad -inf, unk -= unk_penalty, step >= max_len:
// all but </s> -inf, step < min_len: </s> -inf; then the ban, then the constraints' </s> ban, and the cumulative score last.
struct RowMask {
  int pad, unk, eos;
  float unk_pen;
  bool at_max = false, below_min = false;
  const unsigned* banned = nullptr;   // row_ban_map, or null
  bool ban_eos = false;               // constraints: the row's state is not finished
  bool add_cum = false; float cum = 0.f;
};

template <class Logit>
__device__ __forceinline__ float row_masked_lprob(Logit logit, int n, float mx, float lse, const RowMask& m) {
  float v = (logit(n) - mx) - lse;
  if (v != v) v = -INFINITY;
  if (n == m.pad) v = -INFINITY;
  if (n == m.unk) v -= m.unk_pen;
  if (m.at_max && n != m.eos) v = -INFINITY;
  if (m.below_min && n == m.eos) v = -INFINITY;
  if (m.banned && ((m.banned[n >> 5] >> (n & 31)) & 1u)) v = -INFINITY;
  if (m.ban_eos && n == m.eos) v = -INFINITY;
  if (m.add_cum) v = v + m.cum;
  return v;
}

}  // namespace ss
