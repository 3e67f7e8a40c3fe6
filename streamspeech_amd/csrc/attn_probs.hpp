// Head-averaged attention probabilities (attn_probs.hip): what fairseq's MultiheadAttention returns as `attn_weights` with
// need_weights = True (researches/ctc_unity/modules/multihead_attention.py: softmax per head, then the mean over the heads) and the
// generator records as the hypothesis' "attention" (agent/sequence_generator.py:383-392).  The kernels of attention.hip are online
// soft-max forms and never hold a probability; this one materialises P, its row arg-max and two row statistics.
#pragma once
#include "common.hpp"

namespace ss {

constexpr int ATTN_PROBS_MAX_H = 8;

// Ragged launch over the segment tables of launch_attention: segs[4 s] = {q_start, q_len, k_start, k_len}, head h in columns
// [64 h, 64 h + 64) of Q / K.  Of segment s only query rows q_first[s] .. q_len - 1 are answered, n_s = q_len - q_first[s] of them;
// answered row i is output row o = row_off[s] + i - q_first[s]:
//   P[p_off[s] + (i - q_first[s]) * k_len + j] = (1 / H) sum_h softmax_j(scale * q_{i,h} . k_{j,h})     (P may be null: skipped)
//   peak[o] = arg-max_j P[i][j], the lowest j of a tie;  stat[2 o] = P[i][peak],  stat[2 o + 1] = sum_j j * P[i][j]
// A row's bits are a function of its own segment's keys alone.  All pointers are device pointers.
struct AttnProbsArgs {
  const float* Q = nullptr; const float* K = nullptr;
  int ldq = 0, ldk = 0;            // row strides in floats, multiples of 4
  int H = 0;                       // 1 .. ATTN_PROBS_MAX_H
  float scale = 1.0f;
  const int* segs = nullptr; int nseg = 0;
  const int* q_first = nullptr;    // [nseg]
  const int* row_off = nullptr;    // [nseg]
  const long long* p_off = nullptr;   // [nseg], in floats (needed with P only)
  float* P = nullptr;
  int* peak = nullptr;
  float* stat = nullptr;
  int max_rows = 0;                // the most answered rows of one segment (grid sizing)
};

int launch_attention_probs(const AttnProbsArgs& a, hipStream_t stream);

}  // namespace ss
