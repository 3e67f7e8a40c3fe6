// CTC prefix beam search on the two text CTC heads (blank = 0): the most likely TEXT -- the labelling whose probability, summed over
// all its alignments, is highest -- and its runners-up, where the greedy search (ctc_scores.hip) gives the most likely frame path
// and the aligner (ctc_align.hip) scores a given text.  The scores are on the aligner's scale, log p(y | x).  Two kernels:
//   ctc_beam_cand_kernel    per packed frame row the log-softmax denominator (max, log-sum) and the ids of the `cand` largest
//                           logits among the unmasked non-blank columns
//   ctc_beam_search_kernel  one workgroup per utterance, a loop over its frames: beam, candidates and merge state in LDS, the trie
//                           of label strings and its child table in global scratch, the back-trace of the n-best at the end
// The plain-C++ twin of both (ss_ctc_beam_host) is ctc_beam_host.hip; the search, its order and the frame -- passes B and C, node
// creation, the back-trace, the LM finish -- are ctc_beam.hpp's, called by the body below and by the twin: this file keeps the loops
// over 256 threads, the barriers, the rank walk and the slot writes of the next beam.
// The search kernel and the twin each have an LM form (ctc_beam_search_lm_kernel, ss_ctc_beam_lm_host): the same body
// with a back-off n-gram model (ngram_lm.hpp) fused into the order of a frame's entries.  And each of the four has a RESUMABLE form
// (ctc_stream_search_kernel / _lm_kernel, ctc_stream_host_run; the object and its entry points: ctc_stream.hip): the same body
// over a slot's state that outlives the launch, for the frames a call brings, with the stable prefix of the beam at the end.
// The BIAS forms (ctc_beam_search_bias_kernel / _lm_bias_kernel and their resumable pair; ctc_beam.hpp, ctc_bias.hpp) are the same
// body once more, with a hotword set's phrase automaton as one more term of the bonus, alone or beside the model.
#include "ctc_beam.hpp"

#include <cstring>
#include <type_traits>

#include "ctc_bias.hpp"
#include "ngram_lm.hpp"

#include "../../include/streamspeech_hip.h"
#include "ctc_row.hpp"
#include "elementwise.hpp"

namespace ss {

namespace {
constexpr int NONE = 0x7fffffff;
}

// One logits row per workgroup.  den[row] = (max, log-sum), the denominator of ctc_row.hpp -- (NaN, NaN) for a row that holds a
// NaN.  cand_id[row][k]: the k-th column in the order (logit descending, id
// ascending) among the columns that are not blank, pad or unk and whose logit is above -inf; -1 where there are fewer.  One round
// of the block per candidate: every thread offers its best column that comes after the last winner in that order.
// PER > 0: N <= 256 * PER, the row is read once and kept in registers; PER == 0: any N, every pass reads the row again.
template <int PER>
__global__ __launch_bounds__(256) void ctc_beam_cand_kernel(const float* __restrict__ logits, int ld, int N, int pad, int unk, int C,
                                                            float* __restrict__ den, int* __restrict__ cand_id) {
  __shared__ float sm[4], ssum[4], swv[8];
  __shared__ int sn[4], swi[8];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x;
  const float* r = logits + (size_t)row * ld;
  float v[PER > 0 ? PER : 1];                                  // (a column past the row is -inf: never a candidate either)
  const float mx = ctc_row_max<PER>(r, N, v, sm, sn);
  ctc_row_expsum<PER>(r, N, v, mx, ssum);
  if (t == 0) {
    const bool bad = ctc_row_nan(sn);
    den[2 * (size_t)row] = bad ? __builtin_nanf("") : mx;
    den[2 * (size_t)row + 1] = bad ? __builtin_nanf("") : ctc_row_logsum(ssum);
  }
  // ---- the candidates: round k finds the k-th column of the order; (lv, li) is the winner of the round before ----
  float lv = INFINITY;
  int li = -1;
  for (int k = 0; k < C; ++k) {
    float bv = -INFINITY;
    int bi = NONE;
    auto offer = [&](int n, float x) {                         // n ascends per thread: the first maximum wins
      if (n == 0 || n == pad || n == unk || !(x > -INFINITY)) return;
      if (!(x < lv || (x == lv && n > li))) return;
      if (bi == NONE || x > bv) { bv = x; bi = n; }
    };
    if constexpr (PER > 0) {
#pragma unroll
      for (int i = 0; i < PER; ++i) offer(t + 256 * i, v[i]);
    } else {
      for (int n = t; n < N; n += 256) offer(n, r[n]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != NONE && (bi == NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    const int buf = (k & 1) * 4;                               // two sets of wave partials: one barrier per round
    if (lane == 0) { swv[buf + wave] = bv; swi[buf + wave] = bi; }
    __syncthreads();
    bv = swv[buf]; bi = swi[buf];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float ov = swv[buf + w];
      const int oi = swi[buf + w];
      if (oi != NONE && (bi == NONE || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    if (t == 0) cand_id[(size_t)row * C + k] = bi == NONE ? -1 : bi;
    lv = bi == NONE ? -INFINITY : bv;                          // nothing left: nothing comes after it either
    li = bi;
  }
}

// One utterance per workgroup, a loop over its frames with four barriers each (the trip count and every barrier are uniform: T,
// the beam's size and the NaN exit are the same for all threads).
//   A  the frame's values: lp of the blank, of the candidates and of every beam prefix's last label, as (x - max) - logsum from the
//      row itself and the candidate kernel's den
//   B  the entries e = r * (C + 1) + k, a thread per entry (ctc_beam_entry_b)
//   C  each prefix's own entry, a thread per prefix (ctc_beam_entry_c)
//   D  every live entry counts the entries that come before it (ctc_beam_before); with fewer than `beam` of them it is the next
//      beam's prefix of that rank, and makes its node if the string is new (ctc_beam_make_node)
// The two beams are addressed by an integer offset (0 | CTC_BEAM_MAX_BEAM), never through a pointer picked at run time (see
// ctc_align_trellis_kernel).  Every operation of an utterance happens inside its own workgroup in an order that depends on its own
// data alone (node ids are ctc_beam_new_node's, not a counter's; the child table's contents depend on the insertion order only in
// which of two colliding keys sits first, never in what a lookup returns), so its outputs are the same bits alone and in any pack.
// The LM form (LM = true; ctc_beam.hpp, ngram_lm.hpp) is the same body: the frame's order compares e_fus = tot + bonus in place of
// e_tot (8 more bytes of LDS per entry and 8 per beam slot: 8.9 KB at the caps), pass B looks up the bonus of an extension that
// is alive (its node's, or lp_lm from the parent's state: one chain of dependent probes per entry, parallel over the entries),
// pass D gives a new node its three LM fields, and the end ranks the last beam by fin.  The plain form compiles to what it was.
struct CtcBeamLm {
  NgramView lm;
  double lm_weight, word_score;
  int eos_term, pad_;
  double* n_sum;     // [nodes] of the pack, as nodes_all
  double* n_bonus;
  int* n_state;
};

// The bias forms (FORM & CTC_FORM_BIAS; ctc_beam.hpp, ctc_bias.hpp) keep their key where the LM form does -- e_fus and b_bonus,
// nothing more per entry or beam slot -- pass B adds the automaton's step from the parent's b_state to the lookup of a live
// extension that is not in the trie, pass D gives a new node its bias_sum and b_state, and the end takes the finish term off fin.
// The arrays are indexed as the LM's: [nodes] of the pack, or [S][nodes] of a resumable object's slots.
struct CtcBeamBias {
  BiasView bv;
  double scale;
  int finish, pad_;
  double* n_bsum;
  int* n_bstate;
};

// The resumable form (RES = true; ctc_beam.hpp, ss_ctc_stream_advance) is the same body again: workgroup b serves session R.sess[b],
// whose trie, table and stored beam are its slot's (R); the beam is loaded where the one-shot form makes the root (a call that
// starts at frame 0 makes the root), the loop runs the absolute frames [f, upto) over the stacked new rows, the beam is stored
// back, the n-best are written as the one-shot form writes them (the eos term only in the utterance's last call), and one pass
// more finds the stable prefix.  segs / keys_all / vals_all / nodes_all are unused.  The one-shot forms compile to what they were.
template <int FORM, bool RES>
__device__ __forceinline__ void ctc_beam_search_body(const float* __restrict__ logits, int ld, const CtcBeamSeg* __restrict__ segs,
                                                     int beam, int C, int nbest, const float* den, const int* cand_id,
                                                     unsigned long long* keys_all, int* vals_all, int2* nodes_all, void* hyps_out,
                                                     int* tokens, int out_stride, const CtcBeamLm& L, const CtcStreamDev& R,
                                                     const CtcBeamBias& Z) {
  constexpr int MB = CTC_BEAM_MAX_BEAM;
  constexpr bool LM = (FORM & CTC_FORM_LM) != 0, BIAS = (FORM & CTC_FORM_BIAS) != 0, FUSED = FORM != 0;
  __shared__ double b_pb[2 * MB], b_pnb[2 * MB], b_tot[2 * MB];
  __shared__ int b_node[2 * MB], b_last[2 * MB];
  __shared__ double s_pb[MB], s_pnb[MB], s_give[MB];
  __shared__ double e_tot[CTC_BEAM_MAX_ENT];
  __shared__ int e_node[CTC_BEAM_MAX_ENT];
  __shared__ int s_c[CTC_BEAM_MAX_CAND];
  __shared__ float s_lpc[CTC_BEAM_MAX_CAND], s_lpl[MB], s_lp0;
  __shared__ int s_nb[2];
  __shared__ double e_fus[FUSED ? CTC_BEAM_MAX_ENT : 1], b_bonus[FUSED ? 2 * MB : 1];
  const int tid = threadIdx.x;
  CtcBeamSeg sg;                                               // RES: the slot's offsets; row0 + t is the row of ABSOLUTE frame t
  CtcStreamSess se{};
  int t0 = 0;
  if constexpr (RES) {
    se = R.sess[blockIdx.x];
    sg = CtcBeamSeg{se.slot * R.nodes_per, se.slot * R.slots_per, se.row0 - se.f, se.upto, (int)(R.slots_per - 1), 0};
    t0 = se.f;
  } else {
    sg = segs[blockIdx.x];
  }
  unsigned long long* keys = (RES ? R.keys : keys_all) + sg.tab_off;
  int* vals = (RES ? R.vals : vals_all) + sg.tab_off;
  int2* nodes = (RES ? R.nodes : nodes_all) + sg.node_off;
  double* n_sum = LM ? (RES ? R.n_sum : L.n_sum) + sg.node_off : nullptr;
  double* n_bonus = FUSED ? (RES ? R.n_bonus : L.n_bonus) + sg.node_off : nullptr;
  int* n_state = LM ? (RES ? R.n_state : L.n_state) + sg.node_off : nullptr;
  double* n_bsum = BIAS ? Z.n_bsum + sg.node_off : nullptr;
  int* n_bstate = BIAS ? Z.n_bstate + sg.node_off : nullptr;
  const int mask = sg.tab_mask, W = C + 1;
  double* st_f64 = RES ? R.b_f64 + (size_t)se.slot * 4 * beam : nullptr;   // the stored beam of the slot
  int* st_i32 = RES ? R.b_i32 + (size_t)se.slot * (2 * beam + 2) : nullptr;
  const CtcBeamFrame F{b_pb, b_pnb, b_tot, b_bonus, b_node, b_last, s_pb, s_pnb, s_give, e_tot, e_fus, e_node,
                       s_c,  s_lpc, s_lpl, &s_lp0,  keys,   vals,   mask, n_bonus, n_state, n_bstate};
  bool bad = false;
  if (!RES || t0 == 0) {
    if (tid == 0) {
      b_pb[0] = 0.0; b_pnb[0] = -INFINITY; b_tot[0] = 0.0; b_node[0] = 0; b_last[0] = -1;
      s_nb[0] = 1;
      nodes[0] = make_int2(-1, -1);
      if constexpr (LM) { b_bonus[0] = 0.0; n_sum[0] = 0.0; n_bonus[0] = 0.0; n_state[0] = L.lm.start; }
      if constexpr (BIAS) { b_bonus[0] = 0.0; n_bonus[0] = 0.0; n_bsum[0] = 0.0; n_bstate[0] = 0; }
    }
  } else if constexpr (RES) {
    const int nb = st_i32[2 * beam];                           // (uniform; at most beam)
    bad = st_i32[2 * beam + 1] != 0;                           // a NaN row of an earlier call: sticky, no frame runs
    if (bad) t0 = sg.T;
    if (tid < nb) {
      b_pb[tid] = st_f64[tid]; b_pnb[tid] = st_f64[beam + tid]; b_tot[tid] = st_f64[2 * beam + tid];
      if constexpr (FUSED) b_bonus[tid] = st_f64[3 * beam + tid];
      b_node[tid] = st_i32[tid]; b_last[tid] = st_i32[beam + tid];
    }
    if (tid == 0) s_nb[0] = nb;
  }
  __syncthreads();
  int cur = 0;
  for (int t = t0; t < sg.T; ++t) {
    const int row = sg.row0 + t, co = cur * MB, no = (cur ^ 1) * MB;
    const int nb = s_nb[cur];
    const float mx = den[2 * (size_t)row], ls = den[2 * (size_t)row + 1];
    if (ls != ls) { bad = true; break; }                       // a NaN in the row (uniform: every thread reads the same pair)
    const float* r = logits + (size_t)row * ld;
    // ---- A ----
    if (tid < C) {
      const int c = cand_id[(size_t)row * C + tid];
      s_c[tid] = c;
      s_lpc[tid] = c >= 0 ? ctc_beam_lp(r[c], mx, ls) : -INFINITY;
    } else if (tid >= 64 && tid < 64 + nb) {
      const int i = tid - 64, last = b_last[co + i];
      s_lpl[i] = last >= 0 ? ctc_beam_lp(r[last], mx, ls) : -INFINITY;
      s_give[i] = -INFINITY;
    } else if (tid == 128) {
      s_lp0 = ctc_beam_lp(r[0], mx, ls);
      s_nb[cur ^ 1] = 0;
    }
    __syncthreads();
    // ---- B ----
    const int n_ent = nb * W;
    for (int e = tid; e < n_ent; e += 256) ctc_beam_entry_b<FORM>(F, co, nb, W, e, L.lm, L.lm_weight, L.word_score, Z.bv, Z.scale);
    __syncthreads();
    // ---- C ----
    if (tid < nb) ctc_beam_entry_c<FORM>(F, co, W, tid);
    __syncthreads();
    // ---- D ---- (a thread's up to PER entries count in ONE walk over the frame's totals: each total is read once per thread,
    //               and no exit depends on a count, so the loads of the unrolled walk overlap)
    constexpr int PER = (CTC_BEAM_MAX_ENT + 255) / 256;
    const double* e_key = FUSED ? e_fus : e_tot;               // (a compile-time choice: what the order compares)
    double my_tot[PER];
    int my_rank[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + 256 * j;
      my_tot[j] = e < n_ent ? e_key[e] : -INFINITY;
      my_rank[j] = 0;
    }
    if (n_ent > 256 || my_tot[0] > -INFINITY) {
#pragma unroll 4
      for (int f = 0; f < n_ent; ++f) {
        const double tf = e_key[f];
#pragma unroll
        for (int j = 0; j < PER; ++j) my_rank[j] += ctc_beam_before(tf, f, my_tot[j], tid + 256 * j);
      }
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int e = tid + 256 * j, rank = my_rank[j];
      double tot = my_tot[j];
      if (!(tot > -INFINITY) || rank >= beam) continue;       // (an entry past n_ent is -inf)
      if constexpr (FUSED) tot = e_tot[e];                     // the state keeps the pure CTC total
      const int i = e / W, k = e - i * W - 1;
      int node = e_node[e];
      if (k < 0) {
        b_pb[no + rank] = s_pb[i]; b_pnb[no + rank] = s_pnb[i]; b_last[no + rank] = b_last[co + i];
        if constexpr (FUSED) b_bonus[no + rank] = b_bonus[co + i];
      } else {
        const int c = s_c[k];
        if (node < 0)                                          // a new string
          node = ctc_beam_make_node<FORM>(t, beam, rank, b_node[co + i], c, FUSED ? b_bonus[co + i] : 0.0, keys, vals, mask, nodes,
                                          n_sum, n_bonus, n_state, L.lm, L.lm_weight, L.word_score, n_bsum, n_bstate, Z.bv, Z.scale);
        b_pb[no + rank] = -INFINITY; b_pnb[no + rank] = tot; b_last[no + rank] = c;
        if constexpr (FUSED) b_bonus[no + rank] = n_bonus[node];
      }
      b_tot[no + rank] = tot; b_node[no + rank] = node;
      atomicMax(&s_nb[cur ^ 1], rank + 1);                     // ranks are 0 .. alive - 1 without a gap
    }
    __syncthreads();
    cur ^= 1;
  }
  if constexpr (RES) {                                         // the beam that left frame upto - 1, for the next call
    const int nb = bad ? 0 : s_nb[cur];
    if (tid < nb) {
      st_f64[tid] = b_pb[cur * MB + tid]; st_f64[beam + tid] = b_pnb[cur * MB + tid]; st_f64[2 * beam + tid] = b_tot[cur * MB + tid];
      if constexpr (FUSED) st_f64[3 * beam + tid] = b_bonus[cur * MB + tid];
      st_i32[tid] = b_node[cur * MB + tid]; st_i32[beam + tid] = b_last[cur * MB + tid];
    }
    if (tid == 0) { st_i32[2 * beam] = nb; st_i32[2 * beam + 1] = bad ? 1 : 0; }
  }
  if constexpr (!FUSED) {
    // ---- the n-best: the last beam in rank order; thread r walks prefix r back through the trie ----
    ss_ctc_beam_hyp* hyps = static_cast<ss_ctc_beam_hyp*>(hyps_out);
    if (tid < nbest) {
      const int nb = bad ? 0 : s_nb[cur];
      ss_ctc_beam_hyp h;
      h.score = bad ? (double)__builtin_nanf("") : -INFINITY;
      h.n_tokens = 0;
      h.status = bad ? 2 : 1;
      if (tid < nb) {
        h.n_tokens = ctc_beam_trace(nodes, b_node[cur * MB + tid], tokens + ((size_t)blockIdx.x * nbest + tid) * out_stride);
        h.score = b_tot[cur * MB + tid]; h.status = 0;
      }
      hyps[(size_t)blockIdx.x * nbest + tid] = h;
    }
  } else {
    // ---- the n-best of the LM and bias forms: thread r finishes prefix r of the last beam (all of it: the eos and finish terms
    //      can lift a prefix from behind the first nbest), the beam is ranked by fin (s_give), and a prefix of rank < nbest walks
    //      back ----
    typedef typename std::conditional<BIAS, ss_ctc_beam_bias_hyp, ss_ctc_beam_lm_hyp>::type Hyp;
    Hyp* hyps = static_cast<Hyp*>(hyps_out);
    const int nb = bad ? 0 : s_nb[cur];                        // (uniform, as the barrier below)
    double fin = -INFINITY, lm_sum = 0.0;
    [[maybe_unused]] double bias_sum = 0.0;
    if (tid < nb) {
      const int node = b_node[cur * MB + tid];
      if constexpr (LM)
        ctc_beam_finish(b_tot[cur * MB + tid], b_bonus[cur * MB + tid], n_sum[node], n_state[node],
                        L.eos_term && (!RES || se.fin) ? L.lm.eos : -1, L.lm, L.lm_weight, &fin, &lm_sum);
      else
        fin = b_tot[cur * MB + tid] + b_bonus[cur * MB + tid];
      if constexpr (BIAS)
        ctc_beam_bias_finish(Z.bv, n_bstate[node], n_bsum[node], Z.scale, Z.finish && (!RES || se.fin), &fin, &bias_sum);
      s_give[tid] = fin;
    }
    __syncthreads();
    if (tid < nb) {
      int rank = 0;
      for (int f = 0; f < nb; ++f) rank += ctc_beam_before(s_give[f], f, fin, tid);
      if (rank < nbest) {
        Hyp h;
        h.n_tokens = ctc_beam_trace(nodes, b_node[cur * MB + tid], tokens + ((size_t)blockIdx.x * nbest + rank) * out_stride);
        h.score = fin; h.ctc_score = b_tot[cur * MB + tid]; h.lm_score = lm_sum; h.status = 0;
        if constexpr (BIAS) h.bias_score = bias_sum;
        hyps[(size_t)blockIdx.x * nbest + rank] = h;
      }
    } else if (tid < nbest) {                                  // an empty slot
      Hyp h;
      h.score = h.ctc_score = bad ? (double)__builtin_nanf("") : -INFINITY;
      h.lm_score = 0.0; h.n_tokens = 0; h.status = bad ? 2 : 1;
      if constexpr (BIAS) h.bias_score = 0.0;
      hyps[(size_t)blockIdx.x * nbest + tid] = h;
    }
  }
  if constexpr (RES) {
    // ---- the stable prefix: what every string of the beam starts with.  Thread r finds the depth of the lowest common ancestor
    //      of prefix r and prefix 0 by walking parents (at most `frames` steps each, as the n-best walk); the block minimum ----
    __shared__ int s_stable;
    const int nb = bad ? 0 : s_nb[cur];
    if (tid == 0) s_stable = NONE;
    __syncthreads();
    if (tid < nb) atomicMin(&s_stable, ctc_beam_lca_depth(nodes, b_node[cur * MB + tid], b_node[cur * MB]));
    __syncthreads();
    if (tid == 0) R.part[blockIdx.x] = CtcStreamPart{se.upto, nb > 0 ? s_stable : 0, nb, bad ? 2 : 0};
  }
}

__global__ __launch_bounds__(256) void ctc_beam_search_kernel(const float* __restrict__ logits, int ld, const CtcBeamSeg* __restrict__ segs,
                                                              int beam, int C, int nbest, const float* den, const int* cand_id,
                                                              unsigned long long* keys_all, int* vals_all, int2* nodes_all,
                                                              ss_ctc_beam_hyp* hyps, int* tokens, int out_stride) {
  ctc_beam_search_body<0, false>(logits, ld, segs, beam, C, nbest, den, cand_id, keys_all, vals_all, nodes_all, hyps, tokens,
                                 out_stride, CtcBeamLm{}, CtcStreamDev{}, CtcBeamBias{});
}

__global__ __launch_bounds__(256) void ctc_beam_search_lm_kernel(const float* __restrict__ logits, int ld,
                                                                 const CtcBeamSeg* __restrict__ segs, int beam, int C, int nbest,
                                                                 const float* den, const int* cand_id, unsigned long long* keys_all,
                                                                 int* vals_all, int2* nodes_all, ss_ctc_beam_lm_hyp* hyps, int* tokens,
                                                                 int out_stride, CtcBeamLm L) {
  ctc_beam_search_body<CTC_FORM_LM, false>(logits, ld, segs, beam, C, nbest, den, cand_id, keys_all, vals_all, nodes_all, hyps, tokens,
                                           out_stride, L, CtcStreamDev{}, CtcBeamBias{});
}

// The bias forms: L carries the bonus array (and the model, in the LM + bias form; unused otherwise), Z the hotword set.
__global__ __launch_bounds__(256) void ctc_beam_search_bias_kernel(const float* __restrict__ logits, int ld,
                                                                   const CtcBeamSeg* __restrict__ segs, int beam, int C, int nbest,
                                                                   const float* den, const int* cand_id, unsigned long long* keys_all,
                                                                   int* vals_all, int2* nodes_all, ss_ctc_beam_bias_hyp* hyps,
                                                                   int* tokens, int out_stride, CtcBeamLm L, CtcBeamBias Z) {
  ctc_beam_search_body<CTC_FORM_BIAS, false>(logits, ld, segs, beam, C, nbest, den, cand_id, keys_all, vals_all, nodes_all, hyps,
                                             tokens, out_stride, L, CtcStreamDev{}, Z);
}

__global__ __launch_bounds__(256) void ctc_beam_search_lm_bias_kernel(const float* __restrict__ logits, int ld,
                                                                      const CtcBeamSeg* __restrict__ segs, int beam, int C, int nbest,
                                                                      const float* den, const int* cand_id,
                                                                      unsigned long long* keys_all, int* vals_all, int2* nodes_all,
                                                                      ss_ctc_beam_bias_hyp* hyps, int* tokens, int out_stride,
                                                                      CtcBeamLm L, CtcBeamBias Z) {
  ctc_beam_search_body<CTC_FORM_LM | CTC_FORM_BIAS, false>(logits, ld, segs, beam, C, nbest, den, cand_id, keys_all, vals_all,
                                                           nodes_all, hyps, tokens, out_stride, L, CtcStreamDev{}, Z);
}

// The resumable kernels: one workgroup per session of the call (R.sess), logits the stacked new rows.
__global__ __launch_bounds__(256) void ctc_stream_search_kernel(const float* __restrict__ logits, int ld, int beam, int C, int nbest,
                                                                const float* den, const int* cand_id, ss_ctc_beam_hyp* hyps,
                                                                int* tokens, int out_stride, CtcStreamDev R) {
  ctc_beam_search_body<0, true>(logits, ld, nullptr, beam, C, nbest, den, cand_id, nullptr, nullptr, nullptr, hyps, tokens,
                                out_stride, CtcBeamLm{}, R, CtcBeamBias{});
}

__global__ __launch_bounds__(256) void ctc_stream_search_lm_kernel(const float* __restrict__ logits, int ld, int beam, int C, int nbest,
                                                                   const float* den, const int* cand_id, ss_ctc_beam_lm_hyp* hyps,
                                                                   int* tokens, int out_stride, CtcBeamLm L, CtcStreamDev R) {
  ctc_beam_search_body<CTC_FORM_LM, true>(logits, ld, nullptr, beam, C, nbest, den, cand_id, nullptr, nullptr, nullptr, hyps, tokens,
                                          out_stride, L, R, CtcBeamBias{});
}

__global__ __launch_bounds__(256) void ctc_stream_search_bias_kernel(const float* __restrict__ logits, int ld, int beam, int C, int nbest,
                                                                     const float* den, const int* cand_id, ss_ctc_beam_bias_hyp* hyps,
                                                                     int* tokens, int out_stride, CtcBeamLm L, CtcStreamDev R,
                                                                     CtcBeamBias Z) {
  ctc_beam_search_body<CTC_FORM_BIAS, true>(logits, ld, nullptr, beam, C, nbest, den, cand_id, nullptr, nullptr, nullptr, hyps, tokens,
                                            out_stride, L, R, Z);
}

__global__ __launch_bounds__(256) void ctc_stream_search_lm_bias_kernel(const float* __restrict__ logits, int ld, int beam, int C,
                                                                        int nbest, const float* den, const int* cand_id,
                                                                        ss_ctc_beam_bias_hyp* hyps, int* tokens, int out_stride,
                                                                        CtcBeamLm L, CtcStreamDev R, CtcBeamBias Z) {
  ctc_beam_search_body<CTC_FORM_LM | CTC_FORM_BIAS, true>(logits, ld, nullptr, beam, C, nbest, den, cand_id, nullptr, nullptr, nullptr,
                                                          hyps, tokens, out_stride, L, R, Z);
}

size_t ctc_beam_table_bytes(const CtcBeamPlan& p) { return p.segs.size() * sizeof(CtcBeamSeg); }

static int launch_ctc_beam_cand(const float* logits, int ld, int V, int pad, int unk, int rows, int C, float* den, int* cand,
                                hipStream_t stream) {
#define SS_CBC(PER) \
  hipLaunchKernelGGL(ctc_beam_cand_kernel<PER>, dim3(rows), dim3(256), 0, stream, logits, ld, V, pad, unk, C, den, cand)
  if (V <= 2048) SS_CBC(8);
  else if (V <= 4096) SS_CBC(16);
  else if (V <= 6144) SS_CBC(24);
  else if (V <= 8192) SS_CBC(32);
  else SS_CBC(0);
#undef SS_CBC
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// lm == nullptr: the plain search, hyps an ss_ctc_beam_hyp array; else the LM form (d_work holds plan.work_bytes_lm()), hyps an
// ss_ctc_beam_lm_hyp array.  bias != nullptr: a bias form, with or without lm (d_work holds plan.work_bytes_form(form)), hyps an
// ss_ctc_beam_bias_hyp array.
int launch_ctc_beam(const float* logits, int ld, int V, int pad, int unk, const CtcBeamPlan& p, void* d_table, void* d_work,
                    const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, void* hyps, int* tokens, int out_stride, float* den_out,
                    int* cand_out, hipStream_t stream, const ss_ctc_bias* bias, const ss_ctc_bias_opts* bopts) {
  const int B = (int)p.segs.size();
  if (!logits || ld < V || B <= 0 || !d_table || !d_work || !hyps || !tokens) return SS_ERR_ARG;
  CtcBeamLm L{};
  CtcBeamBias Z{};
  if (bias) {
    RET(ctc_beam_bias_check(bias, V, pad, unk, bopts, lm, opts));
    RET(bias_device_view(bias, &Z.bv));
  }
  if (lm) {
    RET(ctc_beam_lm_check(lm, V, opts));
    RET(ngram_device_view(lm, &L.lm));
  }
  unsigned char* w = static_cast<unsigned char*>(d_work);
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(w);
  int2* nodes = reinterpret_cast<int2*>(w + p.key_bytes());
  int* vals = reinterpret_cast<int*>(w + p.key_bytes() + (size_t)p.nodes * 8);
  float* den = reinterpret_cast<float*>(w + (size_t)p.slots * 12 + (size_t)p.nodes * 8);
  int* cand = reinterpret_cast<int*>(den + 2 * (size_t)p.rows);
  if (den_out) den = den_out;
  if (cand_out) cand = cand_out;
  SS_HIP_CHECK(hipMemcpyAsync(d_table, p.segs.data(), ctc_beam_table_bytes(p), hipMemcpyHostToDevice, stream));
  SS_HIP_CHECK(hipMemsetAsync(keys, 0xff, p.key_bytes(), stream));
  RET(launch_ctc_beam_cand(logits, ld, V, pad, unk, p.rows, p.cand, den, cand, stream));
  if (bias) {
    const int form = CTC_FORM_BIAS | (lm ? CTC_FORM_LM : 0);
    const CtcFormNodes fn = ctc_form_carve(w + p.lm_off(), (size_t)p.nodes, form);
    if (lm) { L.lm_weight = opts->lm_weight; L.word_score = opts->word_score; L.eos_term = opts->eos_term ? 1 : 0; }
    L.n_sum = fn.n_sum; L.n_bonus = fn.n_bonus; L.n_state = fn.n_state;
    Z.scale = bopts->scale; Z.finish = bopts->finish ? 1 : 0;
    Z.n_bsum = fn.n_bsum; Z.n_bstate = fn.n_bstate;
    if (lm)
      hipLaunchKernelGGL(ctc_beam_search_lm_bias_kernel, dim3(B), dim3(256), 0, stream, logits, ld,
                         static_cast<const CtcBeamSeg*>(d_table), p.beam, p.cand, p.nbest, den, cand, keys, vals, nodes,
                         static_cast<ss_ctc_beam_bias_hyp*>(hyps), tokens, out_stride, L, Z);
    else
      hipLaunchKernelGGL(ctc_beam_search_bias_kernel, dim3(B), dim3(256), 0, stream, logits, ld,
                         static_cast<const CtcBeamSeg*>(d_table), p.beam, p.cand, p.nbest, den, cand, keys, vals, nodes,
                         static_cast<ss_ctc_beam_bias_hyp*>(hyps), tokens, out_stride, L, Z);
  } else if (!lm) {
    hipLaunchKernelGGL(ctc_beam_search_kernel, dim3(B), dim3(256), 0, stream, logits, ld, static_cast<const CtcBeamSeg*>(d_table),
                       p.beam, p.cand, p.nbest, den, cand, keys, vals, nodes, static_cast<ss_ctc_beam_hyp*>(hyps), tokens, out_stride);
  } else {
    L.lm_weight = opts->lm_weight; L.word_score = opts->word_score; L.eos_term = opts->eos_term ? 1 : 0;
    L.n_sum = reinterpret_cast<double*>(w + p.lm_off());
    L.n_bonus = L.n_sum + p.nodes;
    L.n_state = reinterpret_cast<int*>(L.n_bonus + p.nodes);
    hipLaunchKernelGGL(ctc_beam_search_lm_kernel, dim3(B), dim3(256), 0, stream, logits, ld, static_cast<const CtcBeamSeg*>(d_table),
                       p.beam, p.cand, p.nbest, den, cand, keys, vals, nodes, static_cast<ss_ctc_beam_lm_hyp*>(hyps), tokens,
                       out_stride, L);
  }
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_ctc_stream(const float* logits, int ld, int V, int pad, int unk, int rows, int n, const CtcStreamSess* h_sess, void* d_sess,
                      float* den, int* cand_id, int beam, int C, int nbest, CtcStreamDev dev, const ss_ngram_lm* lm,
                      const ss_ctc_lm_opts* opts, void* hyps, int* tokens, int out_stride, CtcStreamPart* part, hipStream_t stream,
                      const ss_ctc_bias* bias, const ss_ctc_bias_opts* bopts, CtcStreamBiasDev bdev) {
  CtcBeamLm L{};
  CtcBeamBias Z{};
  if (lm) RET(ngram_device_view(lm, &L.lm));
  if (bias) RET(bias_device_view(bias, &Z.bv));
  SS_HIP_CHECK(hipMemcpyAsync(d_sess, h_sess, (size_t)n * sizeof(CtcStreamSess), hipMemcpyHostToDevice, stream));
  if (rows > 0) RET(launch_ctc_beam_cand(logits, ld, V, pad, unk, rows, C, den, cand_id, stream));
  dev.sess = static_cast<const CtcStreamSess*>(d_sess);
  dev.part = part;
  if (bias) {
    if (lm) { L.lm_weight = opts->lm_weight; L.word_score = opts->word_score; L.eos_term = opts->eos_term ? 1 : 0; }
    Z.scale = bopts->scale; Z.finish = bopts->finish ? 1 : 0;
    Z.n_bsum = bdev.n_bsum; Z.n_bstate = bdev.n_bstate;
    if (lm)
      hipLaunchKernelGGL(ctc_stream_search_lm_bias_kernel, dim3(n), dim3(256), 0, stream, logits, ld, beam, C, nbest, den, cand_id,
                         static_cast<ss_ctc_beam_bias_hyp*>(hyps), tokens, out_stride, L, dev, Z);
    else
      hipLaunchKernelGGL(ctc_stream_search_bias_kernel, dim3(n), dim3(256), 0, stream, logits, ld, beam, C, nbest, den, cand_id,
                         static_cast<ss_ctc_beam_bias_hyp*>(hyps), tokens, out_stride, L, dev, Z);
  } else if (!lm) {
    hipLaunchKernelGGL(ctc_stream_search_kernel, dim3(n), dim3(256), 0, stream, logits, ld, beam, C, nbest, den, cand_id,
                       static_cast<ss_ctc_beam_hyp*>(hyps), tokens, out_stride, dev);
  } else {
    L.lm_weight = opts->lm_weight; L.word_score = opts->word_score; L.eos_term = opts->eos_term ? 1 : 0;
    hipLaunchKernelGGL(ctc_stream_search_lm_kernel, dim3(n), dim3(256), 0, stream, logits, ld, beam, C, nbest, den, cand_id,
                       static_cast<ss_ctc_beam_lm_hyp*>(hyps), tokens, out_stride, L, dev);
  }
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss
