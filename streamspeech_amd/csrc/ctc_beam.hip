// CTC prefix beam search on the two text CTC heads (blank = 0): the most likely TEXT -- the labelling whose probability, summed over
// all its alignments, is highest -- and its runners-up, where the greedy search (ctc_scores.hip) gives the most likely frame path
// and the aligner (ctc_align.hip) scores a given text.  The scores are on the aligner's scale, log p(y | x).  Two kernels:
//   ctc_beam_cand_kernel    per packed frame row the log-softmax denominator (max, log-sum) and the ids of the `cand` largest
//                           logits among the unmasked non-blank columns
//   ctc_beam_search_kernel  one workgroup per utterance, a loop over its frames: beam, candidates and merge state in LDS, the trie
//                           of label strings and its child table in global scratch, the back-trace of the n-best at the end
// plus the plain-C++ twin of both (ss_ctc_beam_host) over the same step code (ctc_beam.hpp, where the search and its order are
// defined).  The search kernel and the twin each have an LM form (ctc_beam_search_lm_kernel, ss_ctc_beam_lm_host): the same body
// with a back-off n-gram model (ngram_lm.hpp) fused into the order of a frame's entries.  And each of the four has a RESUMABLE form
// (ctc_stream_search_kernel / _lm_kernel, ctc_stream_host_run; the object and its entry points: ctc_stream.hip): the same body
// over a slot's state that outlives the launch, for the frames a call brings, with the stable prefix of the beam at the end.
#include "ctc_beam.hpp"

#include <cstring>

#include "ngram_lm.hpp"

#include "../../include/streamspeech_hip.h"
#include "elementwise.hpp"

namespace ss {

namespace {
constexpr int NONE = 0x7fffffff;
}

// One logits row per workgroup.  den[row] = (max, log-sum) with masked_argmax_lprob_kernel's arithmetic, operation for operation:
// an f32 max, each thread's f32 sum of expf(x - max) in ascending stride, the xor-shuffle tree, the four wave partials in index
// order, one logf -- (NaN, NaN) for a row that holds a NaN.  cand_id[row][k]: the k-th column in the order (logit descending, id
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
  float v[PER > 0 ? PER : 1];
  float mx = -INFINITY;
  int nan = 0;
  if constexpr (PER > 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int n = t + 256 * i;
      v[i] = n < N ? r[n] : -INFINITY;                         // past the row: no maximum, exp(-inf - max) = 0, never a candidate
      nan |= (v[i] != v[i]);
      mx = fmaxf(mx, v[i]);
    }
  } else {
    for (int n = t; n < N; n += 256) { const float x = r[n]; nan |= (x != x); mx = fmaxf(mx, x); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); nan |= __shfl_xor(nan, o, 64); }
  if (lane == 0) { sm[wave] = mx; sn[wave] = nan; }
  __syncthreads();
  mx = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float sum = 0.f;
  if constexpr (PER > 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const float e = expf(v[i] - mx);
      if (t + 256 * i < N) sum += e;
    }
  } else {
    for (int n = t; n < N; n += 256) sum += expf(r[n] - mx);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) ssum[wave] = sum;
  __syncthreads();
  if (t == 0) {
    const bool bad = sn[0] | sn[1] | sn[2] | sn[3];
    den[2 * (size_t)row] = bad ? __builtin_nanf("") : mx;
    den[2 * (size_t)row + 1] = bad ? __builtin_nanf("") : logf(((ssum[0] + ssum[1]) + ssum[2]) + ssum[3]);
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
//   B  the entries e = r * (C + 1) + k (ctc_beam.hpp): a prefix's own stay terms; an extension's term and its node from the child
//      table -- an extension whose node is in the beam hands its term to that prefix and dies
//   C  each prefix's own entry: pnb' = logadd(stay, handed term), total = logadd(pb', pnb')
//   D  every live entry counts the entries that come before it (ctc_beam_before); with fewer than `beam` of them it is the next
//      beam's prefix of that rank, and makes its node if the string is new
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

// The resumable form (RES = true; ctc_beam.hpp, ss_ctc_stream_advance) is the same body again: workgroup b serves session R.sess[b],
// whose trie, table and stored beam are its slot's (R); the beam is loaded where the one-shot form makes the root (a call that
// starts at frame 0 makes the root), the loop runs the absolute frames [f, upto) over the stacked new rows, the beam is stored
// back, the n-best are written as the one-shot form writes them (the eos term only in the utterance's last call), and one pass
// more finds the stable prefix.  segs / keys_all / vals_all / nodes_all are unused.  The one-shot forms compile to what they were.
template <bool LM, bool RES>
__device__ __forceinline__ void ctc_beam_search_body(const float* __restrict__ logits, int ld, const CtcBeamSeg* __restrict__ segs,
                                                     int beam, int C, int nbest, const float* den, const int* cand_id,
                                                     unsigned long long* keys_all, int* vals_all, int2* nodes_all, void* hyps_out,
                                                     int* tokens, int out_stride, const CtcBeamLm& L, const CtcStreamDev& R) {
  constexpr int MB = CTC_BEAM_MAX_BEAM;
  __shared__ double b_pb[2 * MB], b_pnb[2 * MB], b_tot[2 * MB];
  __shared__ int b_node[2 * MB], b_last[2 * MB];
  __shared__ double s_pb[MB], s_pnb[MB], s_give[MB];
  __shared__ double e_tot[CTC_BEAM_MAX_ENT];
  __shared__ int e_node[CTC_BEAM_MAX_ENT];
  __shared__ int s_c[CTC_BEAM_MAX_CAND];
  __shared__ float s_lpc[CTC_BEAM_MAX_CAND], s_lpl[MB], s_lp0;
  __shared__ int s_nb[2];
  __shared__ double e_fus[LM ? CTC_BEAM_MAX_ENT : 1], b_bonus[LM ? 2 * MB : 1];
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
  double* n_bonus = LM ? (RES ? R.n_bonus : L.n_bonus) + sg.node_off : nullptr;
  int* n_state = LM ? (RES ? R.n_state : L.n_state) + sg.node_off : nullptr;
  const int mask = sg.tab_mask, W = C + 1;
  double* st_f64 = RES ? R.b_f64 + (size_t)se.slot * 4 * beam : nullptr;   // the stored beam of the slot
  int* st_i32 = RES ? R.b_i32 + (size_t)se.slot * (2 * beam + 2) : nullptr;
  bool bad = false;
  if (!RES || t0 == 0) {
    if (tid == 0) {
      b_pb[0] = 0.0; b_pnb[0] = -INFINITY; b_tot[0] = 0.0; b_node[0] = 0; b_last[0] = -1;
      s_nb[0] = 1;
      nodes[0] = make_int2(-1, -1);
      if constexpr (LM) { b_bonus[0] = 0.0; n_sum[0] = 0.0; n_bonus[0] = 0.0; n_state[0] = L.lm.start; }
    }
  } else if constexpr (RES) {
    const int nb = st_i32[2 * beam];                           // (uniform; at most beam)
    bad = st_i32[2 * beam + 1] != 0;                           // a NaN row of an earlier call: sticky, no frame runs
    if (bad) t0 = sg.T;
    if (tid < nb) {
      b_pb[tid] = st_f64[tid]; b_pnb[tid] = st_f64[beam + tid]; b_tot[tid] = st_f64[2 * beam + tid];
      if constexpr (LM) b_bonus[tid] = st_f64[3 * beam + tid];
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
    for (int e = tid; e < n_ent; e += 256) {
      const int i = e / W, k = e - i * W - 1;
      const int node = b_node[co + i], last = b_last[co + i];
      if (k < 0) {
        double pb2, pnb2;
        ctc_beam_stay(b_pnb[co + i], b_tot[co + i], last, s_lp0, s_lpl[i], &pb2, &pnb2);
        s_pb[i] = pb2; s_pnb[i] = pnb2;
        e_node[e] = node;                                      // (its total: pass C)
        continue;
      }
      const int c = s_c[k];
      double term = -INFINITY;
      int child = -1;
      if (c >= 0) {
        term = ctc_beam_ext(b_pb[co + i], b_tot[co + i], last, c, s_lpc[k]);
        child = ctc_beam_find(keys, vals, mask, node, c);
        if (child >= 0) {
          for (int j = 0; j < nb; ++j) {
            if (b_node[co + j] == child) { s_give[j] = term; term = -INFINITY; break; }   // one parent per string: one writer per j
          }
        }
      }
      e_tot[e] = term;
      e_node[e] = child;
      if constexpr (LM) {
        double fus = -INFINITY;
        if (term > -INFINITY) {                                // (a dead entry needs no bonus: no lookup)
          double bonus;
          if (child >= 0) {
            bonus = n_bonus[child];
          } else {
            int nx;
            bonus = ngram_bonus(b_bonus[co + i], L.lm_weight, ngram_lp(L.lm, n_state[node], c, &nx), L.word_score);
          }
          fus = term + bonus;
        }
        e_fus[e] = fus;
      }
    }
    __syncthreads();
    // ---- C ----
    if (tid < nb) {
      const double pnb2 = ctc_beam_logadd(s_pnb[tid], s_give[tid]);
      s_pnb[tid] = pnb2;
      const double tot = ctc_beam_logadd(s_pb[tid], pnb2);
      e_tot[tid * W] = tot;
      if constexpr (LM) e_fus[tid * W] = tot > -INFINITY ? tot + b_bonus[co + tid] : -INFINITY;
    }
    __syncthreads();
    // ---- D ---- (a thread's up to PER entries count in ONE walk over the frame's totals: each total is read once per thread,
    //               and no exit depends on a count, so the loads of the unrolled walk overlap)
    constexpr int PER = (CTC_BEAM_MAX_ENT + 255) / 256;
    const double* e_key = LM ? e_fus : e_tot;                  // (a compile-time choice: what the order compares)
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
      if constexpr (LM) tot = e_tot[e];                        // the state keeps the pure CTC total
      const int i = e / W, k = e - i * W - 1;
      int node = e_node[e];
      if (k < 0) {
        b_pb[no + rank] = s_pb[i]; b_pnb[no + rank] = s_pnb[i]; b_last[no + rank] = b_last[co + i];
        if constexpr (LM) b_bonus[no + rank] = b_bonus[co + i];
      } else {
        const int c = s_c[k];
        if (node < 0) {                                        // a new string: its node, then its place in the child table
          node = ctc_beam_new_node(t, beam, rank);
          nodes[node] = make_int2(b_node[co + i], c);
          if constexpr (LM) {                                  // its LM fields, written once (the lookup of pass B again)
            int nx;
            const double lp = ngram_lp(L.lm, n_state[b_node[co + i]], c, &nx);
            n_state[node] = nx;
            n_sum[node] = n_sum[b_node[co + i]] + lp;
            n_bonus[node] = ngram_bonus(b_bonus[co + i], L.lm_weight, lp, L.word_score);
          }
          const unsigned long long key = ctc_beam_key(b_node[co + i], c);
          for (int s = ctc_beam_slot(key, mask), n = 0; n <= mask; ++n, s = (s + 1) & mask) {
            if (atomicCAS(&keys[s], CTC_BEAM_EMPTY, key) == CTC_BEAM_EMPTY) { vals[s] = node; break; }
          }
        }
        b_pb[no + rank] = -INFINITY; b_pnb[no + rank] = tot; b_last[no + rank] = c;
        if constexpr (LM) b_bonus[no + rank] = n_bonus[node];
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
      if constexpr (LM) st_f64[3 * beam + tid] = b_bonus[cur * MB + tid];
      st_i32[tid] = b_node[cur * MB + tid]; st_i32[beam + tid] = b_last[cur * MB + tid];
    }
    if (tid == 0) { st_i32[2 * beam] = nb; st_i32[2 * beam + 1] = bad ? 1 : 0; }
  }
  if constexpr (!LM) {
    // ---- the n-best: the last beam in rank order; thread r walks prefix r back through the trie ----
    ss_ctc_beam_hyp* hyps = static_cast<ss_ctc_beam_hyp*>(hyps_out);
    if (tid < nbest) {
      const int nb = bad ? 0 : s_nb[cur];
      ss_ctc_beam_hyp h;
      h.score = bad ? (double)__builtin_nanf("") : -INFINITY;
      h.n_tokens = 0;
      h.status = bad ? 2 : 1;
      if (tid < nb) {
        const int node = b_node[cur * MB + tid];
        int len = 0;
        for (int n = node; n > 0; n = nodes[n].x) ++len;
        int* out = tokens + ((size_t)blockIdx.x * nbest + tid) * out_stride;
        int j = len;
        for (int n = node; n > 0 && j > 0; n = nodes[n].x) out[--j] = nodes[n].y;
        h.score = b_tot[cur * MB + tid]; h.n_tokens = len; h.status = 0;
      }
      hyps[(size_t)blockIdx.x * nbest + tid] = h;
    }
  } else {
    // ---- the n-best of the LM form: thread r finishes prefix r of the last beam (all of it: the eos term can lift a prefix
    //      from behind the first nbest), the beam is ranked by fin (s_give), and a prefix of rank < nbest walks back ----
    ss_ctc_beam_lm_hyp* hyps = static_cast<ss_ctc_beam_lm_hyp*>(hyps_out);
    const int nb = bad ? 0 : s_nb[cur];                        // (uniform, as the barrier below)
    double fin = -INFINITY, lm_sum = 0.0;
    if (tid < nb) {
      const int node = b_node[cur * MB + tid];
      const double fused = b_tot[cur * MB + tid] + b_bonus[cur * MB + tid];
      lm_sum = n_sum[node];
      fin = fused;
      if (L.eos_term && (!RES || se.fin)) {
        int nx;
        const double lp = ngram_lp(L.lm, n_state[node], L.lm.eos, &nx);
        fin = ngram_finish(fused, L.lm_weight, lp);
        lm_sum += lp;
      }
      s_give[tid] = fin;
    }
    __syncthreads();
    if (tid < nb) {
      int rank = 0;
      for (int f = 0; f < nb; ++f) rank += ctc_beam_before(s_give[f], f, fin, tid);
      if (rank < nbest) {
        const int node = b_node[cur * MB + tid];
        int len = 0;
        for (int n = node; n > 0; n = nodes[n].x) ++len;
        int* out = tokens + ((size_t)blockIdx.x * nbest + rank) * out_stride;
        int j = len;
        for (int n = node; n > 0 && j > 0; n = nodes[n].x) out[--j] = nodes[n].y;
        ss_ctc_beam_lm_hyp h;
        h.score = fin; h.ctc_score = b_tot[cur * MB + tid]; h.lm_score = lm_sum; h.n_tokens = len; h.status = 0;
        hyps[(size_t)blockIdx.x * nbest + rank] = h;
      }
    } else if (tid < nbest) {                                  // an empty slot
      ss_ctc_beam_lm_hyp h;
      h.score = h.ctc_score = bad ? (double)__builtin_nanf("") : -INFINITY;
      h.lm_score = 0.0; h.n_tokens = 0; h.status = bad ? 2 : 1;
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
    if (tid < nb) {
      int a = b_node[cur * MB + tid], b = b_node[cur * MB];
      int da = 0, db = 0;
      for (int n = a; n > 0; n = nodes[n].x) ++da;
      for (int n = b; n > 0; n = nodes[n].x) ++db;
      for (; da > db; --da) a = nodes[a].x;
      for (; db > da; --db) b = nodes[b].x;
      for (; a != b; --da) { a = nodes[a].x; b = nodes[b].x; }
      atomicMin(&s_stable, da);
    }
    __syncthreads();
    if (tid == 0) R.part[blockIdx.x] = CtcStreamPart{se.upto, nb > 0 ? s_stable : 0, nb, bad ? 2 : 0};
  }
}

__global__ __launch_bounds__(256) void ctc_beam_search_kernel(const float* __restrict__ logits, int ld, const CtcBeamSeg* __restrict__ segs,
                                                              int beam, int C, int nbest, const float* den, const int* cand_id,
                                                              unsigned long long* keys_all, int* vals_all, int2* nodes_all,
                                                              ss_ctc_beam_hyp* hyps, int* tokens, int out_stride) {
  ctc_beam_search_body<false, false>(logits, ld, segs, beam, C, nbest, den, cand_id, keys_all, vals_all, nodes_all, hyps, tokens,
                                     out_stride, CtcBeamLm{}, CtcStreamDev{});
}

__global__ __launch_bounds__(256) void ctc_beam_search_lm_kernel(const float* __restrict__ logits, int ld,
                                                                 const CtcBeamSeg* __restrict__ segs, int beam, int C, int nbest,
                                                                 const float* den, const int* cand_id, unsigned long long* keys_all,
                                                                 int* vals_all, int2* nodes_all, ss_ctc_beam_lm_hyp* hyps, int* tokens,
                                                                 int out_stride, CtcBeamLm L) {
  ctc_beam_search_body<true, false>(logits, ld, segs, beam, C, nbest, den, cand_id, keys_all, vals_all, nodes_all, hyps, tokens,
                                    out_stride, L, CtcStreamDev{});
}

// The resumable kernels: one workgroup per session of the call (R.sess), logits the stacked new rows.
__global__ __launch_bounds__(256) void ctc_stream_search_kernel(const float* __restrict__ logits, int ld, int beam, int C, int nbest,
                                                                const float* den, const int* cand_id, ss_ctc_beam_hyp* hyps,
                                                                int* tokens, int out_stride, CtcStreamDev R) {
  ctc_beam_search_body<false, true>(logits, ld, nullptr, beam, C, nbest, den, cand_id, nullptr, nullptr, nullptr, hyps, tokens,
                                    out_stride, CtcBeamLm{}, R);
}

__global__ __launch_bounds__(256) void ctc_stream_search_lm_kernel(const float* __restrict__ logits, int ld, int beam, int C, int nbest,
                                                                   const float* den, const int* cand_id, ss_ctc_beam_lm_hyp* hyps,
                                                                   int* tokens, int out_stride, CtcBeamLm L, CtcStreamDev R) {
  ctc_beam_search_body<true, true>(logits, ld, nullptr, beam, C, nbest, den, cand_id, nullptr, nullptr, nullptr, hyps, tokens,
                                   out_stride, L, R);
}

size_t ctc_beam_table_bytes(const CtcBeamPlan& p) { return p.segs.size() * sizeof(CtcBeamSeg); }

// What an LM call is refused for past the plain refusals, before anything is launched or written.
int ctc_beam_lm_check(const ss_ngram_lm* lm, int V, const ss_ctc_lm_opts* o) {
  if (!lm || !o || lm->host.V != V || !std::isfinite(o->lm_weight) || !std::isfinite(o->word_score)) return SS_ERR_ARG;
  if (o->eos_term && lm->host.eos < 0) return SS_ERR_ARG;
  return SS_OK;
}

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
// ss_ctc_beam_lm_hyp array.
static int launch_ctc_beam_any(const float* logits, int ld, int V, int pad, int unk, const CtcBeamPlan& p, void* d_table, void* d_work,
                               const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, void* hyps, int* tokens, int out_stride,
                               float* den_out, int* cand_out, hipStream_t stream) {
  const int B = (int)p.segs.size();
  if (!logits || ld < V || B <= 0 || !d_table || !d_work || !hyps || !tokens) return SS_ERR_ARG;
  CtcBeamLm L{};
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
  if (!lm) {
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

int launch_ctc_beam(const float* logits, int ld, int V, int pad, int unk, const CtcBeamPlan& p, void* d_table, void* d_work,
                    ss_ctc_beam_hyp* hyps, int* tokens, int out_stride, float* den_out, int* cand_out, hipStream_t stream) {
  return launch_ctc_beam_any(logits, ld, V, pad, unk, p, d_table, d_work, nullptr, nullptr, hyps, tokens, out_stride, den_out, cand_out,
                             stream);
}

int launch_ctc_beam_lm(const float* logits, int ld, int V, int pad, int unk, const CtcBeamPlan& p, void* d_table, void* d_work,
                       const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, ss_ctc_beam_lm_hyp* hyps, int* tokens, int out_stride,
                       float* den_out, int* cand_out, hipStream_t stream) {
  if (!lm) return SS_ERR_ARG;
  return launch_ctc_beam_any(logits, ld, V, pad, unk, p, d_table, d_work, lm, opts, hyps, tokens, out_stride, den_out, cand_out, stream);
}

int launch_ctc_stream(const float* logits, int ld, int V, int pad, int unk, int rows, int n, const CtcStreamSess* h_sess, void* d_sess,
                      float* den, int* cand_id, int beam, int C, int nbest, CtcStreamDev dev, const ss_ngram_lm* lm,
                      const ss_ctc_lm_opts* opts, void* hyps, int* tokens, int out_stride, CtcStreamPart* part, hipStream_t stream) {
  CtcBeamLm L{};
  if (lm) RET(ngram_device_view(lm, &L.lm));
  SS_HIP_CHECK(hipMemcpyAsync(d_sess, h_sess, (size_t)n * sizeof(CtcStreamSess), hipMemcpyHostToDevice, stream));
  if (rows > 0) RET(launch_ctc_beam_cand(logits, ld, V, pad, unk, rows, C, den, cand_id, stream));
  dev.sess = static_cast<const CtcStreamSess*>(d_sess);
  dev.part = part;
  if (!lm) {
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

namespace {

int g_host_max_beam = CTC_BEAM_MAX_BEAM;      // ss_debug_ctc_beam_host_max: the host twin's cap alone (the exhaustive test)

// ctc_beam_cand_kernel's denominator on the host, in the device's order (ctc_align.hip: row_stats_host).
void row_den_host(const float* r, int N, float* den) {
  float mx = -INFINITY;
  bool nan = false;
  for (int n = 0; n < N; ++n) { nan |= r[n] != r[n]; mx = fmaxf(mx, r[n]); }
  float part[256], tmp[256];
  for (int t = 0; t < 256; ++t) {
    float s = 0.f;
    for (int n = t; n < N; n += 256) s += expf(r[n] - mx);
    part[t] = s;
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int t = 0; t < 256; ++t) tmp[t] = part[t] + part[t ^ o];
    memcpy(part, tmp, sizeof(part));
  }
  den[0] = nan ? __builtin_nanf("") : mx;
  den[1] = nan ? __builtin_nanf("") : logf(((part[0] + part[64]) + part[128]) + part[192]);
}

void row_cand_host(const float* r, int N, int pad, int unk, int C, int* out) {
  float lv = INFINITY;
  int li = -1;
  for (int k = 0; k < C; ++k) {
    float bv = -INFINITY;
    int bi = NONE;
    for (int n = 1; n < N; ++n) {
      const float x = r[n];
      if (n == pad || n == unk || !(x > -INFINITY) || !(x < lv || (x == lv && n > li))) continue;
      if (bi == NONE || x > bv) { bv = x; bi = n; }
    }
    out[k] = bi == NONE ? -1 : bi;
    lv = bi == NONE ? -INFINITY : bv;
    li = bi;
  }
}

}  // namespace

}  // namespace ss

using namespace ss;

extern "C" int ss_debug_ctc_beam_host_max(int max_beam) {
  const int was = g_host_max_beam;
  if (max_beam >= 1) g_host_max_beam = max_beam;
  return was;
}

// ---- the twin of both forms, in three steps over one utterance's state (CtcBeamHostState, ctc_beam.hpp) so that the one-shot twins
// (start, all frames, emit) and the resumable twin (ss_ctc_stream_advance_host: start at a reset, some frames and an emit per
// call) are one statement of the search.  LM = false: lv / lw / ws unused, records ss_ctc_beam_hyp. ----
namespace ss {

void CtcBeamHostState::start(int beam, int max_T, bool lm, int lm_start) {
  long long slots = ctc_stream_slots(beam, max_T);
  mask = (int)(slots - 1);
  const size_t nodes = 1 + (size_t)beam * max_T;
  keys.assign((size_t)slots, CTC_BEAM_EMPTY);
  vals.assign((size_t)slots, -1);
  par.assign(nodes, -1); tok.assign(nodes, -1);
  if (lm) { n_sum.assign(nodes, 0.0); n_bonus.assign(nodes, 0.0); n_state.assign(nodes, 0); n_state[0] = lm_start; }
  bm.assign(1, CtcBeamHostPre{0.0, -INFINITY, 0.0, 0, -1, 0.0});
  frames = 0; bad = false;
}

// The frames S.frames .. S.frames + n - 1 from the n rows at `rows`; h_den [n][2] / h_cand [n][C] (may be NULL) receive the
// candidate kernel's values of every one of them, whatever the search makes of it.
template <bool LM>
static void ctc_beam_host_frames(CtcBeamHostState& S, const float* rows, int ld, int V, int pad, int unk, int n, int beam, int C,
                                 const NgramView& lv, double lw, double ws, float* h_den, int32_t* h_cand_id) {
  const int W = C + 1, mask = S.mask;
  std::vector<unsigned long long>& keys = S.keys;
  std::vector<int>&vals = S.vals, &par = S.par, &tok = S.tok, &n_state = S.n_state;
  std::vector<double>&n_sum = S.n_sum, &n_bonus = S.n_bonus;
  std::vector<CtcBeamHostPre>& bm = S.bm;
  typedef CtcBeamHostPre Pre;
  std::vector<Pre> nx;
  std::vector<double> e_tot, s_pb, s_pnb, s_give, e_fus;
  std::vector<int> e_node, cid_all((size_t)n * C);
  std::vector<float> den_all(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {                                // the candidate kernel: every row, whatever the search makes of it
    const float* r = rows + (size_t)i * ld;
    row_den_host(r, V, &den_all[2 * (size_t)i]);
    row_cand_host(r, V, pad, unk, C, &cid_all[(size_t)i * C]);
  }
  if (h_den && n > 0) memcpy(h_den, den_all.data(), den_all.size() * sizeof(float));
  if (h_cand_id && n > 0) memcpy(h_cand_id, cid_all.data(), cid_all.size() * sizeof(int));
  const int f0 = S.frames;
  S.frames += n;
  for (int t = f0; t < f0 + n && !S.bad; ++t) {
    const float* r = rows + (size_t)(t - f0) * ld;
    const float* den = &den_all[2 * (size_t)(t - f0)];
    const int* cid = &cid_all[(size_t)(t - f0) * C];
    if (den[1] != den[1]) { S.bad = true; break; }
    const int nb = (int)bm.size(), n_ent = nb * W;
    const float lp0 = ctc_beam_lp(r[0], den[0], den[1]);
    e_tot.assign(n_ent, -INFINITY); e_node.assign(n_ent, -1);
    if constexpr (LM) e_fus.assign(n_ent, -INFINITY);
    s_pb.assign(nb, -INFINITY); s_pnb.assign(nb, -INFINITY); s_give.assign(nb, -INFINITY);
    for (int e = 0; e < n_ent; ++e) {                          // B
      const int i = e / W, k = e - i * W - 1;
      const Pre& q = bm[i];
      if (k < 0) {
        ctc_beam_stay(q.pnb, q.tot, q.last, lp0, q.last >= 0 ? ctc_beam_lp(r[q.last], den[0], den[1]) : -INFINITY, &s_pb[i], &s_pnb[i]);
        e_node[e] = q.node;
        continue;
      }
      const int c = cid[k];
      if (c < 0) continue;
      double term = ctc_beam_ext(q.pb, q.tot, q.last, c, ctc_beam_lp(r[c], den[0], den[1]));
      const int child = ctc_beam_find(keys.data(), vals.data(), mask, q.node, c);
      if (child >= 0) {
        for (int j = 0; j < nb; ++j) {
          if (bm[j].node == child) { s_give[j] = term; term = -INFINITY; break; }
        }
      }
      e_tot[e] = term; e_node[e] = child;
      if constexpr (LM) {
        if (term > -INFINITY) {
          int st;
          const double bonus = child >= 0 ? n_bonus[child] : ngram_bonus(q.bonus, lw, ngram_lp(lv, n_state[q.node], c, &st), ws);
          e_fus[e] = term + bonus;
        }
      }
    }
    for (int i = 0; i < nb; ++i) {                             // C
      s_pnb[i] = ctc_beam_logadd(s_pnb[i], s_give[i]);
      e_tot[i * W] = ctc_beam_logadd(s_pb[i], s_pnb[i]);
      if constexpr (LM) e_fus[i * W] = e_tot[i * W] > -INFINITY ? e_tot[i * W] + bm[i].bonus : -INFINITY;
    }
    const std::vector<double>& e_key = LM ? e_fus : e_tot;     // what the order compares
    nx.assign(beam, Pre{0, 0, 0, -1, -1, 0.0});                // D
    int alive = 0;
    for (int e = 0; e < n_ent; ++e) {
      const double tot = e_tot[e], key = e_key[e];
      if (!(key > -INFINITY)) continue;
      int rank = 0;
      for (int f = 0; f < n_ent && rank < beam; ++f) rank += ctc_beam_before(e_key[f], f, key, e);
      if (rank >= beam) continue;
      const int i = e / W, k = e - i * W - 1;
      int node = e_node[e];
      if (k < 0) {
        nx[rank] = Pre{s_pb[i], s_pnb[i], tot, node, bm[i].last, bm[i].bonus};
      } else {
        const int c = cid[k];
        if (node < 0) {
          node = ctc_beam_new_node(t, beam, rank);
          par[node] = bm[i].node; tok[node] = c;
          if constexpr (LM) {
            int st;
            const double lp = ngram_lp(lv, n_state[bm[i].node], c, &st);
            n_state[node] = st; n_sum[node] = n_sum[bm[i].node] + lp; n_bonus[node] = ngram_bonus(bm[i].bonus, lw, lp, ws);
          }
          const unsigned long long key = ctc_beam_key(bm[i].node, c);
          for (int s = ctc_beam_slot(key, mask), n = 0; n <= mask; ++n, s = (s + 1) & mask) {
            if (keys[s] == CTC_BEAM_EMPTY) { keys[s] = key; vals[s] = node; break; }
          }
        }
        nx[rank] = Pre{-INFINITY, tot, tot, node, c, LM ? n_bonus[node] : 0.0};
      }
      if (rank + 1 > alive) alive = rank + 1;
    }
    nx.resize(alive);
    bm.swap(nx);
  }
}

// The n-best of the beam as it stands: h_hyps_b [nbest] records and h_tokens_b [nbest][out_stride] of this utterance.  eos: the LM
// form's eos term.
template <bool LM>
static void ctc_beam_host_emit(const CtcBeamHostState& S, int nbest, bool eos, const NgramView& lv, double lw, void* h_hyps_b,
                               int32_t* h_tokens_b, int out_stride) {
  const std::vector<CtcBeamHostPre>& bm = S.bm;
  const std::vector<int>&par = S.par, &tok = S.tok;
  const bool bad = S.bad;
  if constexpr (!LM) {
    ss_ctc_beam_hyp* h_hyps = static_cast<ss_ctc_beam_hyp*>(h_hyps_b);
    for (int k = 0; k < nbest; ++k) {
      ss_ctc_beam_hyp& h = h_hyps[k];
      h.score = bad ? (double)__builtin_nanf("") : -INFINITY; h.n_tokens = 0; h.status = bad ? 2 : 1;
      if (bad || k >= (int)bm.size()) continue;
      int len = 0;
      for (int n = bm[k].node; n > 0; n = par[n]) ++len;
      int32_t* out = h_tokens_b + (size_t)k * out_stride;
      int j = len;
      for (int n = bm[k].node; n > 0; n = par[n]) out[--j] = tok[n];
      h.score = bm[k].tot; h.n_tokens = len; h.status = 0;
    }
  } else {
    ss_ctc_beam_lm_hyp* h_hyps = static_cast<ss_ctc_beam_lm_hyp*>(h_hyps_b);
    const int nb = bad ? 0 : (int)bm.size();
    std::vector<double> fin(nb), lms(nb);
    for (int r = 0; r < nb; ++r) {
      const double fused = bm[r].tot + bm[r].bonus;
      fin[r] = fused; lms[r] = S.n_sum[bm[r].node];
      if (eos) {
        int st;
        const double lp = ngram_lp(lv, S.n_state[bm[r].node], lv.eos, &st);
        fin[r] = ngram_finish(fused, lw, lp); lms[r] += lp;
      }
    }
    for (int k = nb; k < nbest; ++k) {
      ss_ctc_beam_lm_hyp& h = h_hyps[k];
      h.score = h.ctc_score = bad ? (double)__builtin_nanf("") : -INFINITY; h.lm_score = 0.0; h.n_tokens = 0; h.status = bad ? 2 : 1;
    }
    for (int r = 0; r < nb; ++r) {
      int rank = 0;
      for (int f = 0; f < nb; ++f) rank += ctc_beam_before(fin[f], f, fin[r], r);
      if (rank >= nbest) continue;
      ss_ctc_beam_lm_hyp& h = h_hyps[rank];
      int len = 0;
      for (int n = bm[r].node; n > 0; n = par[n]) ++len;
      int32_t* out = h_tokens_b + (size_t)rank * out_stride;
      int j = len;
      for (int n = bm[r].node; n > 0; n = par[n]) out[--j] = tok[n];
      h.score = fin[r]; h.ctc_score = bm[r].tot; h.lm_score = lms[r]; h.n_tokens = len; h.status = 0;
    }
  }
}

// The stable-prefix pass of the resumable kernel: the smallest depth of the lowest common ancestor of a beam prefix and prefix 0.
static CtcStreamPart ctc_beam_host_part(const CtcBeamHostState& S) {
  const int nb = S.bad ? 0 : (int)S.bm.size();
  int stable = nb > 0 ? NONE : 0;
  for (int r = 0; r < nb; ++r) {
    int a = S.bm[r].node, b = S.bm[0].node, da = 0, db = 0;
    for (int n = a; n > 0; n = S.par[n]) ++da;
    for (int n = b; n > 0; n = S.par[n]) ++db;
    for (; da > db; --da) a = S.par[a];
    for (; db > da; --db) b = S.par[b];
    for (; a != b; --da) { a = S.par[a]; b = S.par[b]; }
    if (da < stable) stable = da;
  }
  return CtcStreamPart{S.frames, stable, nb, S.bad ? 2 : 0};
}

}  // namespace ss

template <bool LM>
static int ctc_beam_host_any(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                             int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* o, void* h_hyps_out, int32_t* h_tokens,
                             int out_stride, float* h_den, int32_t* h_cand_id) {
  if (!h_logits || ld < V || !h_hyps_out || !h_tokens) return SS_ERR_ARG;
  CtcBeamPlan p;
  const int rc = ctc_beam_plan(V, B, h_T, beam, cand, nbest, out_stride, p, g_host_max_beam);
  if (rc != SS_OK) return rc;
  NgramView lv{};
  double lw = 0.0, ws = 0.0;
  if constexpr (LM) {
    RET(ctc_beam_lm_check(lm, V, o));
    lv = lm->host.view(); lw = o->lm_weight; ws = o->word_score;
  }
  const size_t rec = LM ? sizeof(ss_ctc_beam_lm_hyp) : sizeof(ss_ctc_beam_hyp);
  CtcBeamHostState S;
  for (int b = 0; b < B; ++b) {
    const CtcBeamSeg& sg = p.segs[b];
    S.start(beam, sg.T, LM, lv.start);
    ctc_beam_host_frames<LM>(S, h_logits + (size_t)sg.row0 * ld, ld, V, pad, unk, sg.T, beam, cand, lv, lw, ws,
                             h_den ? h_den + 2 * (size_t)sg.row0 : nullptr, h_cand_id ? h_cand_id + (size_t)sg.row0 * cand : nullptr);
    ctc_beam_host_emit<LM>(S, nbest, LM && o->eos_term, lv, lw, static_cast<unsigned char*>(h_hyps_out) + (size_t)b * nbest * rec,
                           h_tokens + (size_t)b * nbest * out_stride, out_stride);
  }
  return SS_OK;
}

// The resumable twin: every pointer a HOST pointer, h_logits the stacked new rows (session i's upto - f rows behind those of the
// sessions before it).  The checks are the caller's (ss_ctc_stream_advance_host, ctc_stream.hip).
namespace ss {
int ctc_stream_host_run(std::vector<CtcBeamHostState>& slots, const float* h_logits, int ld, int V, int pad, int unk, int n,
                        const CtcStreamSess* sess, int beam, int cand, int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* o,
                        void* h_hyps, int32_t* h_tokens, int out_stride, CtcStreamPart* h_part) {
  NgramView lv{};
  double lw = 0.0, ws = 0.0;
  if (lm) { lv = lm->host.view(); lw = o->lm_weight; ws = o->word_score; }
  const size_t rec = lm ? sizeof(ss_ctc_beam_lm_hyp) : sizeof(ss_ctc_beam_hyp);
  for (int i = 0; i < n; ++i) {
    const CtcStreamSess& se = sess[i];
    CtcBeamHostState& S = slots[se.slot];
    const float* rows = h_logits + (size_t)se.row0 * ld;
    unsigned char* hy = static_cast<unsigned char*>(h_hyps) + (size_t)i * nbest * rec;
    int32_t* tk = h_tokens + (size_t)i * nbest * out_stride;
    if (lm) {
      ctc_beam_host_frames<true>(S, rows, ld, V, pad, unk, se.upto - se.f, beam, cand, lv, lw, ws, nullptr, nullptr);
      ctc_beam_host_emit<true>(S, nbest, se.fin && o->eos_term, lv, lw, hy, tk, out_stride);
    } else {
      ctc_beam_host_frames<false>(S, rows, ld, V, pad, unk, se.upto - se.f, beam, cand, lv, lw, ws, nullptr, nullptr);
      ctc_beam_host_emit<false>(S, nbest, false, lv, lw, hy, tk, out_stride);
    }
    h_part[i] = ctc_beam_host_part(S);
  }
  return SS_OK;
}
}  // namespace ss

extern "C" int ss_ctc_beam_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                                int nbest, ss_ctc_beam_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den,
                                int32_t* h_cand_id) {
  return ctc_beam_host_any<false>(h_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, nullptr, nullptr, h_hyps, h_tokens, out_stride,
                                  h_den, h_cand_id);
}

extern "C" int ss_ctc_beam_lm_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                                   int nbest, ss_ctc_beam_lm_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den,
                                   int32_t* h_cand_id, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts) {
  return ctc_beam_host_any<true>(h_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, lm, opts, h_hyps, h_tokens, out_stride, h_den,
                                 h_cand_id);
}
