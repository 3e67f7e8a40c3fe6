// The step kernels of the beam search (beam.hip tells how the search uses them), their launchers and their op-level entry points:
//   beam_topk_kernel   one workgroup per hypothesis row: log-softmax of the logits, the reference's masks, + cumulative score, the
//                      row's 2k best candidates (the global top 2k over beam x vocab is inside the union of the per-row lists)
//   beam_merge_kernel  one workgroup per utterance: the global top 2k in the reference's order (score, then flattened index), the
//                      finalisation into the utterance's table, the active hypotheses, next tokens / scores / ancestry, done flag
//   beam_prefix_score_kernel   one workgroup per forced row: log-softmax value of the forced token, masks as above
//   beam_prefix_chain_kernel   one thread per utterance: the cumulative scores as an in-order float32 chain, and their differences
// The option and constraint variants are instantiations of the same bodies; the launcher of a family picks one from the arguments,
// and with every option at its default that is the plain kernel, the `false` instantiation.
#include <cmath>

#include "beam_rows.hpp"

using namespace ss;

namespace {

// a beats b: higher score, then lower flattened index (torch.topk order); index < 0 = no candidate
__device__ __forceinline__ bool beats(float a, int ia, float b, int ib) {
  return ib < 0 || (ia >= 0 && (a > b || (a == b && ia < ib)));
}

// Row r = b*k + j of the logits -> its 2k best (score, token), score = masked log-softmax + cumulative score of the hypothesis
// (the row phase: beam_rows.hpp).  Lock-step index t; the reference's step of utterance b is npre[b] + t.
//
// OPT (ss_mt_search_opts; the plain search instantiates OPT = false, which is the code it always was): the logits are divided by the
// temperature wherever they are read, and with ngram >= 2 the no-repeat ban is a phase of this kernel, read by the mask chain right
// after min_len.
// CONS (ss_batch_mt_beam_cons; no prefix, so step == t_step): at step > 0 </s> of a row whose constraint state is not finished is
// -inf, after every other mask and before the cumulative score; the scores of the row's next tokens go to ca.next_s as the row is
// filled, before the extraction loop overwrites taken entries.
template <bool OPT, bool CONS = false>
__device__ __forceinline__ void beam_topk_body(const float* __restrict__ logits, int V, int k, int t_step, int min_len,
                                               const int* __restrict__ max_len, const int* __restrict__ npre,
                                               const int* __restrict__ done,
                                               const float* __restrict__ cum, int pad, int unk, int eos, float unk_pen,
                                               float* __restrict__ cand_s, int* __restrict__ cand_t, const TopkOpts& o,
                                               const ConsArgs& ca = ConsArgs{}) {
  extern __shared__ float vals[];                  // [V] candidate scores of the row; NaN = already taken
  __shared__ float sa[4];
  __shared__ int si[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x, b = row / k, j = row - b * k;
  if (done[b] || (t_step == 0 && j != 0)) return;  // first free step: only beam 0 of each utterance takes part (lprobs[:, ::beam])
  const int step = t_step + npre[b];
  const float* r = logits + (size_t)row * V;
  auto logit = [&](int n) -> float {
    if constexpr (OPT) return r[n] / o.temp; else return r[n];
  };
  RowMask m{pad, unk, eos, unk_pen};
  if (OPT && o.ngram >= 2) m.banned = row_ban_map(o, vals, V, row, b, step, npre[b]);
  const float mx = row_max_sums(logit, V, sa);
  const float lse = row_lse(sa);
  m.at_max = step >= max_len[b]; m.below_min = step < min_len;
  m.add_cum = step > 0; m.cum = cum[row];
  [[maybe_unused]] int nt0 = -1, nt1 = -1;
  if constexpr (CONS) {
    const ConsRow cr = cons_row(ca.tab, b);
    const int cs = cons_clamp_state(cr, ca.state[row]);
    m.ban_eos = step > 0 && cs + 1 != cr.C;
    cons_next_tokens(cr, cs, nt0, nt1);
    if (t == 0) {
      ca.next_t[2 * row] = nt0; ca.next_t[2 * row + 1] = nt1;
      if ((unsigned)nt0 >= (unsigned)V) ca.next_s[2 * row] = -INFINITY;
      if ((unsigned)nt1 >= (unsigned)V) ca.next_s[2 * row + 1] = -INFINITY;
    }
  }
  float best = 0.f;
  int bi = -1;
  for (int n = t; n < V; n += 256) {
    const float v = row_masked_lprob(logit, n, mx, lse, m);
    if (OPT && o.row_scores) o.row_scores[(size_t)row * V + n] = v;
    vals[n] = v;
    if constexpr (CONS) {
      if (n == nt0) ca.next_s[2 * row] = v;
      if (n == nt1) ca.next_s[2 * row + 1] = v;
    }
    if (beats(v, n, best, bi)) { best = v; bi = n; }
  }
  const int nc = min(2 * k, V - 1);
  for (int q = 0; q < nc; ++q) {
    float wb = best;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(wb, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (beats(ob, oi, wb, wi)) { wb = ob; wi = oi; }
    }
    __syncthreads();                               // the previous round's readers of sa / si are done
    if (lane == 0) { sa[wave] = wb; si[wave] = wi; }
    __syncthreads();
    wb = sa[0]; wi = si[0];
    for (int w = 1; w < 4; ++w)
      if (beats(sa[w], si[w], wb, wi)) { wb = sa[w]; wi = si[w]; }
    if (t == 0) { cand_s[(size_t)row * kMaxCand + q] = wb; cand_t[(size_t)row * kMaxCand + q] = wi; }
    if (wi >= 0 && (wi & 255) == t) {              // the owner drops the winner and rescans its columns
      vals[wi] = __int_as_float(0x7fc00000);
      best = 0.f; bi = -1;
      for (int n = t; n < V; n += 256) {
        const float v = vals[n];
        if (v == v && beats(v, n, best, bi)) { best = v; bi = n; }
      }
    }
  }
}

__global__ __launch_bounds__(256) void beam_topk_kernel(const float* __restrict__ logits, int V, int k, int t_step, int min_len,
                                                        const int* __restrict__ max_len, const int* __restrict__ npre,
                                                        const int* __restrict__ done,
                                                        const float* __restrict__ cum, int pad, int unk, int eos, float unk_pen,
                                                        float* __restrict__ cand_s, int* __restrict__ cand_t) {
  beam_topk_body<false>(logits, V, k, t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen, cand_s, cand_t, TopkOpts{});
}

__global__ __launch_bounds__(256) void beam_topk_opts_kernel(const float* __restrict__ logits, int V, int k, int t_step, int min_len,
                                                             const int* __restrict__ max_len, const int* __restrict__ npre,
                                                             const int* __restrict__ done,
                                                             const float* __restrict__ cum, int pad, int unk, int eos,
                                                             float unk_pen, float* __restrict__ cand_s, int* __restrict__ cand_t,
                                                             TopkOpts o) {
  beam_topk_body<true>(logits, V, k, t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen, cand_s, cand_t, o);
}

__global__ __launch_bounds__(256) void beam_topk_cons_kernel(const float* __restrict__ logits, int V, int k, int t_step, int min_len,
                                                             const int* __restrict__ max_len, const int* __restrict__ npre,
                                                             const int* __restrict__ done,
                                                             const float* __restrict__ cum, int pad, int unk, int eos,
                                                             float unk_pen, float* __restrict__ cand_s, int* __restrict__ cand_t,
                                                             TopkOpts o, ConsArgs ca) {
  beam_topk_body<true, true>(logits, V, k, t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen, cand_s, cand_t, o, ca);
}

// The rank merge of both merge kernels: the nl sorted lists of nc entries from row r0 on -> sel_* [nc], the global top nc in order.
__device__ __forceinline__ void beam_rank_merge(const float* __restrict__ cand_s, const int* __restrict__ cand_t, int r0, int nl,
                                                int nc, float* sel_s, int* sel_t, int* sel_beam) {
  __shared__ float ms[kMaxBeam * kMaxCand];
  __shared__ int mt[kMaxBeam * kMaxCand];
  const int t = threadIdx.x;
  for (int i = t; i < nl * nc; i += 256) {
    const int l = i / nc, q = i - l * nc;
    ms[i] = cand_s[(size_t)(r0 + l) * kMaxCand + q];
    mt[i] = cand_t[(size_t)(r0 + l) * kMaxCand + q];
  }
  __syncthreads();
  // rank of candidate (list l, position q) = q + the entries of the other lists that beat it; lists are sorted, so each count is a
  // binary search.  A list below l wins ties (lower flattened index), a list above loses them.
  for (int i = t; i < nl * nc; i += 256) {
    const int l = i / nc, q = i - l * nc;
    const float x = ms[i];
    int rank = q;
    for (int l2 = 0; l2 < nl && rank < nc; ++l2) {
      if (l2 == l) continue;
      const float* L = ms + l2 * nc;
      int lo = 0, hi = nc;                         // count of entries e with (l2 < l ? e >= x : e > x)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l2 < l ? L[mid] >= x : L[mid] > x) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < nc) { sel_s[rank] = x; sel_t[rank] = mt[i]; sel_beam[rank] = l; }
  }
  __syncthreads();
}

// Steps 2 - 8 of the constraint rule for utterance b, by the whole workgroup: sel_* [2k] hold the global top 2k (step 2a) on
// entry and the step's selection on return, sel_st [2k] its new states.  One thread per candidate (at most kConsCand = 160): the
// sort, the de-duplication and the stripes are counts over the list in LDS, so every order is decided by comparisons alone.
__device__ __forceinline__ void cons_select(const ConsArgs& ca, const float* __restrict__ cand_s, const int* __restrict__ cand_t,
                                            int b, int k, int t_step, float* sel_s, int* sel_t, int* sel_beam, int* sel_st) {
  __shared__ float c_s[kConsCand], c_key[kConsCand];
  __shared__ int c_t[kConsCand], c_b[kConsCand], c_st[kConsCand], c_rank[kConsCand], c_ib[kConsCand];
  const int t = threadIdx.x, r0 = b * k, nc = 2 * k;
  const ConsRow cr = cons_row(ca.tab, b);
  const int nrow = t_step == 0 ? 1 : k, n1 = nc + (t_step > 0 ? k : 0), N = n1 + 2 * nrow;
  float s = 0.f, key = 0.f;
  int tk = -1, bm = 0, ns = -1;                     // tk < 0: an empty slot of the list
  if (t < N) {
    if (t < nc) { s = sel_s[t]; tk = sel_t[t]; bm = sel_beam[t]; }
    else if (t < n1) { bm = t - nc; s = cand_s[(size_t)(r0 + bm) * kMaxCand]; tk = cand_t[(size_t)(r0 + bm) * kMaxCand]; }
    else { const int i = t - n1; bm = i >> 1; s = ca.next_s[2 * (r0 + bm) + (i & 1)]; tk = ca.next_t[2 * (r0 + bm) + (i & 1)]; }
    if (tk >= 0) {
      ns = cons_advance(cr, cons_clamp_state(cr, ca.state[r0 + bm]), tk);
      key = cons_key(cr, ns, s);
    }
    c_s[t] = s; c_key[t] = key; c_t[t] = tk; c_b[t] = bm; c_st[t] = ns;
  }
  __syncthreads();
  int rank = 0;
  if (t < N && tk >= 0)                             // key descending, ties by list position
    for (int j = 0; j < N; ++j)
      if (c_t[j] >= 0 && (c_key[j] > key || (c_key[j] == key && j < t))) ++rank;
  if (t < N) c_rank[t] = rank;
  __syncthreads();
  bool keep = t < N && tk >= 0;
  if (keep)                                         // the same (beam, token) earlier in the order
    for (int j = 0; j < N; ++j)
      if (c_t[j] == tk && c_b[j] == bm && c_rank[j] < rank) { keep = false; break; }
  __syncthreads();                                  // c_t is read above and rewritten below
  if (t < N && !keep) c_t[t] = -1;
  __syncthreads();
  int ib = 0;
  if (keep)                                         // rank within the own bank (equal state = equal bank)
    for (int j = 0; j < N; ++j)
      if (c_t[j] >= 0 && c_st[j] == ns && c_rank[j] < rank) ++ib;
  if (t < N) c_ib[t] = ib;
  __syncthreads();
  if (keep) {
    int pos = 0;                                    // (rank within bank, then higher bank first); the pairs are distinct
    for (int j = 0; j < N; ++j)
      if (c_t[j] >= 0 && (c_ib[j] < ib || (c_ib[j] == ib && c_st[j] > ns))) ++pos;
    if (pos < nc) { sel_s[pos] = s; sel_t[pos] = tk; sel_beam[pos] = bm; sel_st[pos] = ns; }
  }
  __syncthreads();
}

// An utterance that is finished, before this step or by it: its k rows keep decoding (lockstep) -- keep their tables valid, nothing
// else.  Every slot stays its own ancestor and feeds </s> with score 0.
__device__ __forceinline__ void beam_idle_tables(const int* anc_cur, int* anc_nxt, int* tok_nxt, float* cum_nxt, int r0, int k,
                                                 int Lc, int ci, int eos) {
  const int t = threadIdx.x, na = ci + 2;
  for (int i = t; i < k * na; i += 256) {
    const int j = i / na, p = i - j * na;
    anc_nxt[(size_t)(r0 + j) * Lc + p] = p <= ci ? anc_cur[(size_t)(r0 + j) * Lc + p] : r0 + j;
  }
  if (t < k) { tok_nxt[r0 + t] = eos; cum_nxt[r0 + t] = 0.f; }
}

// One workgroup per utterance: merge the k sorted per-row lists into the global top 2k, then the step logic of
// unity/sequence_generator.py:329-470 and finalize_hypos.  t_step is the lock-step index (reference step npre[b] + t_step); every
// slot wrote cache index c0 + t_step at this step, so the ancestry entries in use are the cache indices 0 .. c0 + t_step.
// LENPEN (ss_mt_search_opts::len_penalty != 1): a finalised score is divided by (step + 1) ** len_penalty, formed as the reference forms
// it -- the power in double, rounded to float32, then one float32 division.  The plain search instantiates LENPEN = false.
template <bool LENPEN, bool CONS = false>
__device__ __forceinline__ void beam_merge_body(const BeamState& st, int k, int R, int Lc, int V, int t_step, int c0, int eos,
                                                int normalize, float len_penalty, const ConsArgs& ca = ConsArgs{}) {
  __shared__ float sel_s[kMaxCand];
  __shared__ int sel_t[kMaxCand], sel_beam[kMaxCand];
  [[maybe_unused]] __shared__ int sel_st[CONS ? kMaxCand : 1];
  __shared__ int fin_c[kMaxBeam], fin_e[kMaxBeam], act_c[kMaxBeam];
  __shared__ int eosm[kMaxCand], f[kMaxBeam];
  __shared__ int n_fin, is_done;
  const int t = threadIdx.x, b = blockIdx.x, r0 = b * k;
  const int npre = st.npre[b], step = t_step + npre;   // the reference's step
  const int ci = c0 + t_step, na = ci + 2;             // cache index written at this step; ancestry entries the next step reads
  const int* anc_cur = st.anc + (size_t)(t_step & 1) * R * Lc;
  int* anc_nxt = st.anc + (size_t)((t_step + 1) & 1) * R * Lc;
  int* tok_nxt = st.tok + (size_t)(t_step + 1) * R;
  float* cum_nxt = st.cum + (size_t)(t_step + 1) * R;
  if (st.done[b]) { beam_idle_tables(anc_cur, anc_nxt, tok_nxt, cum_nxt, r0, k, Lc, ci, eos); return; }
  const int nl = t_step == 0 ? 1 : k, nc = 2 * k;
  beam_rank_merge(st.cand_s, st.cand_t, r0, nl, nc, sel_s, sel_t, sel_beam);
  if constexpr (CONS) cons_select(ca, st.cand_s, st.cand_t, b, k, t_step, sel_s, sel_t, sel_beam, sel_st);
  if (t == 0) {
    // finalisation: </s> candidates among the first k, finite, not ignored (unity/sequence_generator.py:345-372)
    for (int q = 0; q < nc; ++q) {
      eosm[q] = sel_t[q] == eos && sel_s[q] != -INFINITY;
      if (q < k && st.ignore[r0 + q]) eosm[q] = 0;
    }
    int cnt = st.fin_cnt[b], nf = 0;
    for (int q = 0; q < k; ++q)
      if (eosm[q] && cnt < k) {
        fin_c[nf] = q; fin_e[nf] = cnt; ++nf; ++cnt;
        if constexpr (LENPEN)
          st.fin_score[b * k + cnt - 1] = normalize ? sel_s[q] / (float)pow((double)(step + 1), (double)len_penalty) : sel_s[q];
        else
          st.fin_score[b * k + cnt - 1] = normalize ? sel_s[q] / (float)(step + 1) : sel_s[q];   // the full length, prefix included
        st.fin_len[b * k + cnt - 1] = t_step + 1;                                              // tokens after the prefix
      }
    bool any = false;
    for (int q = 0; q < k; ++q) any = any || eosm[q];
    st.fin_cnt[b] = cnt;
    n_fin = nf;
    const int dn = (any && (cnt == k || step == st.max_len[b])) || step >= st.max_len[b];   // is_finished (sequence_generator.py:762)
    is_done = dn;
    st.done[b] = dn;
    // active hypotheses: the first k candidates that are neither </s> nor ignored, then the others in order (topk of active_mask)
    int nact = 0;
    for (int q = 0; q < nc && nact < k; ++q)
      if (!(q < k ? (st.ignore[r0 + q] || eosm[q]) : eosm[q])) act_c[nact++] = q;
    for (int q = 0; q < nact; ++q) f[q] = 0;
    for (int q = 0; q < nc && nact < k; ++q)
      if (q < k ? (st.ignore[r0 + q] || eosm[q]) : eosm[q]) { f[nact] = 1; act_c[nact++] = q; }
    if (!dn)
      for (int q = 0; q < k; ++q) st.ignore[r0 + q] = f[q];
  }
  __syncthreads();
  // finalised entries: the tokens generated so far and </s>, positional scores (differences of the cumulative score; the first one
  // against the prefix' cumulative score when there is a prefix), ancestry snapshot
  for (int e = 0; e < n_fin; ++e) {
    const int q = fin_c[e], slot = fin_e[e], pr = r0 + sel_beam[q];
    const int* a = anc_cur + (size_t)pr * Lc;
    const size_t o = ((size_t)b * k + slot) * Lc;
    for (int p = t; p <= ci; p += 256) st.fin_anc[o + p] = a[p];
    for (int u = t; u <= t_step; u += 256) {
      st.fin_tok[o + u] = u < t_step ? st.tok[(size_t)(u + 1) * R + a[c0 + u + 1]] : eos;
      const float cur = u < t_step ? st.cum[(size_t)(u + 1) * R + a[c0 + u + 1]] : sel_s[q];
      const float prv = u + npre > 0 ? st.cum[(size_t)u * R + a[c0 + u]] : 0.f;
      st.fin_pos[o + u] = u + npre > 0 ? cur - prv : cur;
    }
  }
  if (is_done) { beam_idle_tables(anc_cur, anc_nxt, tok_nxt, cum_nxt, r0, k, Lc, ci, eos); return; }
  // next hypotheses: slot j continues candidate act_c[j] -- its ancestry is its parent's plus itself at the next cache index
  if (t < k) {
    const int q = act_c[t];
    tok_nxt[r0 + t] = sel_t[q];
    cum_nxt[r0 + t] = sel_s[q];
    if constexpr (CONS) ca.state_nxt[r0 + t] = sel_st[q];   // update_constraints(active_hypos)
  }
  for (int i = t; i < k * na; i += 256) {
    const int j = i / na, p = i - j * na;
    const int pr = r0 + sel_beam[act_c[j]];
    anc_nxt[(size_t)(r0 + j) * Lc + p] = p <= ci ? anc_cur[(size_t)pr * Lc + p] : r0 + j;
  }
}

__global__ __launch_bounds__(256) void beam_merge_kernel(BeamState st, int k, int R, int Lc, int V, int t_step, int c0, int eos,
                                                         int normalize) {
  beam_merge_body<false>(st, k, R, Lc, V, t_step, c0, eos, normalize, 1.f);
}

__global__ __launch_bounds__(256) void beam_merge_lenpen_kernel(BeamState st, int k, int R, int Lc, int V, int t_step, int c0, int eos,
                                                                int normalize, float len_penalty) {
  beam_merge_body<true>(st, k, R, Lc, V, t_step, c0, eos, normalize, len_penalty);
}

__global__ __launch_bounds__(256) void beam_merge_cons_kernel(BeamState st, int k, int R, int Lc, int V, int t_step, int c0, int eos,
                                                              int normalize, ConsArgs ca) {
  beam_merge_body<false, true>(st, k, R, Lc, V, t_step, c0, eos, normalize, 1.f, ca);
}

__global__ __launch_bounds__(256) void beam_merge_cons_lenpen_kernel(BeamState st, int k, int R, int Lc, int V, int t_step, int c0,
                                                                     int eos, int normalize, float len_penalty, ConsArgs ca) {
  beam_merge_body<true, true>(st, k, R, Lc, V, t_step, c0, eos, normalize, len_penalty, ca);
}

// The selection stage alone (ss_op_beam_cons_select): the rank merge and cons_select of beam_merge_cons_kernel, then the selection
// written out, row stride kMaxCand.
__global__ __launch_bounds__(256) void beam_cons_select_kernel(const float* __restrict__ cand_s, const int* __restrict__ cand_t,
                                                               ConsArgs ca, int k, int t_step, float* __restrict__ out_s,
                                                               int* __restrict__ out_t, int* __restrict__ out_beam,
                                                               int* __restrict__ out_state) {
  __shared__ float sel_s[kMaxCand];
  __shared__ int sel_t[kMaxCand], sel_beam[kMaxCand], sel_st[kMaxCand];
  const int t = threadIdx.x, b = blockIdx.x, nc = 2 * k;
  beam_rank_merge(cand_s, cand_t, b * k, t_step == 0 ? 1 : k, nc, sel_s, sel_t, sel_beam);
  cons_select(ca, cand_s, cand_t, b, k, t_step, sel_s, sel_t, sel_beam, sel_st);
  if (t < nc) {
    const size_t o = (size_t)b * kMaxCand + t;
    out_s[o] = sel_s[t]; out_t[o] = sel_t[t]; out_beam[o] = sel_beam[t]; out_state[o] = sel_st[t];
  }
}

// Forced prefix rows: row i of the prefix pass' logits -> lp[i] = the masked log-softmax value of the token forced there (ftok[i];
// < 0: the row forces nothing).  The reference masks before it forces (unity/sequence_generator.py:290-327, then _prefix_tokens):
// NaN -> -inf, pad -inf, unk -= unk_penalty; a forced step is below max_len, and min_len is not applied at it.
// TEMP: the logits are divided by the temperature wherever they are read; the plain search instantiates TEMP = false.
template <bool TEMP>
__device__ __forceinline__ void beam_prefix_score_body(const float* __restrict__ logits, int V, const int* __restrict__ ftok, int pad,
                                                       int unk, float unk_pen, float* __restrict__ lp, float temp) {
  __shared__ float sa[4];
  const int row = blockIdx.x, tk = ftok[row];
  if (tk < 0 || tk >= V) return;
  const float* r = logits + (size_t)row * V;
  auto logit = [&](int n) -> float {
    if constexpr (TEMP) return r[n] / temp; else return r[n];
  };
  const float mx = row_max_sums(logit, V, sa);
  if (threadIdx.x != 0) return;
  lp[row] = row_masked_lprob(logit, tk, mx, row_lse(sa), RowMask{pad, unk, -1, unk_pen});
}

__global__ __launch_bounds__(256) void beam_prefix_score_kernel(const float* __restrict__ logits, int V, const int* __restrict__ ftok,
                                                                int pad, int unk, float unk_pen, float* __restrict__ lp) {
  beam_prefix_score_body<false>(logits, V, ftok, pad, unk, unk_pen, lp, 1.f);
}

__global__ __launch_bounds__(256) void beam_prefix_score_temp_kernel(const float* __restrict__ logits, int V,
                                                                     const int* __restrict__ ftok, int pad, int unk, float unk_pen,
                                                                     float* __restrict__ lp, float temp) {
  beam_prefix_score_body<true>(logits, V, ftok, pad, unk, unk_pen, lp, temp);
}

// Per utterance the cumulative score of its forced tokens as the reference forms it (lprobs + scores[:, step - 1], step by step in
// float32): cum_p = lp_p + cum_{p-1}.  pos[row0 + p] = cum_p - cum_{p-1}, the positional score finalize_hypos derives; the last sum
// becomes the cumulative score hypothesis 0 enters the first free step with (cum0[b * k]).
__global__ __launch_bounds__(256) void beam_prefix_chain_kernel(const float* __restrict__ lp, const int* __restrict__ row0,
                                                                const int* __restrict__ npre, int B, int k, float* __restrict__ cum0,
                                                                float* __restrict__ pos) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int n = npre[b], r = row0[b];
  float c = 0.f;
  for (int p = 0; p < n; ++p) {
    const float nc = p > 0 ? lp[r + p] + c : lp[r + p];
    pos[r + p] = p > 0 ? nc - c : nc;
    c = nc;
  }
  if (n > 0) cum0[(size_t)b * k] = c;
}

}  // namespace

// ---- the launchers: the one place each kernel is launched from ----
namespace ss {

// the plain top-2k kernel serves: no constraints, every option at its default, no row scores asked for
static bool topk_plain(const TopkOpts& o, const ConsArgs* ca) { return !ca && o.ngram < 2 && o.temp == 1.f && !o.row_scores; }

int beam_topk_lds(int V, const TopkOpts& o, const ConsArgs* ca, size_t& bytes) {
  bytes = topk_lds_bytes(V, o.ngram, o.Lc);
  return !topk_plain(o, ca) && bytes > 65536 ? SS_ERR_ARG : SS_OK;   // the plain row is the vocabulary limit of the callers
}

int launch_beam_topk(hipStream_t s, int R, const RowStep& a, float* cand_s, int* cand_t, const TopkOpts& o, const ConsArgs* ca) {
  size_t lds;
  RET(beam_topk_lds(a.V, o, ca, lds));
  auto go = [&](auto kernel, auto... more) {   // `more`: the variant's trailing kernel arguments, in the kernel's order (o, then ca)
    hipLaunchKernelGGL(kernel, dim3(R), dim3(256), lds, s, a.logits, a.V, a.k, a.t_step, a.min_len, a.max_len, a.npre, a.done, a.cum,
                       a.pad, a.unk, a.eos, a.unk_pen, cand_s, cand_t, more...);
  };
  if (ca) go(beam_topk_cons_kernel, o, *ca);
  else if (!topk_plain(o, ca)) go(beam_topk_opts_kernel, o);
  else go(beam_topk_kernel);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_beam_merge(hipStream_t s, int B, const BeamState& st, int k, int Lc, int V, int t_step, int c0, int eos, int normalize,
                      float len_penalty, const ConsArgs* ca) {
  const bool lenpen = normalize && len_penalty != 1.f;      // a score that is not normalised takes no penalty
  auto go = [&](auto kernel, auto... more) {   // `more`: the variant's trailing kernel arguments, in the kernel's order (len_penalty, then ca)
    hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, s, st, k, B * k, Lc, V, t_step, c0, eos, normalize ? 1 : 0, more...);
  };
  if (ca && lenpen) go(beam_merge_cons_lenpen_kernel, len_penalty, *ca);
  else if (ca) go(beam_merge_cons_kernel, *ca);
  else if (lenpen) go(beam_merge_lenpen_kernel, len_penalty);
  else go(beam_merge_kernel);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_beam_prefix_score(hipStream_t s, int rows, const float* logits, int V, const int* ftok, int pad, int unk, float unk_pen,
                             float* lp, float temp) {
  if (rows <= 0 || V <= 0) return SS_ERR_ARG;
  if (temp != 1.f)
    hipLaunchKernelGGL(beam_prefix_score_temp_kernel, dim3(rows), dim3(256), 0, s, logits, V, ftok, pad, unk, unk_pen, lp, temp);
  else hipLaunchKernelGGL(beam_prefix_score_kernel, dim3(rows), dim3(256), 0, s, logits, V, ftok, pad, unk, unk_pen, lp);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_beam_prefix_chain(hipStream_t s, const float* lp, const int* row0, const int* npre, int B, int k, float* cum0, float* pos) {
  hipLaunchKernelGGL(beam_prefix_chain_kernel, dim3((B + 255) / 256), dim3(256), 0, s, lp, row0, npre, B, k, cum0, pos);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss

// ---- op-level entry points of the kernels above (include/streamspeech_hip.h; tests/test_glue_ops_gpu.py), and of their option
// variants (ss_mt_search_opts; tests/test_search_options_gpu.py) ----
extern "C" int ss_op_beam_topk_opts(void* stream, const float* logits, int R, int V, int k, int t_step, int min_len,
                                    const int32_t* max_len, const int32_t* npre, const int32_t* done, const float* cum, int pad, int unk,
                                    int eos, float unk_pen, float* cand_s, int32_t* cand_t, float temperature, int no_repeat_ngram,
                                    const int32_t* tok, const int32_t* anc, int Lc, int c0, const int32_t* ptok, const int32_t* row0,
                                    float* row_scores) {
  const ss_mt_search_opts o{(int32_t)sizeof(ss_mt_search_opts), no_repeat_ngram, 1.f, temperature};
  SearchOpts so;
  RET(read_search_opts(&o, so));
  if (R <= 0 || k < 1 || k > kMaxBeam || R % k != 0) return SS_ERR_ARG;                   // the search's own limits (beam_continue_plan)
  if (V < 2 * k + 1 || (size_t)V * sizeof(float) > 65536) return SS_ERR_ARG;
  TopkOpts to = topk_opts(so, R, Lc, c0, tok, anc, ptok, row0);
  to.row_scores = row_scores;
  if (!topk_plain(to, nullptr) && t_step < 0) return SS_ERR_ARG;   // ss_op_beam_topk has never refused it
  if (so.ngram >= 2 && (!tok || !anc || c0 < 0 || c0 + t_step >= Lc)) return SS_ERR_ARG;
  const RowStep a{logits, V, k, t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen};
  return launch_beam_topk((hipStream_t)stream, R, a, cand_s, cand_t, to, nullptr);
}

extern "C" int ss_op_beam_topk(void* stream, const float* logits, int R, int V, int k, int t_step, int min_len, const int32_t* max_len,
                               const int32_t* npre, const int32_t* done, const float* cum, int pad, int unk, int eos, float unk_pen,
                               float* cand_s, int32_t* cand_t) {
  return ss_op_beam_topk_opts(stream, logits, R, V, k, t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen, cand_s, cand_t,
                              1.f, 0, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr);
}

extern "C" int ss_op_beam_merge_opts(void* stream, const ss_op_beam_state* x, int B, int k, int Lc, int V, int t_step, int c0, int eos,
                                     int normalize, float len_penalty) {
  if (!std::isfinite(len_penalty)) return SS_ERR_ARG;
  if (!x || B <= 0 || k < 1 || k > kMaxBeam || t_step < 0 || c0 < 0 || c0 + t_step + 2 > Lc) return SS_ERR_ARG;
  const BeamState st{x->tok, x->cum, x->anc, x->cand_s, x->cand_t, x->ignore, x->done, x->max_len, x->npre,
                     x->fin_cnt, x->fin_score, x->fin_len, x->fin_tok, x->fin_pos, x->fin_anc};   // field for field
  return launch_beam_merge((hipStream_t)stream, B, st, k, Lc, V, t_step, c0, eos, normalize, len_penalty, nullptr);
}

extern "C" int ss_op_beam_merge(void* stream, const ss_op_beam_state* x, int B, int k, int Lc, int V, int t_step, int c0, int eos,
                                int normalize) {
  return ss_op_beam_merge_opts(stream, x, B, k, Lc, V, t_step, c0, eos, normalize, 1.f);
}

extern "C" int ss_op_beam_prefix_score_opts(void* stream, const float* logits, int rows, int V, const int32_t* ftok, int pad, int unk,
                                            float unk_pen, float* lp, float temperature) {
  if (!std::isfinite(temperature) || !(temperature > 0.f)) return SS_ERR_ARG;
  return launch_beam_prefix_score((hipStream_t)stream, rows, logits, V, ftok, pad, unk, unk_pen, lp, temperature);
}

extern "C" int ss_op_beam_prefix_score(void* stream, const float* logits, int rows, int V, const int32_t* ftok, int pad, int unk,
                                       float unk_pen, float* lp) {
  return ss_op_beam_prefix_score_opts(stream, logits, rows, V, ftok, pad, unk, unk_pen, lp, 1.f);
}

extern "C" int ss_op_beam_prefix_chain(void* stream, const float* lp, const int32_t* row0, const int32_t* npre, int B, int k,
                                       float* cum0, float* pos) {
  if (B <= 0 || k < 1) return SS_ERR_ARG;
  return launch_beam_prefix_chain((hipStream_t)stream, lp, row0, npre, B, k, cum0, pos);
}

extern "C" int ss_op_beam_cons_select(void* stream, const float* cand_s, const int32_t* cand_t, const float* next_s,
                                      const int32_t* next_t, const int32_t* state, const int32_t* cons_table, int B, int k, int t_step,
                                      float* out_s, int32_t* out_t, int32_t* out_beam, int32_t* out_state) {
  if (B <= 0 || k < 1 || k > kMaxBeam || t_step < 0) return SS_ERR_ARG;
  if (!cand_s || !cand_t || !next_s || !next_t || !state || !cons_table || !out_s || !out_t || !out_beam || !out_state)
    return SS_ERR_ARG;
  ConsArgs ca;
  ca.tab = cons_table; ca.state = state; ca.next_s = const_cast<float*>(next_s); ca.next_t = const_cast<int32_t*>(next_t);
  hipLaunchKernelGGL(beam_cons_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, cand_s, cand_t, ca, k, t_step, out_s, out_t,
                     out_beam, out_state);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
