// Ragged-batch beam search of the offline first-pass text decoder (ss_batch_mt_beam): B utterances x k hypothesis rows advance in
// lockstep from [</s>].  Reference: SequenceGenerator.generate_decoder (fairseq/examples/speech_to_speech/unity/sequence_generator.py
// :158-525) with BeamSearch.step (fairseq/fairseq/search.py:110-150) and finalize_hypos (fairseq/fairseq/sequence_generator.py:630-760).
//
// Where fairseq reorders every layer's KV cache after each step, hypothesis slot r here writes its K/V row of step s at [r][s] and
// never overwrites it; the ancestry table anc[r][p] names the slot that holds position p of hypothesis r, and the decode attention
// reads keys and values through it (AttnArgs::anc).  A step then moves B*k*L ints instead of layers x B*k*L x 3D floats.  The tokens
// and cumulative scores fed at each step are kept step-major ([step][slot], never overwritten), so a hypothesis' tokens and scores are
// read through the same table.  Per step, after the decoder launches the greedy twin makes as they are:
//   beam_topk_kernel   one workgroup per hypothesis row: log-softmax of the logits, the reference's masks, + cumulative score, the
//                      row's 2k best candidates (the global top 2k over beam x vocab is inside the union of the per-row lists)
//   beam_merge_kernel  one workgroup per utterance: the global top 2k in the reference's order (score, then flattened index), the
//                      finalisation into the utterance's table, the active hypotheses, next tokens / scores / ancestry, done flag
// The host reads the done flags every kCheck steps, as ss_batch_mt_greedy does; nothing else synchronises per step.
//
// ss_batch_mt_beam_continue is the same search behind a forced prefix per utterance (the streaming write path): fairseq's
// prefix_tokens of that generator (_prefix_tokens, fairseq/fairseq/sequence_generator.py:596-623).  The forced positions run ONCE per
// utterance, as rows of the ragged prefix pass the greedy continuation uses (mt_prefix_pass, batch.hip); their K/V rows go to the
// utterance's slot 0, and anc[r][p] starts as "slot 0 of my utterance" for them, so nothing is copied into the other k - 1 slots.
//   beam_prefix_score_kernel   one workgroup per forced row: log-softmax value of the forced token, masks as above
//   beam_prefix_chain_kernel   one thread per utterance: the cumulative scores as an in-order float32 chain, and their differences
// Lock-step index t of utterance b is the reference's step n_prefix[b] + t; row b's cache is shifted as in ss_batch_mt_continue, so
// every row writes cache index c0 + t at step t.  ss_batch_mt_beam is the call with no prefix anywhere (c0 = 0, no prefix pass).
//
// The *_opts entry points carry the reference generator's three further controls (ss_mt_search_opts): temperature and the no-repeat
// n-gram ban are the OPT variant of the top-2k kernel (the ban reads the row's history through the ancestry table and the prefix-pass
// tokens, on the device, inside the step), the temperature also a variant of the prefix score kernel, the length penalty a variant of
// the merge kernel.  The variants are chosen on the host once per search; with every option at its default the launches are the plain
// kernels, which are the `false` instantiations of the same bodies.  A forced prefix that itself repeats an n-gram is refused by the
// planner, so the prefix pass needs no ban; the agents' and pools' committed prefixes never trip that check, because each of their
// tokens was chosen under the same ban.
//
// ss_batch_mt_beam_cons is the search without a prefix under lexical constraints (fairseq's LexicallyConstrainedBeamSearch, ordered):
// the CONS variants of the same two bodies, chosen on the host in the same way, and one int of state per slot beside the ancestry.
#include <cmath>

#include "model_internal.hpp"

namespace {

constexpr int kMaxBeam = 32, kMaxCand = 2 * kMaxBeam;

// a beats b: higher score, then lower flattened index (torch.topk order); index < 0 = no candidate
__device__ __forceinline__ bool beats(float a, int ia, float b, int ib) {
  return ib < 0 || (ia >= 0 && (a > b || (a == b && ia < ib)));
}

// ---- lexical constraints (ss_batch_mt_beam_cons; the rule stands in include/streamspeech_hip.h) ----
// The ordered constraint state of a hypothesis is one int.  The CONS variants of the two step kernels are chosen on the host once
// per search, as OPT and LENPEN are: the top-2k kernel bans </s> for an unfinished row and notes the scores of the row's at most two
// next tokens while it fills the row; the merge kernel runs cons_select between the rank merge and the step logic.
constexpr int kConsMax = SS_MT_CONS_MAX_TOKENS, kConsLd = SS_MT_CONS_TABLE_LD;
constexpr int kConsCand = 5 * kMaxBeam;          // 2k global + k row bests + 2k next tokens

struct ConsArgs {
  const int* tab = nullptr;      // [B][kConsLd] seq | C | U | end bits lo | hi
  const int* state = nullptr;    // [R] the states this step reads
  int* state_nxt = nullptr;      // [R] the states the next step reads
  float* next_s = nullptr;       // [R][2] scores of the row's next tokens
  int* next_t = nullptr;         // [R][2] the row's next tokens, ascending; -1 = none
};

struct ConsRow {
  const int* seq;
  int C, U;
  unsigned long long endm;
};

__host__ __device__ inline ConsRow cons_row(const int* tab, int b) {
  const int* cr = tab + (size_t)b * kConsLd;
  ConsRow c;
  c.seq = cr;
  c.C = cr[kConsMax] < 0 ? 0 : cr[kConsMax] > kConsMax ? kConsMax : cr[kConsMax];
  c.U = cr[kConsMax + 1];
  c.endm = (unsigned long long)(unsigned)cr[kConsMax + 2] | ((unsigned long long)(unsigned)cr[kConsMax + 3] << 32);
  return c;
}

__host__ __device__ inline int cons_clamp_state(const ConsRow& c, int s) { return s < -1 ? -1 : s > c.C - 1 ? c.C - 1 : s; }

// OrderedConstraintState.advance
__host__ __device__ inline int cons_advance(const ConsRow& c, int s, int tok) {
  if (s + 1 == c.C) return s;
  if (c.seq[s + 1] == tok) return s + 1;
  if (s < 0 || ((c.endm >> s) & 1ull)) return s;   // s == -1: endpoints[-1], the last one, always set
  return tok == c.seq[0] ? 0 : -1;
}

// OrderedConstraintState.next_tokens, ascending, -1 = none
__host__ __device__ inline void cons_next_tokens(const ConsRow& c, int s, int& n0, int& n1) {
  n0 = n1 = -1;
  if (s > 0) n0 = c.seq[0];
  if (s + 1 != c.C) {
    const int x = c.seq[s + 1];
    if (n0 < 0) n0 = x;
    else if (x != n0) { n1 = x > n0 ? x : n0; n0 = x > n0 ? n0 : x; }
  }
}

// the sort key of a candidate, formed as the reference forms it: int -> float32, one float32 add
__host__ __device__ inline float cons_key(const ConsRow& c, int new_state, float score) {
  return (float)((c.U - (new_state + 1)) * -100) + score;
}

// Row r = b*k + j of the logits -> its 2k best (score, token), score = masked log-softmax + cumulative score of the hypothesis.
// Log-softmax numerics of log_softmax_kernel (elementwise.hip).  Masks in the reference's order (unity/sequence_generator.py:290-327):
// NaN -> -inf, pad -inf, unk -= unk_penalty, step >= max_len: all but </s> -inf, step < min_len: </s> -inf.
// Lock-step index t; the reference's step of utterance b is npre[b] + t.
//
// OPT (ss_mt_search_opts; the plain search instantiates OPT = false, which is the code it always was): the logits are divided by the
// temperature wherever they are read, and with ngram = n >= 2 the reference's no-repeat ban (fairseq/fairseq/ngram_repeat_block.py
// ::_no_repeat_ngram) is a phase of this kernel.  The row's step + 1 tokens are staged in LDS behind vals -- the forced ones from the
// utterance's prefix-pass tokens, the fed ones through the ancestry table -- the step + 2 - n windows are compared one per thread,
// and a match sets the bit of the token behind the window in a V-bit map, which the mask chain reads right after min_len.
struct TopkOpts {
  float temp = 1.f;        // temperature
  int ngram = 0;           // 0, or 2 .. 32
  const int* tok = nullptr;    // [t_step + 1][R] step-major fed tokens
  const int* anc = nullptr;    // [R][Lc] the ancestry table read at this step
  int R = 0, Lc = 0, c0 = 0;
  const int* ptok = nullptr;   // prefix-pass tokens (</s> first) of utterance b from row0[b]; read for positions < npre[b] only
  const int* row0 = nullptr;
  float* row_scores = nullptr; // [R][V] or null: the candidate scores of the row as the selection sees them
};

// dynamic LDS of the top-2k kernel: the row, and with a ban the row's history and the bit map
size_t topk_lds_bytes(int V, int ngram, int Lc) {
  return (size_t)V * sizeof(float) + (ngram >= 2 ? ((size_t)Lc + (size_t)(V + 31) / 32) * sizeof(int) : 0);
}

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
  [[maybe_unused]] unsigned* banned = nullptr;     // [ceil(V / 32)] bit n: token n is banned at this step
  if constexpr (OPT) {
    if (o.ngram >= 2) {
      int* hist = reinterpret_cast<int*>(vals + V);  // [Lc] tokens[0 .. step] of the row
      banned = reinterpret_cast<unsigned*>(hist + o.Lc);
      const int np = npre[b], n1 = o.ngram - 1, nwin = step + 1 - n1;
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
      for (int i = t; i < nwin; i += 256) {          // window i against the last n - 1 tokens, tokens[nwin .. step]
        bool same = true;
        for (int j = 0; j < n1 && same; ++j) same = hist[i + j] == hist[nwin + j];
        const int tk = hist[i + n1];
        if (same && (unsigned)tk < (unsigned)V) atomicOr(&banned[tk >> 5], 1u << (tk & 31));
      }
      __syncthreads();
    }
  }
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
  const float lse = logf((sa[0] + sa[1]) + (sa[2] + sa[3]));
  const bool at_max = step >= max_len[b];
  const float c = cum[row];
  [[maybe_unused]] bool ban_eos = false;
  [[maybe_unused]] int nt0 = -1, nt1 = -1;
  if constexpr (CONS) {
    const ConsRow cr = cons_row(ca.tab, b);
    const int cs = cons_clamp_state(cr, ca.state[row]);
    ban_eos = step > 0 && cs + 1 != cr.C;
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
    float v = (logit(n) - mx) - lse;
    if (v != v) v = -INFINITY;
    if (n == pad) v = -INFINITY;
    if (n == unk) v -= unk_pen;
    if (at_max && n != eos) v = -INFINITY;
    if (step < min_len && n == eos) v = -INFINITY;
    if constexpr (OPT) {
      if (banned && ((banned[n >> 5] >> (n & 31)) & 1u)) v = -INFINITY;
    }
    if constexpr (CONS) {
      if (ban_eos && n == eos) v = -INFINITY;
    }
    if (step > 0) v = v + c;
    if constexpr (OPT) {
      if (o.row_scores) o.row_scores[(size_t)row * V + n] = v;
    }
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

struct BeamState {
  int* tok;        // [Tn + 3][R] token fed at lock-step index t by slot r
  float* cum;      // [Tn + 3][R] cumulative score of the hypothesis fed at lock-step index t by slot r
  int* anc;        // [2][R][Lc]  ping-pong ancestry over cache indices: anc[t & 1] is read at lock-step index t
  float* cand_s;   // [R][kMaxCand]
  int* cand_t;     // [R][kMaxCand]
  int* ignore;     // [R] cands_to_ignore of the reference (per utterance, per candidate position < k)
  int* done;       // [B]
  int* max_len;    // [B]
  int* npre;       // [B] forced prefix tokens of the utterance (0: the search starts at [</s>])
  // finalised table: count [B], score [B][k] (normalised if asked), length [B][k] (tokens incl. the final </s>),
  // tokens / positional scores (both after the prefix) / ancestry (by cache index) [B][k][Lc]
  int* fin_cnt; float* fin_score; int* fin_len; int* fin_tok; float* fin_pos; int* fin_anc;
};

// One workgroup per utterance: merge the k sorted per-row lists into the global top 2k, then the step logic of
// unity/sequence_generator.py:329-470 and finalize_hypos.  t_step is the lock-step index (reference step npre[b] + t_step); every
// slot wrote cache index c0 + t_step at this step, so the ancestry entries in use are the cache indices 0 .. c0 + t_step.
// LENPEN (ss_mt_search_opts::len_penalty != 1): a finalised score is divided by (step + 1) ** len_penalty, formed as the reference forms
// it -- the power in double, rounded to float32, then one float32 division.  The plain search instantiates LENPEN = false.
// The rank merge of both merge kernels: the nl sorted lists of nc entries from row r0 on -> sel_* [nc], the global top nc in order.
__device__ __forceinline__ void beam_rank_merge(const float* __restrict__ cand_s, const int* __restrict__ cand_t, int r0, int nl,
                                                int nc, float* ms, int* mt, float* sel_s, int* sel_t, int* sel_beam) {
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

template <bool LENPEN, bool CONS = false>
__device__ __forceinline__ void beam_merge_body(const BeamState& st, int k, int R, int Lc, int V, int t_step, int c0, int eos,
                                                int normalize, float len_penalty, const ConsArgs& ca = ConsArgs{}) {
  __shared__ float ms[kMaxBeam * kMaxCand];
  __shared__ int mt[kMaxBeam * kMaxCand];
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
  if (st.done[b]) {                  // finished utterance: its rows keep decoding (lockstep) -- keep their tables valid, nothing else
    for (int i = t; i < k * na; i += 256) {
      const int j = i / na, p = i - j * na;
      anc_nxt[(size_t)(r0 + j) * Lc + p] = p <= ci ? anc_cur[(size_t)(r0 + j) * Lc + p] : r0 + j;
    }
    if (t < k) { tok_nxt[r0 + t] = eos; cum_nxt[r0 + t] = 0.f; }
    return;
  }
  const int nl = t_step == 0 ? 1 : k, nc = 2 * k;
  beam_rank_merge(st.cand_s, st.cand_t, r0, nl, nc, ms, mt, sel_s, sel_t, sel_beam);
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
  if (is_done) {                     // as for a finished utterance above: valid tables for the lockstep rows
    for (int i = t; i < k * na; i += 256) {
      const int j = i / na, p = i - j * na;
      anc_nxt[(size_t)(r0 + j) * Lc + p] = p <= ci ? anc_cur[(size_t)(r0 + j) * Lc + p] : r0 + j;
    }
    if (t < k) { tok_nxt[r0 + t] = eos; cum_nxt[r0 + t] = 0.f; }
    return;
  }
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
  __shared__ float ms[kMaxBeam * kMaxCand];
  __shared__ int mt[kMaxBeam * kMaxCand];
  __shared__ float sel_s[kMaxCand];
  __shared__ int sel_t[kMaxCand], sel_beam[kMaxCand], sel_st[kMaxCand];
  const int t = threadIdx.x, b = blockIdx.x, nc = 2 * k;
  beam_rank_merge(cand_s, cand_t, b * k, t_step == 0 ? 1 : k, nc, ms, mt, sel_s, sel_t, sel_beam);
  cons_select(ca, cand_s, cand_t, b, k, t_step, sel_s, sel_t, sel_beam, sel_st);
  if (t < nc) {
    const size_t o = (size_t)b * kMaxCand + t;
    out_s[o] = sel_s[t]; out_t[o] = sel_t[t]; out_beam[o] = sel_beam[t]; out_state[o] = sel_st[t];
  }
}

// d_feats row i = slot-major state row idx[i]; rows with idx < 0 (past the best hypothesis) are left as they are
__global__ __launch_bounds__(256) void beam_feat_gather_kernel(const int* __restrict__ idx, const float* __restrict__ src, int D,
                                                               int src_rows, float* __restrict__ dst) {
  const int r = idx[blockIdx.x];
  if (r < 0 || r >= src_rows) return;
  for (int c = threadIdx.x; c < D; c += 256) dst[(size_t)blockIdx.x * D + c] = src[(size_t)r * D + c];
}

// Forced prefix rows: row i of the prefix pass' logits -> lp[i] = the masked log-softmax value of the token forced there (ftok[i];
// < 0: the row forces nothing).  Log-softmax numerics of beam_topk_kernel.  The reference masks before it forces
// (unity/sequence_generator.py:290-327, then _prefix_tokens): NaN -> -inf, pad -inf, unk -= unk_penalty; a forced step is below
// max_len, and min_len is not applied at it.
// TEMP: the logits are divided by the temperature wherever they are read; the plain search instantiates TEMP = false.
template <bool TEMP>
__device__ __forceinline__ void beam_prefix_score_body(const float* __restrict__ logits, int V, const int* __restrict__ ftok, int pad,
                                                       int unk, float unk_pen, float* __restrict__ lp, float temp) {
  __shared__ float sa[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, row = blockIdx.x;
  const int tk = ftok[row];
  if (tk < 0 || tk >= V) return;
  const float* r = logits + (size_t)row * V;
  auto logit = [&](int n) -> float {
    if constexpr (TEMP) return r[n] / temp; else return r[n];
  };
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
  if (t != 0) return;
  const float lse = logf((sa[0] + sa[1]) + (sa[2] + sa[3]));
  float v = (logit(tk) - mx) - lse;
  if (v != v) v = -INFINITY;
  if (tk == pad) v = -INFINITY;
  if (tk == unk) v -= unk_pen;
  lp[row] = v;
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

// ---- sampling (ss_batch_mt_sample; the rule stands in include/streamspeech_hip.h at ss_mt_sample_opts) ----
// The same frame as the beam search: B utterances x k slots in lockstep, the same decoder launches, the same state and finalised
// table.  Slot j of an utterance is chain j, an independent ancestral sample, so the ancestry is the identity after the prefix and is
// written once; per step
//   sample_step_kernel     one workgroup per chain row: the row phase of beam_topk_body (temperature, log-softmax, masks, ban; no
//                          cumulative score), the kept set (top-k: a radix select of the K-th value over integer histograms; top-p:
//                          one bitonic sort of the row's ids in LDS, ordered by (value descending, id ascending), and a scan of
//                          the masses in that order), one fixed-order scan of the kept masses in id order, the draw
//   sample_advance_kernel  one workgroup per utterance: cumulative scores, finalisation of the chains that drew </s>, ignore flags,
//                          next tokens, done flag
// No float atomics anywhere: every sum is a per-thread sequential chain over a contiguous chunk, then one shuffle scan per wave and
// the four wave totals in order, so a row's bits depend on the row alone.

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1) -> c
__host__ __device__ inline void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (unsigned)p1; c[2] = n2; c[3] = (unsigned)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// counter (step, j, key_lo, key_hi), key (seed_lo, seed_hi); u = (word 0 >> 8) * 2^-24
__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned long long key, int step, int j, unsigned w[4]) {
  w[0] = (unsigned)step; w[1] = (unsigned)j; w[2] = (unsigned)key; w[3] = (unsigned)(key >> 32);
  philox4x32_10(w, (unsigned)seed, (unsigned)(seed >> 32));
  return (float)(w[0] >> 8) * 0x1p-24f;
}

__global__ __launch_bounds__(256) void sample_uniform_kernel(int n, const unsigned long long* __restrict__ seed,
                                                             const unsigned long long* __restrict__ key, const int* __restrict__ step,
                                                             const int* __restrict__ j, float* __restrict__ u,
                                                             unsigned* __restrict__ words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned w[4];
  u[i] = sample_uniform(seed[i], key[i], step[i], j[i], w);
  for (int q = 0; q < 4; ++q) words[4 * i + q] = w[q];
}

struct SampleArgs {
  int topk = 0;                  // 0 = off
  float topp = 0.f;              // 0 = off
  unsigned long long seed = 0;
  const unsigned long long* keys = nullptr;   // [B] one per utterance
  const int* row_j = nullptr;    // [R] chain index of the row, or null: row - b * k
  const int* ignore = nullptr;   // [R] or null: finalised chains take no part
  int npad = 0;                  // top-p: the power of two >= V the sort runs over
  int out_ld = 1;                // row stride of tok_out / score_out
  int* tok_out = nullptr;        // [R][out_ld] the drawn token
  float* score_out = nullptr;    // [R][out_ld] its value v[token]
  float* u_out = nullptr;        // [R] or null
  int* kept_out = nullptr;       // [R] or null: the size of the kept set
};

// dynamic LDS of the step kernel: the row | with a ban the history and the bit map (as the top-2k kernel) | the ids the sort orders
size_t sample_lds_bytes(int V, int ngram, int Lc, int npad) { return topk_lds_bytes(V, ngram, Lc) + (size_t)npad * sizeof(int); }
constexpr size_t kSampleLdsMax = 144 * 1024;   // of the CU's 160 KiB; a row of 16384 with its ids is 128 KiB

// exclusive prefix of x over the 256 threads in thread order, and the total; sw [4]
__device__ __forceinline__ float block_excl_scan(float x, float* sw, float& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  float ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = 0.f;
  __syncthreads();                                 // earlier readers of sw are done
  if (lane == 63) sw[wave] = inc;
  __syncthreads();
  float base = 0.f;
  for (int w = 0; w < wave; ++w) base += sw[w];
  total = ((sw[0] + sw[1]) + sw[2]) + sw[3];
  return base + ex;
}

// the same over ints
__device__ __forceinline__ int block_excl_scan_int(int x, int* si, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  __syncthreads();
  if (lane == 63) si[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += si[w];
  total = si[0] + si[1] + si[2] + si[3];
  return base + inc - x;
}

// a float as an unsigned that orders as the float does (-0 counts as +0; no NaN comes here)
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned b = v == 0.f ? 0u : __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// OP: 0 sum, 1 min, 2 max over the 256 threads; si [4]
template <int OP>
__device__ __forceinline__ int block_reduce_int(int x, int* si) {
  auto f = [](int a, int b) { return OP == 0 ? a + b : OP == 1 ? min(a, b) : max(a, b); };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = f(x, __shfl_xor(x, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = x;
  __syncthreads();
  return f(f(si[0], si[1]), f(si[2], si[3]));
}

__global__ __launch_bounds__(256) void sample_step_kernel(const float* __restrict__ logits, int V, int k, int t_step, int min_len,
                                                          const int* __restrict__ max_len, const int* __restrict__ npre,
                                                          const int* __restrict__ done, int pad, int unk, int eos, float unk_pen,
                                                          TopkOpts o, SampleArgs sp) {
  extern __shared__ float vals[];                  // [V] the row's candidate values v[n]
  __shared__ float sa[4];
  __shared__ int si[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x, b = row / k, j = sp.row_j ? sp.row_j[row] : row - b * k;
  if ((done && done[b]) || (sp.ignore && sp.ignore[row])) return;
  const int step = t_step + npre[b];
  // first free step: every chain draws from the row of slot 0 (lprobs[:, ::beam_size] of Sampling.step)
  const float* r = logits + (size_t)(t_step == 0 ? b * k : row) * V;
  auto logit = [&](int n) -> float { return r[n] / o.temp; };
  int* ids = reinterpret_cast<int*>(vals + V);     // [npad], behind the ban's arrays when there is a ban
  unsigned* banned = nullptr;
  // ---- the row phase of beam_topk_body<true>, expression for expression ----
  if (o.ngram >= 2) {
    int* hist = reinterpret_cast<int*>(vals + V);
    banned = reinterpret_cast<unsigned*>(hist + o.Lc);
    ids = reinterpret_cast<int*>(banned + (V + 31) / 32);
    const int np = npre[b], n1 = o.ngram - 1, nwin = step + 1 - n1;
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
    for (int i = t; i < nwin; i += 256) {
      bool same = true;
      for (int q = 0; q < n1 && same; ++q) same = hist[i + q] == hist[nwin + q];
      const int tk = hist[i + n1];
      if (same && (unsigned)tk < (unsigned)V) atomicOr(&banned[tk >> 5], 1u << (tk & 31));
    }
    __syncthreads();
  }
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
  const float lse = logf((sa[0] + sa[1]) + (sa[2] + sa[3]));
  const bool at_max = step >= max_len[b];
  int nfin = 0;
  for (int n = t; n < V; n += 256) {
    float v = (logit(n) - mx) - lse;
    if (v != v) v = -INFINITY;
    if (n == pad) v = -INFINITY;
    if (n == unk) v -= unk_pen;
    if (at_max && n != eos) v = -INFINITY;
    if (step < min_len && n == eos) v = -INFINITY;
    if (banned && ((banned[n >> 5] >> (n & 31)) & 1u)) v = -INFINITY;
    vals[n] = v;
    nfin += v > -INFINITY ? 1 : 0;
  }
  nfin = block_reduce_int<0>(nfin, si);            // its barriers also publish vals
  // ---- the kept set: every token that stands at or before (vt, it) in the order (value descending, id ascending) ----
  bool thr = false;                                // a threshold (vt, it) applies; without one every finite token is kept
  float vt = -INFINITY;
  int it = -1, nk = nfin;
  if (sp.topk > 0 && sp.topk < nfin) {
    // top-k: a radix select of the K-th largest value, eight bits a pass, over integer histograms in LDS (exact); then the ties at
    // that value are taken in ascending id order
    __shared__ int hist[256];
    __shared__ unsigned sel[2];
    unsigned prefix = 0;
    int rem = sp.topk;                             // the ranks still to pass inside the current prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[t] = 0;
      __syncthreads();
      const unsigned himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
      for (int n = t; n < V; n += 256) {
        const unsigned key = order_key(vals[n]);
        if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      const int c = hist[255 - t];                 // thread t owns bin 255 - t: the scan runs from the largest values down
      int tot;
      const int ex = block_excl_scan_int(c, si, tot);
      if (ex < rem && rem <= ex + c) { sel[0] = 255u - t; sel[1] = (unsigned)ex; }
      __syncthreads();
      prefix |= sel[0] << shift;
      rem -= (int)sel[1];
      __syncthreads();                             // sel and hist are written again in the next pass
    }
    vt = __uint_as_float((prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix);
    const int C = (V + 255) / 256, n0 = min(t * C, V), n1 = min(n0 + C, V);
    int c = 0;
    for (int n = n0; n < n1; ++n) c += order_key(vals[n]) == prefix ? 1 : 0;
    int tot;
    const int ex = block_excl_scan_int(c, si, tot);
    if (ex < rem && rem <= ex + c) {
      int q = ex;
      for (int n = n0; n < n1; ++n)
        if (order_key(vals[n]) == prefix && ++q == rem) { sel[0] = (unsigned)n; break; }
    }
    __syncthreads();
    it = (int)sel[0];
    nk = sp.topk;
    thr = true;
  } else if (sp.topp > 0.f) {
    const int N = sp.npad;
    for (int i = t; i < N; i += 256) ids[i] = i < V ? i : -1;
    __syncthreads();
    auto before = [&](int a, int c) -> bool {      // a stands before c; ids < 0 are the padding and stand last
      if (c < 0) return a >= 0;
      if (a < 0) return false;
      const float va = vals[a], vc = vals[c];
      return va > vc || (va == vc && a < c);
    };
    for (int size = 2; size <= N; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = t; i < (N >> 1); i += 256) {
          const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo + stride;
          const int a = ids[lo], c = ids[hi];
          if ((lo & size) == 0 ? before(c, a) : before(a, c)) { ids[lo] = c; ids[hi] = a; }
        }
        __syncthreads();
      }
    // _sample_topp: position i of the order is kept while the mass before it is < P; one fixed-order scan over the positions
    const int C = (N + 255) / 256, i0 = t * C, i1 = min(i0 + C, nfin);
    float loc = 0.f;
    for (int i = i0; i < i1; ++i) loc += expf(vals[ids[i]]);
    float tot;
    const float ex = block_excl_scan(loc, sa, tot);
    int first = nfin;
    float run = 0.f;
    for (int i = i0; i < i1; ++i) {
      if (!(ex + run < sp.topp)) { first = i; break; }
      run += expf(vals[ids[i]]);
    }
    nk = block_reduce_int<1>(first, si);
    if (nk > 0) { it = ids[nk - 1]; vt = vals[it]; thr = true; }
  }
  auto kept = [&](int n, float v) -> bool {
    if (!(v > -INFINITY)) return false;
    return !thr || v > vt || (v == vt && n <= it);
  };
  // ---- the draw: the kept masses in ascending id order, one scan; the first id whose cumulative mass exceeds u * Z ----
  unsigned w[4];
  const float u = sample_uniform(sp.seed, sp.keys[b], step, j, w);
  const int C = (V + 255) / 256, n0 = min(t * C, V), n1 = min(n0 + C, V);
  float loc = 0.f;
  int cnt = 0, last = -1;
  for (int n = n0; n < n1; ++n) {
    const float v = vals[n];
    if (kept(n, v)) { loc += expf(v); ++cnt; last = n; }
  }
  float Z;
  const float ex = block_excl_scan(loc, sa, Z);
  const float target = u * Z;
  int pick = 0x7fffffff;
  float run = 0.f;
  for (int n = n0; n < n1; ++n) {
    const float v = vals[n];
    if (!kept(n, v)) continue;
    run += expf(v);
    if (ex + run > target) { pick = n; break; }
  }
  pick = block_reduce_int<1>(pick, si);
  last = block_reduce_int<2>(last, si);
  cnt = block_reduce_int<0>(cnt, si);
  if (pick == 0x7fffffff) pick = last >= 0 ? last : eos;   // u * Z rounded up to the last sum: the last kept id; nothing kept: </s>
  if (t == 0) {
    sp.tok_out[(size_t)row * sp.out_ld] = pick;
    sp.score_out[(size_t)row * sp.out_ld] = vals[pick];
    if (sp.u_out) sp.u_out[row] = u;
    if (sp.kept_out) sp.kept_out[row] = cnt;
  }
}

// One workgroup per utterance, after sample_step_kernel: chain j = slot j takes its drawn token.  Its cumulative score is the
// in-order float32 sum of the positional scores (behind a prefix, on top of the prefix' sum, which slot 0 holds at lock-step index
// 0).  A chain that drew </s> is finalised into entry j of the utterance's table -- score as beam_merge_body forms it -- and is
// ignored from then on; the utterance is done when all k chains are.  Tokens and positional scores go to entry j step by step; the
// ancestry never changes (both halves of st.anc hold it from the start), so a finalised entry copies its row.
__global__ __launch_bounds__(64) void sample_advance_kernel(BeamState st, int k, int R, int Lc, int t_step, int c0, int eos,
                                                            int normalize, float len_penalty) {
  const int t = threadIdx.x, b = blockIdx.x, r0 = b * k, r = r0 + t;
  int* tok_nxt = st.tok + (size_t)(t_step + 1) * R;
  float* cum_nxt = st.cum + (size_t)(t_step + 1) * R;
  if (st.done[b]) {                  // finished utterance: its rows keep decoding (lockstep)
    if (t < k) { tok_nxt[r] = eos; cum_nxt[r] = 0.f; }
    return;
  }
  const int step = t_step + st.npre[b], ci = c0 + t_step;
  bool fin = false, now = false;
  if (t < k) {
    fin = st.ignore[r] != 0;
    int tk = eos;
    float c = 0.f;
    if (!fin) {
      tk = st.cand_t[(size_t)r * kMaxCand];
      const float v = st.cand_s[(size_t)r * kMaxCand];
      const float prv = st.cum[(size_t)t_step * R + (t_step == 0 ? r0 : r)];
      c = step > 0 ? v + prv : v;
      const size_t o = (size_t)r * Lc;
      st.fin_tok[o + t_step] = tk;
      st.fin_pos[o + t_step] = v;
      if (tk == eos) {
        float s = c;
        if (normalize)
          s = len_penalty != 1.f ? c / (float)pow((double)(step + 1), (double)len_penalty) : c / (float)(step + 1);
        st.fin_score[r] = s;
        st.fin_len[r] = t_step + 1;
        st.ignore[r] = 1;
        fin = now = true;
        c = 0.f;
      }
    }
    tok_nxt[r] = tk;
    cum_nxt[r] = c;
  }
  const unsigned long long fm = __ballot(fin), nm = __ballot(now);
  const int cnt = __popcll(fm);
  if (t == 0) {
    st.fin_cnt[b] = cnt;
    st.done[b] = cnt == k || step >= st.max_len[b];
  }
  const int* anc_cur = st.anc + (size_t)(t_step & 1) * R * Lc;
  for (int q = 0; q < k; ++q)
    if ((nm >> q) & 1ull)
      for (int p = t; p <= ci; p += 64) st.fin_anc[(size_t)(r0 + q) * Lc + p] = anc_cur[(size_t)(r0 + q) * Lc + p];
}

// ss_mt_sample_opts as the search uses it
struct SampleOpts {
  int topk = 0;
  float topp = 0.f;
  unsigned long long seed = 0;
  const int64_t* h_keys = nullptr;
};

// The refusals of the sampling entry points that need no model, in the documented order.
int read_sample_opts(const ss_mt_sample_opts* o, const int64_t* h_keys, SampleOpts& sp) {
  if (!o || o->size < (int32_t)sizeof(ss_mt_sample_opts)) return SS_ERR_ARG;
  if (o->topk < 0) return SS_ERR_ARG;
  if (!std::isfinite(o->topp) || o->topp < 0.f || o->topp > 1.f) return SS_ERR_ARG;
  if (o->topk > 0 && o->topp > 0.f) return SS_ERR_ARG;            // the reference silently prefers top-p
  if (!h_keys) return SS_ERR_ARG;
  sp.topk = o->topk; sp.topp = o->topp; sp.seed = o->seed; sp.h_keys = h_keys;
  return SS_OK;
}

int sample_npad(const SampleOpts& sp, int V) {
  if (sp.topp == 0.f) return 0;                    // top-k selects without a sort
  int n = 1;
  while (n < V) n <<= 1;
  return n;
}

// Host-side layout of one beam call behind forced prefixes, and every refusal it makes (exported as ss_batch_mt_beam_continue_plan).
// Utterance b has npp_b rows in the prefix pass, fed [</s>, prefix_b...] from position 0.  With beam > 1 the last forced token is the
// first lock-step row of all k slots (pm = 0, npp_b = n_prefix_b), exactly as </s> is with no prefix: ss_batch_mt_beam is then the
// case n_prefix = 0 launch for launch.  ss_batch_mt_beam_continue at beam 1 takes pm = 1: the last forced token is the last row of
// the prefix pass (npp_b = n_prefix_b + 1) and the first free step reads that row's projection, which is ss_batch_mt_continue's
// arithmetic.  Row b's cache is shifted by sh_b = Smax - npp_b (Smax = the most prefix-pass rows), so lock-step index t writes
// cache index c0 + t everywhere (c0 = the longest prefix).
// `tab` holds, in this order: lock-step cross segs [4R] | lock-step self segs [Tn + 1][4R] | row position offset [R] | first
// prefix-pass row [B] | prefix self segs [4 nseg] | prefix cross segs [4 nseg] | prefix tokens | positions | cache rows | feature rows
// | forced tokens [Np] each | last prefix-pass row [B].
// ss_mt_search_opts as the search uses it; the defaults are the search without options.
struct SearchOpts {
  int ngram = 0;
  float len_penalty = 1.f, temp = 1.f;
};

// The option refusals of the *_opts entry points, made before every other check.
int read_search_opts(const ss_mt_search_opts* o, SearchOpts& so) {
  so = SearchOpts{};
  if (!o) return SS_OK;
  if (o->size < (int32_t)sizeof(ss_mt_search_opts)) return SS_ERR_ARG;
  const int n = o->no_repeat_ngram;
  if (n != 0 && (n < 2 || n > 32)) return SS_ERR_ARG;            // n = 1: the reference's two implementations disagree
  if (!std::isfinite(o->len_penalty)) return SS_ERR_ARG;
  if (!std::isfinite(o->temperature) || !(o->temperature > 0.f)) return SS_ERR_ARG;
  so.ngram = n; so.len_penalty = o->len_penalty; so.temp = o->temperature;
  return SS_OK;
}

// The refusals of ss_mt_cons_table_host, and the table the kernels read ([B][kConsLd], ConsArgs::tab).
int cons_table(int B, const int32_t* h_cons, const int32_t* h_off, const int32_t* h_end, int V, int pad, int eos,
               const int32_t* h_max_len, std::vector<int>& tab) {
  if (B <= 0 || !h_off) return SS_ERR_ARG;
  tab.assign((size_t)B * kConsLd, 0);
  for (int b = 0; b < B; ++b) {
    const int o = h_off[b], C = h_off[b + 1] - o;
    if (o < 0 || C < 0 || C > kConsMax) return SS_ERR_ARG;
    if (C > 0 && (!h_cons || !h_end)) return SS_ERR_ARG;
    if (h_max_len && C > h_max_len[b]) return SS_ERR_ARG;
    int* row = tab.data() + (size_t)b * kConsLd;
    unsigned long long endm = 0;
    int U = 0;
    for (int i = 0; i < C; ++i) {
      const int id = h_cons[o + i];
      if (id < 0 || id >= V || id == pad || id == eos) return SS_ERR_ARG;
      U += std::find(row, row + i, id) == row + i ? 1 : 0;
      row[i] = id;
      if (h_end[o + i]) endm |= 1ull << i;
    }
    if (C > 0 && !((endm >> (C - 1)) & 1ull)) return SS_ERR_ARG;   // the last phrase is empty or open
    row[kConsMax] = C; row[kConsMax + 1] = U; row[kConsMax + 2] = (int)(unsigned)endm; row[kConsMax + 3] = (int)(unsigned)(endm >> 32);
  }
  return SS_OK;
}

// tokens[0 .. n) = </s>, then the prefix: does any n-gram stand in it twice?  Then the ban would hit a forced token.
bool prefix_repeats_ngram(const std::vector<int>& tokens, int ngram) {
  const int L = (int)tokens.size();
  for (int e = ngram; e < L; ++e)                                // a later n-gram tokens[e - ngram + 1 .. e] ...
    for (int i = 0; i + ngram - 1 < e; ++i)                      // ... against an earlier one tokens[i .. i + ngram - 1]
      if (std::equal(tokens.begin() + i, tokens.begin() + i + ngram, tokens.begin() + e - ngram + 1)) return true;
  return false;
}

struct BcPlan {
  int pm = 0, S = 0, Smax = 0, c0 = 0, Tn = 0, Lc = 0, Np = 0, np_max = 0, nseg = 0, R = 0;
  std::vector<int> tab, tok0;
  size_t o_lself = 0, o_rowpos = 0, o_row0 = 0, o_pself = 0, o_pcross = 0, o_ptok = 0, o_plast = 0;
};

int beam_continue_plan(int B, int beam, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix,
                       const int32_t* h_max_len, int min_len, int out_stride, int feat_rows, int max_tgt_pos, int vocab, int eos,
                       int pad, int pm, BcPlan& P, int ngram = 0) {
  if (B <= 0 || beam < 1 || beam > kMaxBeam || !h_Tp || !h_max_len) return SS_ERR_ARG;
  if ((long)B * beam > 256) return SS_ERR_CAPACITY;              // the row limit of the greedy twin (segment tables of the slab kernels)
  if (vocab < 2 * beam + 1 || (size_t)vocab * sizeof(float) > 65536) return SS_ERR_ARG;   // the top-2k kernel holds a row in LDS
  const int k = beam, R = B * beam;
  auto npre = [&](int b) { return h_n_prefix ? h_n_prefix[b] : 0; };
  int S = 0, Tn = 0, Np = 0, np_max = 0, nseg = 0;
  for (int b = 0; b < B; ++b) {
    const int st = npre(b);
    if (h_Tp[b] <= 0 || st < 0 || h_max_len[b] < st || min_len > h_max_len[b]) return SS_ERR_ARG;
    if (st > 0 && !h_prefix) return SS_ERR_ARG;
    S = std::max(S, st);
    Tn = std::max(Tn, h_max_len[b] - st);
    Np += st + pm;
    np_max = std::max(np_max, st + pm);
    nseg += st + pm > 0 ? 1 : 0;
  }
  for (int b = 0, o = 0; b < B; ++b) {
    for (int i = 0; i < npre(b); ++i) {
      const int id = h_prefix[o + i];
      if (id < 0 || id >= vocab) return SS_ERR_ARG;              // nn.Embedding's IndexError in the reference
      if (id == eos || id == pad) return SS_ERR_ARG;             // a committed prefix never holds one (no replicate_first_beam, no padding)
    }
    o += npre(b);
  }
  for (int b = 0; b < B; ++b)                            // fed positions 0 .. max_len_b; scores of up to max_len_b + 1 tokens
    if (h_max_len[b] + 1 > feat_rows || h_max_len[b] + 1 > out_stride || h_max_len[b] + 4 > max_tgt_pos) return SS_ERR_CAPACITY;
  if (ngram >= 2)                                        // a prefix that repeats an n-gram would ban one of its own forced tokens
    for (int b = 0, o = 0; b < B; o += npre(b), ++b) {
      std::vector<int> tokens(1, eos);
      tokens.insert(tokens.end(), h_prefix + (npre(b) ? o : 0), h_prefix + (npre(b) ? o + npre(b) : 0));
      if (prefix_repeats_ngram(tokens, ngram)) return SS_ERR_ARG;
    }
  const int Smax = S + pm, c0 = S, Lc = c0 + Tn + 2;
  const Offsets oe = prefix(h_Tp, B);
  P.pm = pm; P.S = S; P.Smax = Smax; P.c0 = c0; P.Tn = Tn; P.Lc = Lc; P.Np = Np; P.np_max = np_max; P.nseg = nseg; P.R = R;
  const size_t np = (size_t)Np, nl = (size_t)(Tn + 1) * 4 * R;
  P.o_lself = 4 * (size_t)R; P.o_rowpos = P.o_lself + nl; P.o_row0 = P.o_rowpos + R; P.o_pself = P.o_row0 + B;
  P.o_pcross = P.o_pself + 4 * (size_t)nseg; P.o_ptok = P.o_pcross + 4 * (size_t)nseg; P.o_plast = P.o_ptok + 5 * np;
  P.tab.assign(P.o_plast + B, 0);
  P.tok0.assign(R, eos);
  int* cs = P.tab.data(); int* ls = cs + P.o_lself; int* rp = cs + P.o_rowpos; int* r0s = cs + P.o_row0; int* ps = cs + P.o_pself;
  int* pc = cs + P.o_pcross; int* pt = cs + P.o_ptok; int* pp = pt + np; int* pk = pp + np; int* pf = pk + np; int* ft = pf + np;
  int* pl = cs + P.o_plast;
  for (int b = 0, o = 0, row = 0, seg = 0; b < B; ++b) {
    const int st = npre(b), npp = st + pm, sh = Smax - npp;
    for (int j = 0; j < k; ++j) {
      const int r = b * k + j;
      cs[4 * r] = r; cs[4 * r + 1] = 1; cs[4 * r + 2] = oe.off[b]; cs[4 * r + 3] = h_Tp[b];
      rp[r] = -sh;
      for (int t = 0; t <= Tn; ++t) {
        int* e = &ls[((size_t)t * R + r) * 4];
        e[0] = r; e[1] = 1; e[2] = sh; e[3] = c0 + t + 1 - sh;       // keys: cache indices sh .. c0 + t (positions 0 .. n_prefix + t)
      }
      if (st > 0) P.tok0[r] = h_prefix[o + st - 1];
    }
    r0s[b] = row;
    pl[b] = npp > 0 ? row + npp - 1 : 0;
    if (npp > 0) {
      ps[4 * seg] = row; ps[4 * seg + 1] = npp; ps[4 * seg + 2] = row; ps[4 * seg + 3] = npp;
      pc[4 * seg] = row; pc[4 * seg + 1] = npp; pc[4 * seg + 2] = oe.off[b]; pc[4 * seg + 3] = h_Tp[b];
      ++seg;
    }
    for (int p = 0; p < npp; ++p) {
      pt[row + p] = p == 0 ? eos : h_prefix[o + p - 1];
      pp[row + p] = p;
      pk[row + p] = b * k * Lc + sh + p;                             // slot 0 of the utterance
      pf[row + p] = b * feat_rows + p;
      ft[row + p] = p < st ? h_prefix[o + p] : -1;
    }
    row += npp;
    o += st;
  }
  return SS_OK;
}

// The search of both entry points; the checks of `P` are done.  With `smp` the same call samples: sample_step_kernel and
// sample_advance_kernel stand where the top-2k and merge kernels stand, everything else is shared.
int beam_search(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp, const int32_t* h_n_prefix,
                const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, const BcPlan& P, int32_t* h_out_tokens,
                int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                const SearchOpts& so, const SampleOpts* smp = nullptr, const std::vector<int>* cons_tab = nullptr) {
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, F = c.dec_ffn, V = c.tgt_vocab, k = beam, R = B * beam;
  const int Lc = P.Lc, Tn = P.Tn, c0 = P.c0, Np = P.Np;
  // the option kernels are chosen here, once: a search without options launches what it always launched
  const bool topk_opts = so.ngram >= 2 || so.temp != 1.f, merge_lenpen = normalize && so.len_penalty != 1.f;
  if ((topk_opts || cons_tab) && topk_lds_bytes(V, so.ngram, Lc) > 65536) return SS_ERR_ARG;
  const int npad = smp ? sample_npad(*smp, V) : 0;
  const size_t smp_lds = smp ? sample_lds_bytes(V, so.ngram, Lc, npad) : 0;
  if (smp_lds > kSampleLdsMax) return SS_ERR_ARG;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  const Offsets oe = prefix(h_Tp, B);
  // ---- scratch: everything booked before the first launch ----
  const size_t np = (size_t)Np;
  const size_t n_tok = (size_t)(Tn + 3) * R, n_anc = (size_t)2 * R * Lc, n_cand = (size_t)R * kMaxCand, n_fin = (size_t)B * k * Lc;
  const size_t n_fin_words = B + 2 * (size_t)B * k + 3 * n_fin;
  // constraints: states [2][R] (ping-pong, as the ancestry) | next-token scores and ids [R][2] each | the table
  const size_t n_cons = cons_tab ? 6 * (size_t)R + cons_tab->size() : 0;
  const size_t n_state = 2 * n_tok + n_anc + 2 * n_cand + R + 3 * (size_t)B + n_fin_words + n_cons;
  RET(m->sc->mt_cross.ensure((size_t)c.mt_layers * oe.total * 2 * D * sizeof(float)));
  RET(m->sc->bmt_self.ensure((size_t)c.mt_layers * R * Lc * 3 * D * sizeof(float)));
  RET(m->sc->bmb_feat.ensure((size_t)R * Lc * D * sizeof(float)));
  RET(m->sc->mt_ws.ensure((MtRowsWs::floats(R, D, F, V) + (P.pm ? (size_t)R * D : 0)) * sizeof(float)));
  RET(m->sc->bmb_state.ensure(n_state * sizeof(int)));
  // prefix pass: its workspace (mt_prefix_pass) | logits [Np][V] | forced log-probabilities [Np] | their positional scores [Np]
  if (Np > 0) RET(m->sc->ws.ensure((np * (7 * D + F) + np * V + 2 * np) * sizeof(float)));
  // int tables: the plan's tables | feature gather [B][feat_rows]
  const size_t o_keys = (P.tab.size() + (size_t)B * feat_rows + 1) / 2 * 2;   // sampling: the utterances' keys, 8-byte aligned
  RET(m->sc->seg_buf.ensure((smp ? o_keys + 2 * (size_t)B : P.tab.size() + (size_t)B * feat_rows) * sizeof(int)));

  RET(mt_cross_kv(m, s, d_enc_out, oe.total));
  float* feat = m->sc->bmb_feat.f();           // [R][Lc][D] post-LN decoder states of every slot and cache index
  const MtRowsWs rows_ws(m->sc->mt_ws.f(), R, D, F);
  float* logits = rows_ws.logits;
  float* last_rows = logits + (size_t)R * V;   // beam 1: each utterance's last prefix-pass state
  int* w = (int*)m->sc->bmb_state.p;
  BeamState st;
  st.tok = w; w += n_tok;
  st.cum = (float*)w; w += n_tok;
  st.anc = w; w += n_anc;
  st.cand_s = (float*)w; w += n_cand;
  st.cand_t = w; w += n_cand;
  st.ignore = w; w += R;
  st.done = w; w += B;
  st.max_len = w; w += B;
  st.npre = w; w += B;
  int* fin_base = w;
  st.fin_cnt = w; w += B;
  st.fin_score = (float*)w; w += (size_t)B * k;
  st.fin_len = w; w += (size_t)B * k;
  st.fin_tok = w; w += n_fin;
  st.fin_pos = (float*)w; w += n_fin;
  st.fin_anc = w; w += n_fin;
  int* cons_state = w;
  ConsArgs ca;
  if (cons_tab) {
    ca.next_s = (float*)(w + 2 * R); ca.next_t = w + 4 * R; ca.tab = w + 6 * R;
  }
  int* d_tab = (int*)m->sc->seg_buf.p;
  const int* d_cross = d_tab;
  const int* d_self = d_tab + P.o_lself;
  const int* d_rowpos = d_tab + P.o_rowpos;
  const int* d_row0 = d_tab + P.o_row0;
  int* d_gather = d_tab + P.tab.size();
  const std::vector<int> np0 = h_n_prefix ? std::vector<int>(h_n_prefix, h_n_prefix + B) : std::vector<int>(B, 0);   // lives to the end of the call
  SS_HIP_CHECK(hipMemsetAsync(m->sc->bmb_state.p, 0, n_state * sizeof(int), s));   // slot 0 / score 0 / nothing finalised everywhere
  {
    std::vector<int> a0((size_t)R * Lc), ml(h_max_len, h_max_len + B);
    for (int r = 0; r < R; ++r) {                // prefix-pass positions live in slot 0 of the utterance, the others in the slot itself
      std::fill(a0.begin() + (size_t)r * Lc, a0.begin() + (size_t)r * Lc + P.Smax, (r / k) * k);
      std::fill(a0.begin() + (size_t)r * Lc + P.Smax, a0.begin() + (size_t)(r + 1) * Lc, r);
    }
    RET(upload(s, st.tok, P.tok0)); RET(upload(s, st.max_len, ml)); RET(upload(s, d_tab, P.tab));
    RET(upload(s, st.anc, a0));
    if (smp) {                                   // the ancestry never changes: both halves hold it
      RET(upload(s, st.anc + (size_t)R * Lc, a0));
      SS_HIP_CHECK(hipMemcpyAsync(d_tab + o_keys, smp->h_keys, (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    if (h_n_prefix) RET(upload(s, st.npre, np0));
    if (cons_tab) {                              // every hypothesis starts at the root
      RET(upload(s, cons_state, std::vector<int>((size_t)2 * R, -1)));
      RET(upload(s, cons_state + 6 * R, *cons_tab));
    }
  }
  const float* d_prepos = nullptr;
  if (Np > 0) {
    // ---- the prefix pass: every forced position once per utterance, K/V into slot 0, then the forced tokens' scores ----
    const int* d_ptok = d_tab + P.o_ptok;
    const int *d_ppos = d_ptok + np, *d_pcache = d_ppos + np, *d_pfeat = d_pcache + np, *d_ftok = d_pfeat + np;
    const float* pfo = nullptr;
    RET(mt_prefix_pass(m, s, P.nseg, Np, P.np_max, oe.total, d_ptok, d_ppos, d_tab + P.o_pself, d_tab + P.o_pcross, nullptr, d_pcache,
                       R * Lc, &pfo));
    RET(launch_scatter_rows(d_pfeat, pfo, D, d_feats, D, D, Np, B * feat_rows, s));
    float* plog = m->sc->ws.f() + np * (7 * D + F);
    float* lp = plog + np * V;
    float* prepos = lp + np;
    Lin proj{m->mt_emb, nullptr};
    RET(linear(s, pfo, D, Np, proj, V, D, plog, V));
    if (so.temp != 1.f)
      hipLaunchKernelGGL(beam_prefix_score_temp_kernel, dim3(Np), dim3(256), 0, s, plog, V, d_ftok, c.pad, c.unk, unk_penalty, lp,
                         so.temp);
    else
      hipLaunchKernelGGL(beam_prefix_score_kernel, dim3(Np), dim3(256), 0, s, plog, V, d_ftok, c.pad, c.unk, unk_penalty, lp);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_prefix_chain_kernel, dim3((B + 255) / 256), dim3(256), 0, s, lp, d_row0, st.npre, B, k, st.cum, prepos);
    SS_LAUNCH_CHECK();
    if (P.pm) RET(launch_gather_rows(d_tab + P.o_plast, pfo, D, last_rows, B, s, Np));
    d_prepos = prepos;
  }
  std::vector<int> host_done(B, 0);
  int step = 0;                                // lock-step index
  constexpr int kCheck = 4;
  CanonScope decode_scope(m->pack_invariant ? CANON_SMALLM : CANON_NONE);   // the greedy twin's decode-row GEMM form
  while (true) {
    const int ci = c0 + step;                  // cache index every slot writes at this step
    if (P.pm && step == 0) {                   // beam 1: the first free step reads the last prefix-pass row, projected as a lock-step row
      Lin proj{m->mt_emb, nullptr};
      RET(linear(s, last_rows, D, R, proj, V, D, logits, V));
    } else {                                   // a slot's cache rows are written once and never reordered: the ancestor table finds them
      MtRowsStep a;
      a.rows = R; a.cache_ld = Lc; a.ci = ci; a.tok = st.tok + (size_t)step * R; a.row_pos = d_rowpos; a.row_pad = -1;
      a.self_segs = d_self + (size_t)step * 4 * R; a.cross_segs = d_cross; a.n_enc = oe.total;
      a.anc = st.anc + (size_t)(step & 1) * R * Lc; a.anc_ld = Lc; a.anc_slots = R;
      a.states = feat + (size_t)ci * D; a.states_ld = Lc * D;
      RET(mt_decode_rows(m, s, rows_ws, a));
    }
    if (smp) {
      TopkOpts to;
      to.temp = so.temp; to.ngram = so.ngram; to.tok = st.tok; to.anc = st.anc; to.R = R; to.Lc = Lc; to.c0 = c0;
      to.ptok = d_tab + P.o_ptok; to.row0 = d_row0;
      SampleArgs sa;
      sa.topk = smp->topk; sa.topp = smp->topp; sa.seed = smp->seed;
      sa.keys = reinterpret_cast<const unsigned long long*>(d_tab + o_keys); sa.ignore = st.ignore; sa.npad = npad;
      sa.out_ld = kMaxCand; sa.tok_out = st.cand_t; sa.score_out = st.cand_s;
      SS_MAX_LDS_ONCE(sample_step_kernel, kSampleLdsMax);
      hipLaunchKernelGGL(sample_step_kernel, dim3(R), dim3(256), smp_lds, s, logits, V, k, step, min_len, st.max_len, st.npre, st.done,
                         c.pad, c.unk, c.eos, unk_penalty, to, sa);
    } else if (cons_tab) {
      TopkOpts to;
      to.temp = so.temp; to.ngram = so.ngram; to.tok = st.tok; to.anc = st.anc + (size_t)(step & 1) * R * Lc; to.R = R; to.Lc = Lc;
      to.c0 = c0; to.ptok = d_tab + P.o_ptok; to.row0 = d_row0;
      ca.state = cons_state + (size_t)(step & 1) * R; ca.state_nxt = cons_state + (size_t)((step + 1) & 1) * R;
      hipLaunchKernelGGL(beam_topk_cons_kernel, dim3(R), dim3(256), topk_lds_bytes(V, so.ngram, Lc), s, logits, V, k, step, min_len,
                         st.max_len, st.npre, st.done, st.cum + (size_t)step * R, c.pad, c.unk, c.eos, unk_penalty, st.cand_s,
                         st.cand_t, to, ca);
    } else if (topk_opts) {
      TopkOpts to;
      to.temp = so.temp; to.ngram = so.ngram; to.tok = st.tok; to.anc = st.anc + (size_t)(step & 1) * R * Lc; to.R = R; to.Lc = Lc;
      to.c0 = c0; to.ptok = d_tab + P.o_ptok; to.row0 = d_row0;
      hipLaunchKernelGGL(beam_topk_opts_kernel, dim3(R), dim3(256), topk_lds_bytes(V, so.ngram, Lc), s, logits, V, k, step, min_len,
                         st.max_len, st.npre, st.done, st.cum + (size_t)step * R, c.pad, c.unk, c.eos, unk_penalty, st.cand_s,
                         st.cand_t, to);
    } else {
      hipLaunchKernelGGL(beam_topk_kernel, dim3(R), dim3(256), V * sizeof(float), s, logits, V, k, step, min_len, st.max_len, st.npre,
                         st.done, st.cum + (size_t)step * R, c.pad, c.unk, c.eos, unk_penalty, st.cand_s, st.cand_t);
    }
    SS_LAUNCH_CHECK();
    if (smp)
      hipLaunchKernelGGL(sample_advance_kernel, dim3(B), dim3(64), 0, s, st, k, R, Lc, step, c0, c.eos, normalize ? 1 : 0, so.len_penalty);
    else if (cons_tab && merge_lenpen)
      hipLaunchKernelGGL(beam_merge_cons_lenpen_kernel, dim3(B), dim3(256), 0, s, st, k, R, Lc, V, step, c0, c.eos, 1, so.len_penalty,
                         ca);
    else if (cons_tab)
      hipLaunchKernelGGL(beam_merge_cons_kernel, dim3(B), dim3(256), 0, s, st, k, R, Lc, V, step, c0, c.eos, normalize ? 1 : 0, ca);
    else if (merge_lenpen)
      hipLaunchKernelGGL(beam_merge_lenpen_kernel, dim3(B), dim3(256), 0, s, st, k, R, Lc, V, step, c0, c.eos, 1, so.len_penalty);
    else
      hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(256), 0, s, st, k, R, Lc, V, step, c0, c.eos, normalize ? 1 : 0);
    SS_LAUNCH_CHECK();
    const bool last = step >= Tn;              // every utterance is done at its max_len step
    ++step;
    if (last || step % kCheck == 0) {
      SS_HIP_CHECK(hipMemcpyAsync(host_done.data(), st.done, B * sizeof(int), hipMemcpyDeviceToHost, s));
      SS_HIP_CHECK(hipStreamSynchronize(s));
      bool all = true;
      for (int b = 0; b < B; ++b) all = all && host_done[b];
      if (all || last) break;
    }
  }
  // ---- results: the finalised tables, sorted by score (descending; ties keep finalisation order) ----
  std::vector<int> fin(n_fin_words);
  std::vector<float> prepos(np);
  SS_HIP_CHECK(hipMemcpyAsync(fin.data(), fin_base, n_fin_words * sizeof(int), hipMemcpyDeviceToHost, s));
  if (Np > 0) SS_HIP_CHECK(hipMemcpyAsync(prepos.data(), d_prepos, np * sizeof(float), hipMemcpyDeviceToHost, s));
  SS_HIP_CHECK(hipStreamSynchronize(s));
  const int* f_cnt = fin.data();
  const float* f_score = reinterpret_cast<const float*>(f_cnt + B);
  const int* f_len = f_cnt + B + (size_t)B * k;
  const int* f_tok = f_len + (size_t)B * k;
  const float* f_pos = reinterpret_cast<const float*>(f_tok + n_fin);
  const int* f_anc = f_tok + 2 * n_fin;
  const int* row0 = P.tab.data() + P.o_row0;
  std::vector<int> gidx((size_t)B * feat_rows, -1);
  for (int b = 0; b < B; ++b) {
    const int n = std::min(f_cnt[b], k), npre = h_n_prefix ? h_n_prefix[b] : 0, npp = npre + P.pm, sh = P.Smax - npp;
    std::vector<int> ord(n);
    for (int e = 0; e < n; ++e) ord[e] = e;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int e) { return f_score[b * k + a] > f_score[b * k + e]; });
    for (int i = 0; i < k; ++i) {
      const size_t o = (size_t)b * k + i;
      if (i >= n) { h_n_out[o] = 0; h_scores[o] = -INFINITY; continue; }
      const int e = ord[i], len = f_len[b * k + e];
      const size_t src = ((size_t)b * k + e) * Lc;
      h_n_out[o] = len;
      h_scores[o] = f_score[b * k + e];
      for (int p = 0; p < len; ++p) h_out_tokens[o * out_stride + p] = f_tok[src + p];
      if (h_pos_scores) {                      // the whole hypothesis: the forced tokens' scores, then the generated ones'
        for (int p = 0; p < npre; ++p) h_pos_scores[o * out_stride + p] = prepos[row0[b] + p];
        for (int p = 0; p < len; ++p) h_pos_scores[o * out_stride + npre + p] = f_pos[src + p];
      }
      if (i == 0)           // the best hypothesis' decoder states past the prefix pass: fed positions npp .. n_prefix + len - 1
        for (int q = npp; q < npre + len; ++q) gidx[(size_t)b * feat_rows + q] = f_anc[src + sh + q] * Lc + sh + q;
    }
  }
  RET(upload(s, d_gather, gidx));
  hipLaunchKernelGGL(beam_feat_gather_kernel, dim3(B * feat_rows), dim3(256), 0, s, d_gather, feat, D, R * Lc, d_feats);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace

// Batched beam search of the first-pass text decoder (include/streamspeech_hip.h): the search with no prefix anywhere.
static int mt_beam_entry(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                         const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                         int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                         const ss_mt_search_opts* opts, const SampleOpts* smp, const int32_t* h_cons = nullptr,
                         const int32_t* h_cons_off = nullptr, const int32_t* h_cons_end = nullptr) {
  SearchOpts so;
  RET(read_search_opts(opts, so));
  if (!m || B <= 0 || beam < 1 || beam > kMaxBeam || !d_feats || !h_out_tokens || !h_n_out || !h_scores) return SS_ERR_ARG;
  if ((long)B * beam > 256) return SS_ERR_CAPACITY;              // the row limit of the greedy twin (segment tables of the slab kernels)
  const ss_config& c = m->cfg;
  if (c.tgt_vocab < 2 * beam + 1 || (size_t)c.tgt_vocab * sizeof(float) > 65536) return SS_ERR_ARG;   // the top-2k kernel holds a row in LDS
  int Lmax = 0;
  for (int b = 0; b < B; ++b) {
    if (h_Tp[b] <= 0 || h_max_len[b] < 0 || min_len > h_max_len[b]) return SS_ERR_ARG;
    Lmax = std::max(Lmax, h_max_len[b]);
  }
  if (Lmax + 2 > feat_rows || Lmax + 4 > c.max_tgt_pos || out_stride < Lmax + 1) return SS_ERR_CAPACITY;
  BcPlan P;
  RET(beam_continue_plan(B, beam, h_Tp, nullptr, nullptr, h_max_len, min_len, out_stride, feat_rows, c.max_tgt_pos, c.tgt_vocab, c.eos,
                         c.pad, 0, P));      // position 0 is a lock-step row at every beam (beam 1 is ss_batch_mt_greedy bit for bit)
  std::vector<int> cons_tab;
  if (h_cons_off) RET(cons_table(B, h_cons, h_cons_off, h_cons_end, c.tgt_vocab, c.pad, c.eos, h_max_len, cons_tab));
  return beam_search(m, stream, B, beam, d_enc_out, h_Tp, nullptr, h_max_len, min_len, unk_penalty, normalize, P, h_out_tokens,
                     out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, so, smp, h_cons_off ? &cons_tab : nullptr);
}

extern "C" int ss_batch_mt_beam_cons(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                     const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                     int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                     int feat_rows, const ss_mt_search_opts* opts, const int32_t* h_cons, const int32_t* h_cons_off,
                                     const int32_t* h_cons_end) {
  if (!h_cons_off) return SS_ERR_ARG;
  return mt_beam_entry(m, stream, B, beam, d_enc_out, h_Tp, h_max_len, min_len, unk_penalty, normalize, h_out_tokens, out_stride,
                       h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts, nullptr, h_cons, h_cons_off, h_cons_end);
}

extern "C" int ss_mt_cons_table_host(int B, const int32_t* h_cons, const int32_t* h_cons_off, const int32_t* h_cons_end, int V,
                                     int pad, int eos, const int32_t* h_max_len, int32_t* h_table) {
  std::vector<int> tab;
  RET(cons_table(B, h_cons, h_cons_off, h_cons_end, V, pad, eos, h_max_len, tab));
  if (h_table) std::copy(tab.begin(), tab.end(), h_table);
  return SS_OK;
}

// Steps 1 - 8 of the rule, serially: the twin of beam_topk_cons_kernel's masks and beam_merge_cons_kernel's selection.
extern "C" int ss_mt_cons_select_host(const float* h_lprobs, const float* h_cum, int k, int V, int step, int eos,
                                      const int32_t* h_state, const int32_t* h_cons, int n_cons, const int32_t* h_cons_end,
                                      float* out_scores, int32_t* out_tokens, int32_t* out_beams, int32_t* out_states) {
  if (!h_lprobs || !h_cum || !h_state || !out_scores || !out_tokens || !out_beams || !out_states) return SS_ERR_ARG;
  if (k < 1 || k > kMaxBeam || V < 2 * k + 1 || step < 0 || eos < 0 || eos >= V || n_cons < 0) return SS_ERR_ARG;
  const int32_t off[2] = {0, n_cons};
  std::vector<int> tab;
  RET(cons_table(1, h_cons, off, h_cons_end, V, -1, eos, nullptr, tab));
  const ConsRow cr = cons_row(tab.data(), 0);
  const int nrow = step == 0 ? 1 : k, nc = 2 * k;
  for (int j = 0; j < nrow; ++j)
    if (h_state[j] < -1 || h_state[j] > cr.C - 1) return SS_ERR_ARG;
  struct Cand { float s, key; int tok, beam, st, bank_rank; };
  std::vector<float> v((size_t)nrow * V);
  for (int j = 0; j < nrow; ++j)
    for (int n = 0; n < V; ++n) {
      float x = h_lprobs[(size_t)j * V + n];
      if (step > 0 && n == eos && h_state[j] + 1 != cr.C) x = -INFINITY;
      if (step > 0) x = x + h_cum[j];
      v[(size_t)j * V + n] = x;
    }
  std::vector<Cand> list;
  auto push = [&](int j, int n) {
    Cand c;
    c.s = v[(size_t)j * V + n]; c.tok = n; c.beam = j; c.st = cons_advance(cr, h_state[j], n); c.key = cons_key(cr, c.st, c.s);
    c.bank_rank = 0;
    list.push_back(c);
  };
  {
    std::vector<int> idx((size_t)nrow * V);
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
    std::partial_sort(idx.begin(), idx.begin() + nc, idx.end(), [&](int a, int e) { return v[a] > v[e] || (v[a] == v[e] && a < e); });
    for (int q = 0; q < nc; ++q) push(idx[q] / V, idx[q] % V);
  }
  if (step > 0)
    for (int j = 0; j < k; ++j) {
      int bi = 0;
      for (int n = 1; n < V; ++n)
        if (v[(size_t)j * V + n] > v[(size_t)j * V + bi]) bi = n;
      push(j, bi);
    }
  for (int j = 0; j < nrow; ++j) {
    int n0, n1;
    cons_next_tokens(cr, h_state[j], n0, n1);
    if (n0 >= 0) push(j, n0);
    if (n1 >= 0) push(j, n1);
  }
  std::stable_sort(list.begin(), list.end(), [](const Cand& a, const Cand& e) { return a.key > e.key; });
  std::vector<Cand> uniq;
  for (const Cand& c : list) {
    bool seen = false;
    for (const Cand& u : uniq) seen = seen || (u.beam == c.beam && u.tok == c.tok);
    if (!seen) uniq.push_back(c);
  }
  for (size_t i = 0; i < uniq.size(); ++i)
    for (size_t j = 0; j < i; ++j) uniq[i].bank_rank += uniq[j].st == uniq[i].st ? 1 : 0;
  std::stable_sort(uniq.begin(), uniq.end(), [](const Cand& a, const Cand& e) {
    return a.bank_rank < e.bank_rank || (a.bank_rank == e.bank_rank && a.st > e.st);
  });
  for (int q = 0; q < nc; ++q) {
    out_scores[q] = uniq[q].s; out_tokens[q] = uniq[q].tok; out_beams[q] = uniq[q].beam; out_states[q] = uniq[q].st;
  }
  return SS_OK;
}

extern "C" int ss_batch_mt_beam_opts(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                     const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                     int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                     int feat_rows, const ss_mt_search_opts* opts) {
  return mt_beam_entry(m, stream, B, beam, d_enc_out, h_Tp, h_max_len, min_len, unk_penalty, normalize, h_out_tokens, out_stride,
                       h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts, nullptr);
}

// Sampling (include/streamspeech_hip.h at ss_mt_sample_opts): the sampling refusals, then the entry above.
static int sample_entry_opts(const ss_model* m, const int64_t* h_keys, const ss_mt_sample_opts* sample, SampleOpts& smp) {
  RET(read_sample_opts(sample, h_keys, smp));
  if (!m) return SS_ERR_ARG;
  if (smp.topk > m->cfg.tgt_vocab) return SS_ERR_ARG;
  return SS_OK;
}

extern "C" int ss_batch_mt_sample(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                  const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                  int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                  int feat_rows, const ss_mt_search_opts* opts, const int64_t* h_keys,
                                  const ss_mt_sample_opts* sample) {
  SampleOpts smp;
  RET(sample_entry_opts(m, h_keys, sample, smp));
  return mt_beam_entry(m, stream, B, beam, d_enc_out, h_Tp, h_max_len, min_len, unk_penalty, normalize, h_out_tokens, out_stride,
                       h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts, &smp);
}

extern "C" int ss_batch_mt_beam(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                int feat_rows) {
  return ss_batch_mt_beam_opts(m, stream, B, beam, d_enc_out, h_Tp, h_max_len, min_len, unk_penalty, normalize, h_out_tokens,
                               out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, nullptr);
}

// The same search behind a forced prefix per utterance (include/streamspeech_hip.h).
static int mt_beam_continue_entry(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                  const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                  float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                                  float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows, const ss_mt_search_opts* opts,
                                  const SampleOpts* smp) {
  SearchOpts so;
  RET(read_search_opts(opts, so));
  if (!m || !d_enc_out || !h_n_prefix || !d_feats || !h_out_tokens || !h_n_out || !h_scores) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  BcPlan P;
  RET(beam_continue_plan(B, beam, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, out_stride, feat_rows, c.max_tgt_pos, c.tgt_vocab,
                         c.eos, c.pad, beam == 1 ? 1 : 0, P, so.ngram));
  return beam_search(m, stream, B, beam, d_enc_out, h_Tp, h_n_prefix, h_max_len, min_len, unk_penalty, normalize, P, h_out_tokens,
                     out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, so, smp);
}

extern "C" int ss_batch_mt_beam_continue_opts(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                              const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len,
                                              int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride,
                                              int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                                              const ss_mt_search_opts* opts) {
  return mt_beam_continue_entry(m, stream, B, beam, d_enc_out, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, unk_penalty, normalize,
                                h_out_tokens, out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts, nullptr);
}

extern "C" int ss_batch_mt_sample_continue(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                           const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                           float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                                           float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                                           const ss_mt_search_opts* opts, const int64_t* h_keys, const ss_mt_sample_opts* sample) {
  SampleOpts smp;
  RET(sample_entry_opts(m, h_keys, sample, smp));
  return mt_beam_continue_entry(m, stream, B, beam, d_enc_out, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, unk_penalty, normalize,
                                h_out_tokens, out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts, &smp);
}

extern "C" int ss_batch_mt_beam_continue(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                         const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                         float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                                         float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows) {
  return ss_batch_mt_beam_continue_opts(m, stream, B, beam, d_enc_out, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, unk_penalty,
                                        normalize, h_out_tokens, out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows,
                                        nullptr);
}

extern "C" int ss_batch_mt_beam_continue_plan_opts(int B, int beam, const int32_t* h_Tp, const int32_t* h_prefix,
                                                   const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len, int out_stride,
                                                   int feat_rows, int max_tgt_pos, int vocab, int eos, int pad, int32_t* h_dims,
                                                   int32_t* h_tables, int64_t tables_cap, int64_t* h_n_tables,
                                                   const ss_mt_search_opts* opts) {
  SearchOpts so;
  RET(read_search_opts(opts, so));
  if (!h_n_prefix) return SS_ERR_ARG;
  BcPlan P;
  RET(beam_continue_plan(B, beam, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, out_stride, feat_rows, max_tgt_pos, vocab, eos, pad,
                         beam == 1 ? 1 : 0, P, so.ngram));
  if (h_dims) {
    h_dims[0] = P.S; h_dims[1] = P.Tn; h_dims[2] = P.Lc; h_dims[3] = P.Np; h_dims[4] = P.R; h_dims[5] = P.c0; h_dims[6] = P.nseg;
    h_dims[7] = P.pm;
  }
  if (h_n_tables) *h_n_tables = (int64_t)P.tab.size();
  if (h_tables) {
    if (tables_cap < (int64_t)P.tab.size()) return SS_ERR_CAPACITY;
    std::copy(P.tab.begin(), P.tab.end(), h_tables);
  }
  return SS_OK;
}

extern "C" int ss_batch_mt_beam_continue_plan(int B, int beam, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix,
                                              const int32_t* h_max_len, int min_len, int out_stride, int feat_rows, int max_tgt_pos,
                                              int vocab, int eos, int pad, int32_t* h_dims, int32_t* h_tables, int64_t tables_cap,
                                              int64_t* h_n_tables) {
  return ss_batch_mt_beam_continue_plan_opts(B, beam, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, out_stride, feat_rows,
                                             max_tgt_pos, vocab, eos, pad, h_dims, h_tables, tables_cap, h_n_tables, nullptr);
}

// ---- op-level entry points of the kernels above (include/streamspeech_hip.h; tests/test_glue_ops_gpu.py) ----
// The limits both top-k ops share: the search's own (beam_continue_plan).
static int op_topk_limits(int R, int V, int k) {
  if (R <= 0 || k < 1 || k > kMaxBeam || R % k != 0) return SS_ERR_ARG;
  if (V < 2 * k + 1 || (size_t)V * sizeof(float) > 65536) return SS_ERR_ARG;
  return SS_OK;
}

// The checks of both merge ops, and their state as the kernels take it.
static int op_beam_state(const ss_op_beam_state* x, int B, int k, int Lc, int t_step, int c0, BeamState& st) {
  if (!x || B <= 0 || k < 1 || k > kMaxBeam || t_step < 0 || c0 < 0 || c0 + t_step + 2 > Lc) return SS_ERR_ARG;
  st.tok = x->tok; st.cum = x->cum; st.anc = x->anc; st.cand_s = x->cand_s; st.cand_t = x->cand_t; st.ignore = x->ignore;
  st.done = x->done; st.max_len = x->max_len; st.npre = x->npre;
  st.fin_cnt = x->fin_cnt; st.fin_score = x->fin_score; st.fin_len = x->fin_len; st.fin_tok = x->fin_tok; st.fin_pos = x->fin_pos;
  st.fin_anc = x->fin_anc;
  return SS_OK;
}

extern "C" int ss_op_beam_topk(void* stream, const float* logits, int R, int V, int k, int t_step, int min_len, const int32_t* max_len,
                               const int32_t* npre, const int32_t* done, const float* cum, int pad, int unk, int eos, float unk_pen,
                               float* cand_s, int32_t* cand_t) {
  RET(op_topk_limits(R, V, k));
  hipLaunchKernelGGL(beam_topk_kernel, dim3(R), dim3(256), V * sizeof(float), (hipStream_t)stream, logits, V, k, t_step, min_len,
                     max_len, npre, done, cum, pad, unk, eos, unk_pen, cand_s, cand_t);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_op_beam_merge(void* stream, const ss_op_beam_state* x, int B, int k, int Lc, int V, int t_step, int c0, int eos,
                                int normalize) {
  BeamState st;
  RET(op_beam_state(x, B, k, Lc, t_step, c0, st));
  hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, st, k, B * k, Lc, V, t_step, c0, eos,
                     normalize ? 1 : 0);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_op_beam_prefix_score(void* stream, const float* logits, int rows, int V, const int32_t* ftok, int pad, int unk,
                                       float unk_pen, float* lp) {
  if (rows <= 0 || V <= 0) return SS_ERR_ARG;
  hipLaunchKernelGGL(beam_prefix_score_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, V, ftok, pad, unk, unk_pen, lp);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_op_beam_prefix_chain(void* stream, const float* lp, const int32_t* row0, const int32_t* npre, int B, int k,
                                       float* cum0, float* pos) {
  if (B <= 0 || k < 1) return SS_ERR_ARG;
  hipLaunchKernelGGL(beam_prefix_chain_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, lp, row0, npre, B, k, cum0,
                     pos);
  SS_LAUNCH_CHECK();
  return SS_OK;
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

// ---- the option variants (ss_mt_search_opts; tests/test_search_options_gpu.py) ----
extern "C" int ss_op_beam_topk_opts(void* stream, const float* logits, int R, int V, int k, int t_step, int min_len,
                                    const int32_t* max_len, const int32_t* npre, const int32_t* done, const float* cum, int pad, int unk,
                                    int eos, float unk_pen, float* cand_s, int32_t* cand_t, float temperature, int no_repeat_ngram,
                                    const int32_t* tok, const int32_t* anc, int Lc, int c0, const int32_t* ptok, const int32_t* row0,
                                    float* row_scores) {
  const ss_mt_search_opts o{(int32_t)sizeof(ss_mt_search_opts), no_repeat_ngram, 1.f, temperature};
  SearchOpts so;
  RET(read_search_opts(&o, so));
  if (so.ngram == 0 && so.temp == 1.f && !row_scores)
    return ss_op_beam_topk(stream, logits, R, V, k, t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen, cand_s, cand_t);
  RET(op_topk_limits(R, V, k));
  if (t_step < 0) return SS_ERR_ARG;
  if (so.ngram >= 2 && (!tok || !anc || c0 < 0 || c0 + t_step >= Lc)) return SS_ERR_ARG;
  if (topk_lds_bytes(V, so.ngram, Lc) > 65536) return SS_ERR_ARG;
  TopkOpts to;
  to.temp = so.temp; to.ngram = so.ngram; to.tok = tok; to.anc = anc; to.R = R; to.Lc = Lc; to.c0 = c0; to.ptok = ptok; to.row0 = row0;
  to.row_scores = row_scores;
  hipLaunchKernelGGL(beam_topk_opts_kernel, dim3(R), dim3(256), topk_lds_bytes(V, so.ngram, Lc), (hipStream_t)stream, logits, V, k,
                     t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen, cand_s, cand_t, to);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_op_beam_merge_opts(void* stream, const ss_op_beam_state* x, int B, int k, int Lc, int V, int t_step, int c0, int eos,
                                     int normalize, float len_penalty) {
  if (!std::isfinite(len_penalty)) return SS_ERR_ARG;
  if (len_penalty == 1.f || !normalize) return ss_op_beam_merge(stream, x, B, k, Lc, V, t_step, c0, eos, normalize);
  BeamState st;
  RET(op_beam_state(x, B, k, Lc, t_step, c0, st));
  hipLaunchKernelGGL(beam_merge_lenpen_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, st, k, B * k, Lc, V, t_step, c0, eos, 1,
                     len_penalty);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_op_beam_prefix_score_opts(void* stream, const float* logits, int rows, int V, const int32_t* ftok, int pad, int unk,
                                            float unk_pen, float* lp, float temperature) {
  if (!std::isfinite(temperature) || !(temperature > 0.f)) return SS_ERR_ARG;
  if (temperature == 1.f) return ss_op_beam_prefix_score(stream, logits, rows, V, ftok, pad, unk, unk_pen, lp);
  if (rows <= 0 || V <= 0) return SS_ERR_ARG;
  hipLaunchKernelGGL(beam_prefix_score_temp_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, V, ftok, pad, unk, unk_pen,
                     lp, temperature);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ---- sampling (ss_mt_sample_opts; tests/test_sampling_ops_gpu.py) ----
extern "C" int ss_op_sample_step(void* stream, const float* logits, int R, int V, int t_step, int min_len, const int32_t* max_len,
                                 const int32_t* npre, int pad, int unk, int eos, float unk_pen, float temperature, int no_repeat_ngram,
                                 const int32_t* tok, const int32_t* anc, int Lc, int c0, const int32_t* ptok, const int32_t* row0,
                                 const int32_t* row_j, const int64_t* keys, const ss_mt_sample_opts* sample, int32_t* out_tok,
                                 float* out_score, float* out_u, int32_t* out_kept) {
  SampleOpts smp;
  RET(read_sample_opts(sample, keys, smp));
  if (smp.topk > V) return SS_ERR_ARG;
  const ss_mt_search_opts o{(int32_t)sizeof(ss_mt_search_opts), no_repeat_ngram, 1.f, temperature};
  SearchOpts so;
  RET(read_search_opts(&o, so));
  if (R <= 0 || V < 1 || (size_t)V * sizeof(float) > 65536 || t_step < 0 || eos < 0 || eos >= V) return SS_ERR_ARG;
  if (!logits || !max_len || !npre || !row_j || !out_tok || !out_score) return SS_ERR_ARG;
  if (so.ngram >= 2 && (!tok || !anc || c0 < 0 || c0 + t_step >= Lc)) return SS_ERR_ARG;
  const int npad = sample_npad(smp, V);
  const size_t lds = sample_lds_bytes(V, so.ngram, Lc, npad);
  if (lds > kSampleLdsMax) return SS_ERR_ARG;
  TopkOpts to;
  to.temp = so.temp; to.ngram = so.ngram; to.tok = tok; to.anc = anc; to.R = R; to.Lc = Lc; to.c0 = c0; to.ptok = ptok; to.row0 = row0;
  SampleArgs sa;
  sa.topk = smp.topk; sa.topp = smp.topp; sa.seed = smp.seed; sa.keys = reinterpret_cast<const unsigned long long*>(keys);
  sa.row_j = row_j; sa.npad = npad; sa.out_ld = 1; sa.tok_out = out_tok; sa.score_out = out_score; sa.u_out = out_u;
  sa.kept_out = out_kept;
  SS_MAX_LDS_ONCE(sample_step_kernel, kSampleLdsMax);
  hipLaunchKernelGGL(sample_step_kernel, dim3(R), dim3(256), lds, (hipStream_t)stream, logits, V, 1, t_step, min_len, max_len, npre,
                     (const int*)nullptr, pad, unk, eos, unk_pen, to, sa);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_op_sample_uniform(void* stream, int n, const uint64_t* seed, const int64_t* key, const int32_t* step,
                                    const int32_t* j, float* u, uint32_t* words) {
  if (n <= 0 || !seed || !key || !step || !j || !u || !words) return SS_ERR_ARG;
  hipLaunchKernelGGL(sample_uniform_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n,
                     reinterpret_cast<const unsigned long long*>(seed), reinterpret_cast<const unsigned long long*>(key), step, j, u,
                     words);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
