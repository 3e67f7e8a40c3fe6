// CTC prefix beam search on the two text heads: what the device search (ctc_beam.hip) and its host twin (ctc_beam_host.hip) share --
// the limits, the argument checks, the table of a ragged pack, the trie's child lookup, the step code and the frame: passes B and
// C, node creation, the back-trace, the LM finish and the stable-prefix depth are stated here once and called by both.
//
// A hypothesis is a label string (blank = 0 never in it).  Its state is two float64 numbers: pb, the log-probability of all its
// alignments that end in blank, and pnb, of those that end in its last label.  Per frame, with tot = logadd(pb, pnb) and lp the
// frame's float32 log-softmax (pad / unk -inf):
//   p keeps          pb'  += tot + lp[0]                      (ctc_beam_stay)
//   non-empty p      pnb' += pnb + lp[last(p)]                (the TRUE lp of the last label, candidate of this frame or not)
//   p + c            pnb' += (c == last(p) ? pb : tot) + lp[c] (ctc_beam_ext) for the frame's candidates c
// Identity is the string: every string is one node of a per-utterance trie whose child lookup (parent node, token) -> node is an
// open-addressed table that persists over all frames, so a string that left the beam and is proposed again is the node it was.  A
// string has one parent, so a frame's hypothesis gets at most two terms: its own stay and its parent's extension.
//
// THE ORDER of a frame's hypotheses, and with it every tie: the frame's entries are numbered e = r * (cand + 1) + k, where r is the
// rank of the source prefix in the beam that entered the frame (0 = best), k = 0 the prefix itself and k = 1 + j its extension by
// the frame's j-th candidate (candidates ordered by logit descending, lower id first on equal logits).  An extension whose string
// is itself in the beam is folded into that prefix's own entry.  Entry e comes before entry f when tot_e > tot_f, or the totals are
// equal and e < f (ctc_beam_before).  The beam that leaves the frame is the first `beam` entries of that order whose total is above
// -inf, and its ranks are their places in it; the result is the first `nbest` prefixes of the last frame's beam.
//
// THE LM FORM (ss_*_ctc_beam_lm; the model and its scoring rule: ngram_lm.hpp) changes none of the above and adds three things.
// A node also carries lm_state, lm_sum (the sum of lp_lm over its tokens) and bonus, properties of the string written once, when
// the node is made: the root (start state, 0, 0), the child by c with lp = lp_lm(c | lm_state[parent]) gets lm_sum[parent] + lp and
// bonus[parent] + ((lm_weight * lp) + word_score) (ngram_bonus: three rounded operations).  The order of a frame's entries compares
// fused = tot + bonus in place of tot -- an extension's bonus is its node's when the string is in the trie, and is computed from the
// parent's state otherwise, each frame it is proposed -- while pb / pnb / tot stay pure CTC quantities and an entry is alive when its
// tot is above -inf.  At the end hypothesis r of the last beam gets fin = fused + lm_weight * lp_lm(eos | lm_state) (eos_term; fin =
// fused without it; word_score is not applied to eos), and the n-best are the last beam by fin descending, the earlier rank first
// on a tie.  The candidates are chosen by the acoustic logit alone.  Per utterance 20 more bytes per node.
//
// THE BIAS FORM (ss_*_ctc_beam_bias; the hotword set and its scoring rule: ctc_bias.hpp) is one more term of the same bonus, with or
// without a model.  A node also carries b_state, the phrase automaton's state of its string, and bias_sum, the unscaled sum of the
// deltas of its tokens: the root (0, 0), the child by c with delta = bias_step(b_state[parent], c) gets bias_sum[parent] + delta and
// bonus = B1 + (scale * delta) (bias_bonus: two rounded operations), where B1 is ngram_bonus(bonus[parent], ...) with a model and
// bonus[parent] without.  An extension that is not in the trie computes the same from the parent's states each frame it is
// proposed.  At the end fin = fused [+ the eos term] - scale * open(b_state) with `finish` (bias_finish; an unfinished phrase earns
// nothing), and the record's bias_score is bias_sum - open(b_state).  The form is two bits, CTC_FORM_LM | CTC_FORM_BIAS: the bias
// forms keep their keys where the LM form does (e_fus, b_bonus) and add 20 bytes per node alone, 32 with a model.
#pragma once
#include <stdint.h>

#include <vector>

#include "ctc_align.hpp"

struct ss_ngram_lm;                  // include/streamspeech_hip.h
struct ss_ctc_lm_opts;
struct ss_ctc_bias;
struct ss_ctc_bias_opts;

namespace ss {

constexpr int CTC_BEAM_MAX_BEAM = 32;
constexpr int CTC_BEAM_MAX_CAND = 32;
constexpr int CTC_BEAM_MAX_T = CTC_ALIGN_MAX_T;
constexpr int CTC_BEAM_MAX_ENT = CTC_BEAM_MAX_BEAM * (CTC_BEAM_MAX_CAND + 1);
constexpr unsigned long long CTC_BEAM_EMPTY = ~0ull;        // an unused slot of the child table (the buffer is filled with 0xff)
constexpr int CTC_FORM_LM = 1, CTC_FORM_BIAS = 2;           // the bits of a search's form (0: the plain search)

// The per-node fields a form adds: bonus with either bit, lm_sum and lm_state with LM, bias_sum and b_state with BIAS.
constexpr size_t ctc_form_node_bytes(int form) { return form == 0 ? 0 : form == (CTC_FORM_LM | CTC_FORM_BIAS) ? 32 : 20; }
struct CtcFormNodes { double *n_sum, *n_bonus, *n_bsum; int *n_state, *n_bstate; };
// ... and where they lie in `nodes * ctc_form_node_bytes(form)` bytes at an 8-byte aligned w: the doubles first (lm_sum | bonus |
// bias_sum), then the ints (lm_state | b_state), each array `nodes` long, a form's absent ones left out -- the LM form's layout as
// it was.
inline CtcFormNodes ctc_form_carve(void* w, size_t nodes, int form) {
  CtcFormNodes f{nullptr, nullptr, nullptr, nullptr, nullptr};
  double* d = static_cast<double*>(w);
  if (form & CTC_FORM_LM) { f.n_sum = d; d += nodes; }
  if (form) { f.n_bonus = d; d += nodes; }
  if (form & CTC_FORM_BIAS) { f.n_bsum = d; d += nodes; }
  int* i = reinterpret_cast<int*>(d);
  if (form & CTC_FORM_LM) { f.n_state = i; i += nodes; }
  if (form & CTC_FORM_BIAS) f.n_bstate = i;
  return f;
}

// One utterance of a pack.  Its trie: node 0 is the empty string; the node an entry of rank r creates at frame t is
// 1 + t * beam + r, so ids need no counter and at most 1 + beam * T exist.  Its child table has tab_mask + 1 slots, a power of two
// >= 2 * beam * T: never more than half full.
struct CtcBeamSeg {
  long long node_off;   // first node {parent, token} of its trie
  long long tab_off;    // first slot of its child table (keys and values)
  int row0, T;          // packed frame rows [row0, row0 + T)
  int tab_mask, pad_;
};

struct CtcBeamPlan {
  std::vector<CtcBeamSeg> segs;
  long long nodes = 0, slots = 0;
  int rows = 0, max_T = 0, beam = 0, cand = 0, nbest = 0;
  // the work buffer: child keys [slots] u64 | nodes [nodes] int2 | child values [slots] int | den [rows][2] float | cand_id [rows][cand] int
  size_t key_bytes() const { return (size_t)slots * 8; }
  size_t work_bytes() const { return (size_t)slots * 12 + (size_t)nodes * 8 + (size_t)rows * (8 + 4 * (size_t)cand); }
  // the LM form appends, 8-byte aligned: lm_sum [nodes] double | bonus [nodes] double | lm_state [nodes] int
  size_t lm_off() const { return (work_bytes() + 7) & ~(size_t)7; }
  size_t work_bytes_lm() const { return lm_off() + (size_t)nodes * 20; }
  // every form: its per-node fields at lm_off(), ctc_form_carve'd (20 bytes per node, 32 with a model and a bias set)
  size_t work_bytes_form(int form) const { return form == 0 ? work_bytes() : lm_off() + (size_t)nodes * ctc_form_node_bytes(form); }
};

// The sizes of one trie of T frames (an utterance of a pack, or a slot of the resumable form made for T = max_frames).
inline long long ctc_stream_nodes(int beam, int T) { return 1 + (long long)beam * T; }
inline long long ctc_stream_slots(int beam, int T) {
  long long slots = 2;
  while (slots < 2LL * beam * T) slots *= 2;
  return slots;
}

// Every refusal of the three entry points past their pointers, before anything is launched or written: B <= 0, a beam / cand
// outside [1, max_beam] / [1, CTC_BEAM_MAX_CAND], nbest outside [1, beam], a T outside [1, CTC_BEAM_MAX_T], out_stride < max T.
inline int ctc_beam_plan(int V, int B, const int32_t* h_T, int beam, int cand, int nbest, int out_stride, CtcBeamPlan& p,
                         int max_beam = CTC_BEAM_MAX_BEAM) {
  if (V <= 0 || B <= 0 || !h_T || beam < 1 || beam > max_beam || cand < 1 || cand > CTC_BEAM_MAX_CAND || nbest < 1 || nbest > beam)
    return SS_ERR_ARG;
  p.beam = beam; p.cand = cand; p.nbest = nbest;
  p.segs.resize(B);
  for (int b = 0; b < B; ++b) {
    const int T = h_T[b];
    if (T < 1 || T > CTC_BEAM_MAX_T || out_stride < T) return SS_ERR_ARG;
    const long long slots = ctc_stream_slots(beam, T);
    p.segs[b] = CtcBeamSeg{p.nodes, p.slots, p.rows, T, (int)(slots - 1), 0};
    p.nodes += ctc_stream_nodes(beam, T);
    p.slots += slots;
    p.rows += T;
    if (T > p.max_T) p.max_T = T;
  }
  return SS_OK;
}

// ---- the resumable form (ss_ctc_stream_*: ctc_stream.hip, the kernel in ctc_beam.hip) ----
// The same search stopped after any frame and taken up at the next: node ids hold the ABSOLUTE frame, the child table lives as long
// as the utterance, and the beam that left the last frame of a call is stored beside them, so the frames [f, upto) of a call are the
// frames f .. upto - 1 of the one-shot search bit for bit.  Every slot of an object has the same sizes, made for max_frames:
// nodes 1 + beam * max_frames, a table of the power of two >= 2 * beam * max_frames slots (ctc_beam_plan's rule).
struct CtcStreamSess {  // one session of an advance call
  int slot;             // whose state
  int row0;             // its first stacked new row: frame f is row row0
  int f, upto;          // the frames [f, upto) run in this call
  int fin, pad_;        // the utterance's last call: the LM form's eos term, the bias form's finish term
};

struct CtcStreamPart { int frames, n_stable, n_alive, status; };   // ss_ctc_stream_part

// Where the slots' state lies (device pointers; array a of slot s starts at a + s * its per-slot count).
struct CtcStreamDev {
  unsigned long long* keys;   // [S][slots]
  int2* nodes;                // [S][nodes]
  int* vals;                  // [S][slots]
  double* n_sum;              // [S][nodes]   LM form
  double* n_bonus;            // [S][nodes]   LM and bias forms
  int* n_state;               // [S][nodes]   LM form
  double* b_f64;              // [S][4][beam]: pb | pnb | tot | bonus of the stored beam
  int* b_i32;                 // [S][2 beam + 2]: node | last | alive, NaN seen
  long long nodes_per, slots_per;
  const CtcStreamSess* sess;
  CtcStreamPart* part;
};

// The bias forms' two arrays more, [S][nodes] each (beside CtcStreamDev, which the four kernels without a bias set take as it was).
struct CtcStreamBiasDev { double* n_bsum; int* n_bstate; };

// The bytes of one slot, the header's figure: 12 per table slot, 8 per node (28 in the LM form and in the bias form, 40 with both),
// 32 + 8 per beam slot, 8.  form: the CTC_FORM_* bits (0 / 1 are the earlier false / true).
inline size_t ctc_stream_slot_bytes(int beam, int max_frames, int form) {
  const size_t nodes = (size_t)ctc_stream_nodes(beam, max_frames), slots = (size_t)ctc_stream_slots(beam, max_frames);
  return slots * 12 + nodes * (8 + ctc_form_node_bytes(form)) + (size_t)beam * 32 + ((size_t)beam * 2 + 2) * 4;
}
// The arrays of S slots in one piece of S * ctc_stream_slot_bytes: the 8-byte ones first (keys, nodes, the stored beam's doubles,
// the form's doubles), then the 4-byte ones, so every array is aligned whatever S, beam and max_frames are.
inline void ctc_stream_carve(void* mem, int S, int beam, int max_frames, int form, CtcStreamDev* d, CtcStreamBiasDev* bd = nullptr) {
  const bool lm = (form & CTC_FORM_LM) != 0, bias = (form & CTC_FORM_BIAS) != 0;
  const size_t nodes = (size_t)ctc_stream_nodes(beam, max_frames), slots = (size_t)ctc_stream_slots(beam, max_frames);
  unsigned char* w = static_cast<unsigned char*>(mem);
  d->keys = reinterpret_cast<unsigned long long*>(w); w += (size_t)S * slots * 8;
  d->nodes = reinterpret_cast<int2*>(w); w += (size_t)S * nodes * 8;
  d->b_f64 = reinterpret_cast<double*>(w); w += (size_t)S * beam * 32;
  d->n_sum = d->n_bonus = nullptr; d->n_state = nullptr;
  if (bd) { bd->n_bsum = nullptr; bd->n_bstate = nullptr; }
  if (lm) { d->n_sum = reinterpret_cast<double*>(w); w += (size_t)S * nodes * 8; }
  if (form) { d->n_bonus = reinterpret_cast<double*>(w); w += (size_t)S * nodes * 8; }
  if (bias && bd) { bd->n_bsum = reinterpret_cast<double*>(w); w += (size_t)S * nodes * 8; }
  d->vals = reinterpret_cast<int*>(w); w += (size_t)S * slots * 4;
  if (lm) { d->n_state = reinterpret_cast<int*>(w); w += (size_t)S * nodes * 4; }
  if (bias && bd) { bd->n_bstate = reinterpret_cast<int*>(w); w += (size_t)S * nodes * 4; }
  d->b_i32 = reinterpret_cast<int*>(w);
  d->nodes_per = (long long)nodes; d->slots_per = (long long)slots;
  d->sess = nullptr; d->part = nullptr;
}

// One utterance's state in the plain-C++ twins (ctc_beam_host.hip): the kernel's arrays as vectors in the kernel's layout.  The two
// beams are the halves [0, beam) and [beam, 2 beam) of the b_* arrays; the beam that left the last frame is the first `alive`
// entries of half `cur`, in rank order -- which is also all a resumable call stores for the next.
struct CtcBeamHostState {
  std::vector<unsigned long long> keys;
  std::vector<int> vals, n_state, n_bstate;
  std::vector<int2> nodes;
  std::vector<double> n_sum, n_bonus, n_bsum;
  std::vector<double> b_pb, b_pnb, b_tot, b_bonus;
  std::vector<int> b_node, b_last;
  int beam = 0, cur = 0, alive = 0;
  int mask = 0, frames = 0;
  bool bad = false;
  void start(int beam, int max_T, int form, int lm_start);  // the empty string, an empty table for max_T frames (form: CTC_FORM_*)
};

// One launch of the candidate kernel over the `rows` stacked new rows (none: no launch) into den [rows][2] / cand [rows][C], the
// upload of the n sessions to d_sess (n * sizeof(CtcStreamSess)) and one launch of the resumable search kernel, one workgroup per
// session.  dev: the carved state (sess / part are set here).  lm == nullptr: the plain form, hyps ss_ctc_beam_hyp [n][nbest].
// bias != nullptr: a bias form (bdev: its two arrays), with or without lm, hyps ss_ctc_beam_bias_hyp [n][nbest].
// Nothing is checked here: the refusals and the clearing of a reset slot's table are the caller's (ctc_stream.hip).
int launch_ctc_stream(const float* logits, int ld, int V, int pad, int unk, int rows, int n, const CtcStreamSess* h_sess, void* d_sess,
                      float* den, int* cand_id, int beam, int C, int nbest, CtcStreamDev dev, const ss_ngram_lm* lm,
                      const ss_ctc_lm_opts* opts, void* hyps, int* tokens, int out_stride, CtcStreamPart* part, hipStream_t stream,
                      const ss_ctc_bias* bias = nullptr, const ss_ctc_bias_opts* bopts = nullptr, CtcStreamBiasDev bdev = {nullptr, nullptr});
// The same in plain C++ on host logits and host state (ctc_beam_host.hip; one CtcBeamHostState per slot, started by the caller).
int ctc_stream_host_run(std::vector<CtcBeamHostState>& slots, const float* h_logits, int ld, int V, int pad, int unk, int n,
                        const CtcStreamSess* sess, int beam, int cand, int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* o,
                        void* h_hyps, int32_t* h_tokens, int out_stride, CtcStreamPart* h_part, const ss_ctc_bias* bias = nullptr,
                        const ss_ctc_bias_opts* bo = nullptr);

// ---- the step code ----
SS_HD float ctc_beam_lp(float x, float mx, float logsum) { return (x - mx) - logsum; }

SS_HD double ctc_beam_logadd(double a, double b) { return ctc_align_logadd3(a, b, -INFINITY); }

// What prefix (pb, pnb, tot, last) keeps: *pb2 = tot + lp[0]; *pnb2 = pnb + lp[last] (-inf for the empty prefix, last < 0).
SS_HD void ctc_beam_stay(double pnb, double tot, int last, float lp0, float lp_last, double* pb2, double* pnb2) {
  *pb2 = tot + (double)lp0;
  *pnb2 = last >= 0 ? pnb + (double)lp_last : -INFINITY;
}

// What the prefix gives its extension by c.
SS_HD double ctc_beam_ext(double pb, double tot, int last, int c, float lp_c) { return (c == last ? pb : tot) + (double)lp_c; }

// Entry f comes before entry e (the order of the header comment).
SS_HD bool ctc_beam_before(double tot_f, int f, double tot_e, int e) { return tot_f > tot_e || (tot_f == tot_e && f < e); }

SS_HD int ctc_beam_new_node(int t, int beam, int rank) { return 1 + t * beam + rank; }

SS_HD unsigned long long ctc_beam_key(int parent, int tok) { return ((unsigned long long)(unsigned)parent << 32) | (unsigned)tok; }

SS_HD int ctc_beam_slot(unsigned long long key, int mask) { return (int)((key * 0x9E3779B97F4A7C15ull) >> 33) & mask; }

// The child (parent, tok) of the trie, or -1: linear probing from the key's slot to the first unused one.
SS_HD int ctc_beam_find(const unsigned long long* keys, const int* vals, int mask, int parent, int tok) {
  const unsigned long long key = ctc_beam_key(parent, tok);
  for (int s = ctc_beam_slot(key, mask), n = 0; n <= mask; ++n, s = (s + 1) & mask) {
    const unsigned long long k = keys[s];
    if (k == key) return vals[s];
    if (k == CTC_BEAM_EMPTY) return -1;
  }
  return -1;
}

// ---- the frame: what ctc_beam_search_body (ctc_beam.hip) and the twin (ctc_beam_host.hip) both call, on one layout ----
// The LM's lookup and its two rounding rules (ngram_lm.hpp, which includes this file: declared here, defined there).
struct NgramView;
SS_HD double ngram_lp(const NgramView& lm, int state, int c, int* next);
SS_HD double ngram_bonus(double parent, double lm_weight, double lp, double word_score);
SS_HD double ngram_finish(double fused, double lm_weight, double lp_eos);
// The phrase automaton's step and its rounding rules (ctc_bias.hpp, likewise).
struct BiasView;
SS_HD double bias_step(const BiasView& b, int state, int c, int* next);
SS_HD double bias_open(const BiasView& b, int state);
SS_HD double bias_bonus(double b1, double scale, double delta);
SS_HD double bias_finish(double fused, double scale, double open);

// The arrays a frame works on.  The kernel fills it once from its LDS arrays and its utterance's global pointers, the twin from
// vectors of the same names.  The current and the next beam are integer offsets co / no into the b_* arrays, passed to the
// functions and never folded into a pointer (ctc_align_trellis_kernel says why); each side has its own stride between the two.
struct CtcBeamFrame {
  double *b_pb, *b_pnb, *b_tot, *b_bonus; int *b_node, *b_last;   // the two beams (b_bonus: the LM form)
  double *s_pb, *s_pnb, *s_give;                                  // per entering prefix: what it keeps, what an extension hands it
  double *e_tot, *e_fus; int* e_node;                             // per entry (e_fus: the LM form)
  int* s_c; float *s_lpc, *s_lpl, *s_lp0;                         // the candidates, their lp, the lp of each last label, of the blank
  unsigned long long* keys; int* vals; int mask;                  // the child table
  double* n_bonus; int* n_state;                                  // per node (the LM form; n_bonus: the bias forms too)
  int* n_bstate;                                                  // per node (the bias forms)
};

// The bonus of the string parent + c that is not in the trie, from the parent's bonus and its node's states: the LM term, then the
// bias term, each where the form has it.
template <int FORM>
SS_HD double ctc_beam_ext_bonus(const CtcBeamFrame& F, double parent_bonus, int node, int c, const NgramView& lm, double lm_weight,
                                double word_score, const BiasView& bv, double bias_scale) {
  int nx;
  double b1 = parent_bonus;
  if constexpr ((FORM & CTC_FORM_LM) != 0) b1 = ngram_bonus(b1, lm_weight, ngram_lp(lm, F.n_state[node], c, &nx), word_score);
  if constexpr ((FORM & CTC_FORM_BIAS) != 0) b1 = bias_bonus(b1, bias_scale, bias_step(bv, F.n_bstate[node], c, &nx));
  return b1;
}

// Pass B for entry e = i * W + (k + 1) of a beam of nb prefixes: prefix i's own stay terms (k < 0; its total is pass C's), or the
// term of its extension by candidate k and that string's node from the child table -- an extension whose node is in the beam hands
// its term to that prefix and dies (one parent per string: one writer per s_give[j]).  The LM and bias forms add the entry's fused
// key.
template <int FORM>
SS_HD void ctc_beam_entry_b(const CtcBeamFrame& F, int co, int nb, int W, int e, const NgramView& lm, double lm_weight,
                            double word_score, const BiasView& bv, double bias_scale) {
  const int i = e / W, k = e - i * W - 1;
  const int node = F.b_node[co + i], last = F.b_last[co + i];
  if (k < 0) {
    double pb2, pnb2;
    ctc_beam_stay(F.b_pnb[co + i], F.b_tot[co + i], last, *F.s_lp0, F.s_lpl[i], &pb2, &pnb2);
    F.s_pb[i] = pb2; F.s_pnb[i] = pnb2;
    F.e_node[e] = node;
    return;
  }
  const int c = F.s_c[k];
  double term = -INFINITY;
  int child = -1;
  if (c >= 0) {
    term = ctc_beam_ext(F.b_pb[co + i], F.b_tot[co + i], last, c, F.s_lpc[k]);
    child = ctc_beam_find(F.keys, F.vals, F.mask, node, c);
    if (child >= 0) {
      for (int j = 0; j < nb; ++j) {
        if (F.b_node[co + j] == child) { F.s_give[j] = term; term = -INFINITY; break; }
      }
    }
  }
  F.e_tot[e] = term;
  F.e_node[e] = child;
  if constexpr (FORM != 0) {
    double fus = -INFINITY;
    if (term > -INFINITY)                                      // (a dead entry needs no bonus: no lookup)
      fus = term + (child >= 0 ? F.n_bonus[child]
                               : ctc_beam_ext_bonus<FORM>(F, F.b_bonus[co + i], node, c, lm, lm_weight, word_score, bv, bias_scale));
    F.e_fus[e] = fus;
  }
}

// Pass C for prefix i: pnb' = logadd(stay, handed term), its entry's total = logadd(pb', pnb') and, in the LM and bias forms, the
// fused key.
template <int FORM>
SS_HD void ctc_beam_entry_c(const CtcBeamFrame& F, int co, int W, int i) {
  const double pnb2 = ctc_beam_logadd(F.s_pnb[i], F.s_give[i]);
  F.s_pnb[i] = pnb2;
  const double tot = ctc_beam_logadd(F.s_pb[i], pnb2);
  F.e_tot[i * W] = tot;
  if constexpr (FORM != 0) F.e_fus[i * W] = tot > -INFINITY ? tot + F.b_bonus[co + i] : -INFINITY;
}

// A new string, parent + c, that takes rank `rank` of the beam leaving frame t: its id, its node with the form's fields (written
// once: the lookup of pass B again), and its place in the child table (never more than half full).  A frame's entries claim slots
// concurrently on the device and one after another on the host: the claim is the one line that differs.
template <int FORM>
SS_HD int ctc_beam_make_node(int t, int beam, int rank, int parent, int c, double parent_bonus, unsigned long long* keys, int* vals,
                             int mask, int2* nodes, double* n_sum, double* n_bonus, int* n_state, const NgramView& lm,
                             double lm_weight, double word_score, double* n_bsum, int* n_bstate, const BiasView& bv,
                             double bias_scale) {
  const int node = ctc_beam_new_node(t, beam, rank);
  nodes[node] = make_int2(parent, c);
  if constexpr (FORM == CTC_FORM_LM) {
    int nx;
    const double lp = ngram_lp(lm, n_state[parent], c, &nx);
    n_state[node] = nx;
    n_sum[node] = n_sum[parent] + lp;
    n_bonus[node] = ngram_bonus(parent_bonus, lm_weight, lp, word_score);
  } else if constexpr (FORM != 0) {
    int nx;
    double b1 = parent_bonus;
    if constexpr ((FORM & CTC_FORM_LM) != 0) {
      const double lp = ngram_lp(lm, n_state[parent], c, &nx);
      n_state[node] = nx;
      n_sum[node] = n_sum[parent] + lp;
      b1 = ngram_bonus(parent_bonus, lm_weight, lp, word_score);
    }
    const double delta = bias_step(bv, n_bstate[parent], c, &nx);
    n_bstate[node] = nx;
    n_bsum[node] = n_bsum[parent] + delta;
    n_bonus[node] = bias_bonus(b1, bias_scale, delta);
  }
  const unsigned long long key = ctc_beam_key(parent, c);
  for (int s = ctc_beam_slot(key, mask), n = 0; n <= mask; ++n, s = (s + 1) & mask) {
#ifdef __HIP_DEVICE_COMPILE__
    if (atomicCAS(&keys[s], CTC_BEAM_EMPTY, key) == CTC_BEAM_EMPTY) { vals[s] = node; break; }
#else
    if (keys[s] == CTC_BEAM_EMPTY) { keys[s] = key; vals[s] = node; break; }
#endif
  }
  return node;
}

// The string of a node, walked back through the trie: its tokens into out[0 .. len), its length returned.
SS_HD int ctc_beam_trace(const int2* nodes, int node, int* out) {
  int len = 0;
  for (int n = node; n > 0; n = nodes[n].x) ++len;
  int j = len;
  for (int n = node; n > 0 && j > 0; n = nodes[n].x) out[--j] = nodes[n].y;
  return len;
}

// The LM form's end for one prefix of the last beam: fin = (tot + bonus) and lm_sum = its node's sum, each with the eos term when
// eos >= 0 (the model's eos id; < 0: no eos term).  (Lm = NgramView: a template for the files that include this header without it.)
template <class Lm>
SS_HD void ctc_beam_finish(double tot, double bonus, double node_sum, int node_state, int eos, const Lm& lm, double lm_weight,
                           double* fin, double* lm_sum) {
  const double fused = tot + bonus;
  *fin = fused;
  *lm_sum = node_sum;
  if (eos >= 0) {
    int nx;
    const double lp = ngram_lp(lm, node_state, eos, &nx);
    *fin = ngram_finish(fused, lm_weight, lp);
    *lm_sum = node_sum + lp;
  }
}

// The bias forms' end for one prefix of the last beam, after the LM's: with `finish`, *fin -= scale * open(state) and *bias_sum =
// the node's sum - open(state); without, fin stays and *bias_sum = the node's sum.  (Bs = BiasView, as Lm above.)
template <class Bs>
SS_HD void ctc_beam_bias_finish(const Bs& bv, int b_state, double node_bsum, double bias_scale, bool finish, double* fin,
                                double* bias_sum) {
  *bias_sum = node_bsum;
  if (finish) {
    const double open = bias_open(bv, b_state);
    *fin = bias_finish(*fin, bias_scale, open);
    *bias_sum = node_bsum - open;
  }
}

// The depth of the lowest common ancestor of nodes a and b: the length of what the two strings start with (the stable-prefix pass).
SS_HD int ctc_beam_lca_depth(const int2* nodes, int a, int b) {
  int da = 0, db = 0;
  for (int n = a; n > 0; n = nodes[n].x) ++da;
  for (int n = b; n > 0; n = nodes[n].x) ++db;
  for (; da > db; --da) a = nodes[a].x;
  for (; db > da; --db) b = nodes[b].x;
  for (; a != b; --da) { a = nodes[a].x; b = nodes[b].x; }
  return da;
}

}  // namespace ss
