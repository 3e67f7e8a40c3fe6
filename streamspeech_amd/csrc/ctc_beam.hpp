// CTC prefix beam search on the two text heads (ctc_beam.hip): what the device search and its host twin (ss_ctc_beam_host) share --
// the limits, the argument checks, the table of a ragged pack, the trie's child lookup and the step code.
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
#pragma once
#include <stdint.h>

#include <vector>

#include "ctc_align.hpp"

namespace ss {

constexpr int CTC_BEAM_MAX_BEAM = 32;
constexpr int CTC_BEAM_MAX_CAND = 32;
constexpr int CTC_BEAM_MAX_T = CTC_ALIGN_MAX_T;
constexpr int CTC_BEAM_MAX_ENT = CTC_BEAM_MAX_BEAM * (CTC_BEAM_MAX_CAND + 1);
constexpr unsigned long long CTC_BEAM_EMPTY = ~0ull;        // an unused slot of the child table (the buffer is filled with 0xff)

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
};

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
    long long slots = 2;
    while (slots < 2LL * beam * T) slots *= 2;
    p.segs[b] = CtcBeamSeg{p.nodes, p.slots, p.rows, T, (int)(slots - 1), 0};
    p.nodes += 1 + (long long)beam * T;
    p.slots += slots;
    p.rows += T;
    if (T > p.max_T) p.max_T = T;
  }
  return SS_OK;
}

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

}  // namespace ss
