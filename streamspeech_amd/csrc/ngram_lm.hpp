// A back-off n-gram language model for the CTC prefix beam search's shallow fusion (ngram_lm.hip, ctc_beam.hip): the table, its
// host builder (no kernel and no HIP call: tools/ngram_lm_host_check.cpp runs it under a sanitizer) and the lookup that the device
// kernels, the host twins and the score op share.
//
// A forward trie in ONE open-addressed table, the child table of ctc_beam.hpp read-only: entry 0 is the root (the empty context),
// the n-gram (w1 .. wk) is the child (entry of (w1 .. wk-1), wk); slots are a power of two >= 2 * entries, probing is linear
// (ctc_beam_key / _slot / _find as they are).  Values are natural logarithms, float32, taken as given.
//
// THE SCORING RULE, lp(c | state) -> (float64 value, new state):
//   acc = 0.0;  loop:  (state, c) is an entry e  -> acc + logp[e], next_state[e]
//                      state is the root         -> leave the loop
//                      else                      -> acc += backoff[state]; state = backoff_state[state]
//   at the root without a unigram for c: the model has a unigram for unk -> acc + logp[unk entry], next_state[unk entry]
//                                        else                             -> acc + oov_logp, the root
// which is ARPA back-off -- the longest context first, a context's back-off weight only where that context exists -- over states.
// A hypothesis starts in the state reached from the root by bos (when bos >= 0 and the model has that unigram; the root otherwise);
// the bos unigram's own probability is never scored.
#pragma once
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "ctc_beam.hpp"

namespace ss {

constexpr int NGRAM_MAX_ORDER = 6;
constexpr long long NGRAM_MAX_ENTRIES = 1LL << 30;

struct NgramEntry {
  float logp, backoff;   // backoff 0 where the file gives none
  int next_state;        // the longest suffix of the n-gram, at most order - 1 tokens long, that is an entry (may be the root)
  int backoff_state;     // the longest PROPER suffix that is an entry (the root for a unigram)
};

// What a lookup reads, host or device pointers alike.
struct NgramView {
  const unsigned long long* keys;
  const int* vals;
  const NgramEntry* ent;
  int mask, start, unk_entry, eos;   // unk_entry < 0: no unigram for unk
  double oov_logp;
};

SS_HD double ngram_lp(const NgramView& lm, int state, int c, int* next) {
  double acc = 0.0;
  for (;;) {
    const int e = ctc_beam_find(lm.keys, lm.vals, lm.mask, state, c);
    if (e >= 0) { *next = lm.ent[e].next_state; return acc + (double)lm.ent[e].logp; }
    if (state == 0) break;
    acc += (double)lm.ent[state].backoff;
    state = lm.ent[state].backoff_state;
  }
  if (lm.unk_entry >= 0) { *next = lm.ent[lm.unk_entry].next_state; return acc + (double)lm.ent[lm.unk_entry].logp; }
  *next = 0;
  return acc + lm.oov_logp;
}

// bonus[child] = bonus[parent] + ((lm_weight * lp) + word_score): three separately rounded float64 operations, in that order, on
// the device, in the twin and in tests/ctc_beam_lm_ref.py -- no compiler may contract the multiply and the add.
SS_HD double ngram_bonus(double parent, double lm_weight, double lp, double word_score) {
#pragma clang fp contract(off)
  const double m = lm_weight * lp;
  const double a = m + word_score;
  return parent + a;
}

// fin = fused + lm_weight * lp(eos | state): two rounded operations.
SS_HD double ngram_finish(double fused, double lm_weight, double lp_eos) {
#pragma clang fp contract(off)
  const double m = lm_weight * lp_eos;
  return fused + m;
}

// The model on the host: what ss_ngram_lm_create uploads, and what the host twins read.
struct NgramTable {
  int order = 0, V = 0, bos = -1, eos = -1, unk = -1;
  int entries = 0, mask = 0, start = 0, unk_entry = -1;
  float oov_logp = 0.f;
  std::vector<unsigned long long> keys;
  std::vector<int> vals;
  std::vector<NgramEntry> ent;
  NgramView view() const { return NgramView{keys.data(), vals.data(), ent.data(), mask, start, unk_entry, eos, (double)oov_logp}; }
  size_t table_bytes() const { return keys.size() * 12 + ent.size() * sizeof(NgramEntry); }
};

// The entry of the token string w[0 .. n), or -1.
inline int ngram_walk(const NgramTable& t, const int32_t* w, int n) {
  int s = 0;
  for (int j = 0; j < n && s >= 0; ++j) s = ctc_beam_find(t.keys.data(), t.vals.data(), t.mask, s, w[j]);
  return s;
}

// The checks, the trie, the two links and the slot placement.  n-grams grouped by order, ascending; order k holds counts[k - 1]
// rows of k ids.  SS_ERR_ARG (t is left empty): an order outside [1, NGRAM_MAX_ORDER], V <= 0, a negative count, bos / eos / unk
// outside [-1, V), an id outside [0, V), a duplicate n-gram, an n-gram whose context (itself minus its last token) is not an entry,
// a non-finite logp / backoff / oov_logp, more than 2^30 entries.  A missing SUFFIX is legal: the links skip it.
inline int ngram_build(int order, const int64_t* counts, const int32_t* tokens, const float* logp, const float* backoff, int V, int bos,
                       int eos, int unk, float oov_logp, NgramTable& t) {
  t = NgramTable();
  if (order < 1 || order > NGRAM_MAX_ORDER || !counts || V <= 0 || !std::isfinite(oov_logp)) return SS_ERR_ARG;
  if (bos < -1 || bos >= V || eos < -1 || eos >= V || unk < -1 || unk >= V) return SS_ERR_ARG;
  long long n = 0;
  for (int k = 0; k < order; ++k) {
    if (counts[k] < 0 || counts[k] > NGRAM_MAX_ENTRIES) return SS_ERR_ARG;
    n += counts[k];
  }
  if (1 + n > NGRAM_MAX_ENTRIES || (n > 0 && (!tokens || !logp || !backoff))) return SS_ERR_ARG;
  long long slots = 2;
  while (slots < 2 * (1 + n)) slots *= 2;
  NgramTable b;
  b.order = order; b.V = V; b.bos = bos; b.eos = eos; b.unk = unk; b.oov_logp = oov_logp;
  b.entries = (int)(1 + n); b.mask = (int)(slots - 1);
  b.keys.assign((size_t)slots, CTC_BEAM_EMPTY);
  b.vals.assign((size_t)slots, -1);
  b.ent.assign((size_t)b.entries, NgramEntry{0.f, 0.f, 0, 0});
  std::vector<long long> row_off((size_t)b.entries, 0);      // entry -> first id of its row in tokens
  std::vector<signed char> len((size_t)b.entries, 0);
  long long off = 0;
  int e = 1;
  for (int k = 1; k <= order; ++k) {
    for (int64_t r = 0; r < counts[k - 1]; ++r, ++e, off += k) {
      const int32_t* w = tokens + off;
      for (int j = 0; j < k; ++j)
        if (w[j] < 0 || w[j] >= V) return SS_ERR_ARG;
      if (!std::isfinite(logp[e - 1]) || !std::isfinite(backoff[e - 1])) return SS_ERR_ARG;
      const int ctx = ngram_walk(b, w, k - 1);
      if (ctx < 0 || ctc_beam_find(b.keys.data(), b.vals.data(), b.mask, ctx, w[k - 1]) >= 0) return SS_ERR_ARG;
      const unsigned long long key = ctc_beam_key(ctx, w[k - 1]);
      for (int s = ctc_beam_slot(key, b.mask);; s = (s + 1) & b.mask) {      // never more than half full: a free slot exists
        if (b.keys[s] == CTC_BEAM_EMPTY) { b.keys[s] = key; b.vals[s] = e; break; }
      }
      b.ent[e].logp = logp[e - 1]; b.ent[e].backoff = backoff[e - 1];
      row_off[e] = off; len[e] = (signed char)k;
    }
  }
  for (e = 1; e < b.entries; ++e) {
    const int32_t* w = tokens + row_off[e];
    const int k = len[e];
    int suf = 0;
    for (int j = 1; j < k; ++j) {                             // proper suffixes, the longest first
      const int s = ngram_walk(b, w + j, k - j);
      if (s >= 0) { suf = s; break; }
    }
    b.ent[e].backoff_state = suf;
    b.ent[e].next_state = k < order ? e : suf;
  }
  if (bos >= 0) {
    const int s = ctc_beam_find(b.keys.data(), b.vals.data(), b.mask, 0, bos);
    if (s >= 0) b.start = b.ent[s].next_state;
  }
  if (unk >= 0) b.unk_entry = ctc_beam_find(b.keys.data(), b.vals.data(), b.mask, 0, unk);
  t = std::move(b);
  return SS_OK;
}

// ss_ngram_score_host's loop, and the score kernel's: the n tokens of one sequence from the start state, then eos when asked.
SS_HD void ngram_score_seq(const NgramView& lm, const int32_t* tok, int n, int with_eos, double* lp, int32_t* state) {
  int s = lm.start;
  for (int j = 0; j < n + (with_eos ? 1 : 0); ++j) {
    int nx;
    lp[j] = ngram_lp(lm, s, j < n ? tok[j] : lm.eos, &nx);
    s = nx;
    if (state) state[j] = s;
  }
}

}  // namespace ss

// The handle of the C ABI (include/streamspeech_hip.h): the host table and its one upload (ngram_lm.hip: ngram_device_view).
struct ss_ngram_lm {
  ss::NgramTable host;
  std::mutex mu;                  // guards the upload alone: everything else is read-only
  void* d_mem = nullptr;          // keys [slots] u64 | entries [entries] NgramEntry | vals [slots] int
  size_t d_bytes = 0;             // the size of that buffer
  ss::NgramView dev{};
};

namespace ss {
int ngram_device_view(const ss_ngram_lm* lm, NgramView* out);   // the view over device pointers; uploads on the first call
}
