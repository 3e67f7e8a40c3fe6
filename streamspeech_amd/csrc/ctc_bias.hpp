// Hotword biasing for the CTC prefix beam search (ctc_bias.hip, ctc_beam.hip): a set of phrases to prefer, as a phrase automaton --
// the table, its host builder (no kernel and no HIP call: tools/ctc_bias_host_check.cpp runs it under a sanitizer) and the step
// that the device kernels, the host twins and the score op share.
//
// A bias set is P phrases of 1 .. CTC_BIAS_MAX_LEN token ids, each with a boost: a finite float32 in natural-log units, earned per
// token of the phrase, negative to discourage.  THE AUTOMATON: node 0 is the root (the empty string) and there is one node per
// distinct phrase prefix, the child (node of w1 .. wk-1, wk) in ONE open-addressed table, the child table of ctc_beam.hpp read-only
// (ctc_beam_key / _slot / _find as they are; slots a power of two >= 2 * nodes).  Per node n:
//   boost[n]     the largest boost of the phrases that pass through n
//   held[n]      held[parent] + (double)boost[n], summed root-down in float64: what a string that stands at n has been lent
//   floor[n]     held of the deepest node on the path root .. n (n included) that ends a phrase, 0 if none: what it keeps for good
//   fail[n]      the longest PROPER suffix of n's string that is a node (Aho-Corasick)
//
// THE SCORING RULE.  The state of a string y is the longest suffix of y that is a node.  On token c state s moves to n, the longest
// suffix of s + c that is a node (goto along the fail links), and the string earns
//   delta = held[n] - held[s]                   when n is s extended by c (a DIRECT move)
//   delta = (held[n] - held[s]) + floor[s]      otherwise: two separately rounded float64 operations, in that order
// so a partial match that breaks is paid back, except for what it earned up to the last phrase it completed, and the part of the
// suffix that still matches keeps its credit.  With open(s) = held[s] - floor[s], the bias of a FINISHED string is
// sum(delta) - open(state): an unfinished phrase earns nothing.
//
// A phrase may be a prefix of another ("new", "new york"); a phrase that occurs inside another one at a position other than its
// start is refused at creation.  With that restriction the finished bias of y is the sum of held[end(p)] over the occurrences
// (p, i) of phrases in y that are not a proper prefix of another occurrence starting at the same i (tests/ctc_bias_ref.py states both
// forms, and tests/test_ctc_bias_cpu.py holds one against the other).
#pragma once
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "ctc_beam.hpp"

namespace ss {

constexpr int CTC_BIAS_MAX_LEN = 32;
constexpr int CTC_BIAS_MAX_PHRASES = 4096;

struct BiasNode {
  float boost;
  int fail;
  double held;
  double floor;
  int terminal;          // 1: a phrase ends here
  int pad_;
};

// What a step reads, host or device pointers alike.
struct BiasView {
  const unsigned long long* keys;
  const int* vals;
  const BiasNode* node;
  int mask, pad_;
};

// state --c--> *next, the delta returned (the rule above).  A token that no phrase holds leads to the root.
SS_HD double bias_step(const BiasView& b, int state, int c, int* next) {
#pragma clang fp contract(off)
  const double held_s = b.node[state].held;
  int n = ctc_beam_find(b.keys, b.vals, b.mask, state, c);
  if (n >= 0) { *next = n; return b.node[n].held - held_s; }
  n = 0;
  for (int s = state; s != 0;) {
    s = b.node[s].fail;
    const int ch = ctc_beam_find(b.keys, b.vals, b.mask, s, c);
    if (ch >= 0) { n = ch; break; }
  }
  *next = n;
  const double d = b.node[n].held - held_s;
  return d + b.node[state].floor;
}

// What a string that stands at state s has been lent and does not keep when it ends there.
SS_HD double bias_open(const BiasView& b, int state) { return b.node[state].held - b.node[state].floor; }

// bonus[child] = b1 + (scale * delta): two separately rounded float64 operations, as ngram_bonus's.
SS_HD double bias_bonus(double b1, double scale, double delta) {
#pragma clang fp contract(off)
  const double m = scale * delta;
  return b1 + m;
}

// fin = fused - (scale * open(state)): two rounded operations.
SS_HD double bias_finish(double fused, double scale, double open) {
#pragma clang fp contract(off)
  const double m = scale * open;
  return fused - m;
}

// The automaton on the host: what the first device call uploads, and what the host twins read.
struct BiasTable {
  int V = 0, pad = -1, unk = -1, phrases = 0;
  int nodes = 0, mask = 0;
  std::vector<unsigned long long> keys;
  std::vector<int> vals;
  std::vector<BiasNode> node;
  BiasView view() const { return BiasView{keys.data(), vals.data(), node.data(), mask, 0}; }
  size_t table_bytes() const { return keys.size() * 12 + node.size() * sizeof(BiasNode); }
};

// The checks, the trie, held / floor, the fail links and the occurrence rule.  Phrase p is tokens[off[p] .. off[p + 1]) with
// boost[p].  SS_ERR_ARG (t is left empty): P outside [0, CTC_BIAS_MAX_PHRASES], V <= 0, pad / unk outside [-1, V), offsets that do
// not ascend from 0, an empty phrase or one longer than CTC_BIAS_MAX_LEN, an id outside [0, V), blank (0), pad or unk in a phrase,
// a duplicate phrase, a non-finite boost, a phrase that occurs inside another at a position other than its start.
inline int bias_build(int P, const int32_t* tokens, const int32_t* off, const float* boost, int V, int pad, int unk, BiasTable& t) {
  t = BiasTable();
  if (P < 0 || P > CTC_BIAS_MAX_PHRASES || V <= 0 || pad < -1 || pad >= V || unk < -1 || unk >= V) return SS_ERR_ARG;
  if (P > 0 && (!tokens || !off || !boost || off[0] != 0)) return SS_ERR_ARG;
  long long total = 0;
  for (int p = 0; p < P; ++p) {
    const long long len = (long long)off[p + 1] - off[p];
    if (len < 1 || len > CTC_BIAS_MAX_LEN || !std::isfinite(boost[p])) return SS_ERR_ARG;
    for (int j = off[p]; j < off[p + 1]; ++j)
      if (tokens[j] <= 0 || tokens[j] >= V || tokens[j] == pad || tokens[j] == unk) return SS_ERR_ARG;
    total += len;
  }
  long long slots = 2;
  while (slots < 2 * (1 + total)) slots *= 2;                  // (for the most nodes the phrases can make: never more than half full)
  BiasTable b;
  b.V = V; b.pad = pad; b.unk = unk; b.phrases = P;
  b.mask = (int)(slots - 1);
  b.keys.assign((size_t)slots, CTC_BEAM_EMPTY);
  b.vals.assign((size_t)slots, -1);
  b.node.reserve((size_t)(1 + total));
  b.node.push_back(BiasNode{0.f, 0, 0.0, 0.0, 0, 0});
  std::vector<int> parent(1, -1), tok(1, -1), depth(1, 0);
  for (int p = 0; p < P; ++p) {                                // the trie: a node's parent has the smaller id
    int s = 0;
    for (int j = off[p]; j < off[p + 1]; ++j) {
      int n = ctc_beam_find(b.keys.data(), b.vals.data(), b.mask, s, tokens[j]);
      if (n < 0) {
        n = (int)b.node.size();
        const unsigned long long key = ctc_beam_key(s, tokens[j]);
        for (int q = ctc_beam_slot(key, b.mask);; q = (q + 1) & b.mask) {
          if (b.keys[q] == CTC_BEAM_EMPTY) { b.keys[q] = key; b.vals[q] = n; break; }
        }
        b.node.push_back(BiasNode{boost[p], 0, 0.0, 0.0, 0, 0});
        parent.push_back(s); tok.push_back(tokens[j]); depth.push_back(depth[s] + 1);
      } else if (boost[p] > b.node[n].boost) {
        b.node[n].boost = boost[p];
      }
      s = n;
    }
    if (b.node[s].terminal) return SS_ERR_ARG;                 // a duplicate
    b.node[s].terminal = 1;
  }
  b.nodes = (int)b.node.size();
  long long fit = 2;
  while (fit < 2LL * b.nodes) fit *= 2;
  if (fit < slots) {                                           // shared prefixes made fewer nodes: the table of the header's size
    b.mask = (int)(fit - 1);
    b.keys.assign((size_t)fit, CTC_BEAM_EMPTY);
    b.vals.assign((size_t)fit, -1);
    for (int n = 1; n < b.nodes; ++n) {
      const unsigned long long key = ctc_beam_key(parent[n], tok[n]);
      for (int q = ctc_beam_slot(key, b.mask);; q = (q + 1) & b.mask) {
        if (b.keys[q] == CTC_BEAM_EMPTY) { b.keys[q] = key; b.vals[q] = n; break; }
      }
    }
  }
  std::vector<int> order;                                     // the nodes by depth: a fail link points to a shallower node
  order.reserve(b.node.size());
  for (int d = 1; d <= CTC_BIAS_MAX_LEN; ++d)
    for (int n = 1; n < b.nodes; ++n)
      if (depth[n] == d) order.push_back(n);
  std::vector<char> inside((size_t)b.nodes, 0);                // a phrase ends at a proper suffix of the node's string
  for (int n = 1; n < b.nodes; ++n) {                          // (ascending id: the parent first)
    BiasNode& e = b.node[n];
    e.held = b.node[parent[n]].held + (double)e.boost;
    e.floor = e.terminal ? e.held : b.node[parent[n]].floor;
  }
  for (int n : order) {
    int f = 0;
    if (depth[n] > 1) {
      for (int s = b.node[parent[n]].fail;; s = b.node[s].fail) {
        const int ch = ctc_beam_find(b.keys.data(), b.vals.data(), b.mask, s, tok[n]);
        if (ch >= 0) { f = ch; break; }
        if (s == 0) break;
      }
    }
    b.node[n].fail = f;
    inside[n] = f != 0 && (b.node[f].terminal || inside[f]);
    if (inside[n]) return SS_ERR_ARG;                          // the occurrence rule
  }
  t = std::move(b);
  return SS_OK;
}

// ss_ctc_bias_score_host's loop, and the score kernel's: the n tokens of one sequence from the root; delta / state per token (state
// may be NULL); *sum = the sum of the deltas in order, minus open(final state) when finish is set.
SS_HD void bias_score_seq(const BiasView& b, const int32_t* tok, int n, int finish, double* delta, int32_t* state, double* sum) {
  int s = 0;
  double acc = 0.0;
  for (int j = 0; j < n; ++j) {
    int nx;
    const double d = bias_step(b, s, tok[j], &nx);
    delta[j] = d;
    acc += d;
    s = nx;
    if (state) state[j] = s;
  }
  *sum = finish ? acc - bias_open(b, s) : acc;
}

}  // namespace ss

// The handle of the C ABI (include/streamspeech_hip.h): the host table and its one upload (ctc_bias.hip: bias_device_view).
struct ss_ctc_bias {
  ss::BiasTable host;
  std::mutex mu;                  // guards the upload alone: everything else is read-only
  void* d_mem = nullptr;          // keys [slots] u64 | nodes [nodes] BiasNode | vals [slots] int
  size_t d_bytes = 0;             // the size of that buffer
  ss::BiasView dev{};
};

namespace ss {
int bias_device_view(const ss_ctc_bias* bias, BiasView* out);   // the view over device pointers; uploads on the first call
}
