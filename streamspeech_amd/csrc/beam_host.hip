// Text search, host stage: the option readers, the constraint table, the planner of a call behind forced prefixes (every refusal
// that needs no model, in the documented order) and the serial host twin of the constraint selection.  Pure host code: no kernel,
// no HIP runtime call, no global state; tools/beam_host_check.cpp links this unit alone.
#include <algorithm>
#include <cmath>

#include "beam.hpp"

namespace ss {

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

// The refusals of the sampling entry points that need no model, in the documented order.
int read_sample_opts(const ss_mt_sample_opts* o, const int64_t* h_keys, SampleArgs& sp) {
  if (!o || o->size < (int32_t)sizeof(ss_mt_sample_opts)) return SS_ERR_ARG;
  if (o->topk < 0) return SS_ERR_ARG;
  if (!std::isfinite(o->topp) || o->topp < 0.f || o->topp > 1.f) return SS_ERR_ARG;
  if (o->topk > 0 && o->topp > 0.f) return SS_ERR_ARG;            // the reference silently prefers top-p
  if (!h_keys) return SS_ERR_ARG;
  sp.topk = o->topk; sp.topp = o->topp; sp.seed = o->seed;
  return SS_OK;
}

TopkOpts topk_opts(const SearchOpts& so, int R, int Lc, int c0, const int* tok, const int* anc, const int* ptok, const int* row0) {
  TopkOpts to;
  to.temp = so.temp; to.ngram = so.ngram; to.R = R; to.Lc = Lc; to.c0 = c0; to.tok = tok; to.anc = anc; to.ptok = ptok; to.row0 = row0;
  return to;
}

int sample_npad(const SampleArgs& sp, int V) {
  if (sp.topp == 0.f) return 0;                    // top-k selects without a sort
  int n = 1;
  while (n < V) n <<= 1;
  return n;
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
static bool prefix_repeats_ngram(const std::vector<int>& tokens, int ngram) {
  const int L = (int)tokens.size();
  for (int e = ngram; e < L; ++e)                                // a later n-gram tokens[e - ngram + 1 .. e] ...
    for (int i = 0; i + ngram - 1 < e; ++i)                      // ... against an earlier one tokens[i .. i + ngram - 1]
      if (std::equal(tokens.begin() + i, tokens.begin() + i + ngram, tokens.begin() + e - ngram + 1)) return true;
  return false;
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
int beam_continue_plan(int B, int beam, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix,
                       const int32_t* h_max_len, int min_len, int out_stride, int feat_rows, int max_tgt_pos, int vocab, int eos,
                       int pad, int pm, BcPlan& P, int ngram) {
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
  P.pm = pm; P.S = S; P.Smax = Smax; P.c0 = c0; P.Tn = Tn; P.Lc = Lc; P.Np = Np; P.np_max = np_max; P.nseg = nseg; P.R = R;
  const size_t np = (size_t)Np, nl = (size_t)(Tn + 1) * 4 * R;
  P.o_lself = 4 * (size_t)R; P.o_rowpos = P.o_lself + nl; P.o_row0 = P.o_rowpos + R; P.o_pself = P.o_row0 + B;
  P.o_pcross = P.o_pself + 4 * (size_t)nseg; P.o_ptok = P.o_pcross + 4 * (size_t)nseg; P.o_plast = P.o_ptok + 5 * np;
  P.tab.assign(P.o_plast + B, 0);
  P.tok0.assign(R, eos);
  int* cs = P.tab.data(); int* ls = cs + P.o_lself; int* rp = cs + P.o_rowpos; int* r0s = cs + P.o_row0; int* ps = cs + P.o_pself;
  int* pc = cs + P.o_pcross; int* pt = cs + P.o_ptok; int* pp = pt + np; int* pk = pp + np; int* pf = pk + np; int* ft = pf + np;
  int* pl = cs + P.o_plast;
  for (int b = 0, o = 0, row = 0, seg = 0, eoff = 0; b < B; eoff += h_Tp[b], ++b) {   // eoff: the utterance's first encoder row
    const int st = npre(b), npp = st + pm, sh = Smax - npp;
    for (int j = 0; j < k; ++j) {
      const int r = b * k + j;
      cs[4 * r] = r; cs[4 * r + 1] = 1; cs[4 * r + 2] = eoff; cs[4 * r + 3] = h_Tp[b];
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
      pc[4 * seg] = row; pc[4 * seg + 1] = npp; pc[4 * seg + 2] = eoff; pc[4 * seg + 3] = h_Tp[b];
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

}  // namespace ss

using namespace ss;

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
