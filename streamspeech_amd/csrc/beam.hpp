// What the units of the text decoder's beam search and sampling share (the search itself: beam.hip):
//   beam_host.hip     the option readers, the constraint table, the planner of a call behind forced prefixes, the serial host twin of
//                     the constraint selection -- pure host code
//   beam_kernels.hip  the top-2k, merge, constraint-select, prefix-score and prefix-chain kernels, their launchers
//   beam_sample.hip   the sampling kernels and their launchers
//   beam.hip          the search driver with the feature-gather kernel only it launches, the ss_batch_mt_* entry points
// Each launcher picks the instantiation of its kernel family from the filled argument structs; the driver and the ss_op_* entries
// both go through it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/streamspeech_hip.h"
#include "common.hpp"

namespace ss {

constexpr int kMaxBeam = 32, kMaxCand = 2 * kMaxBeam;

// ---- lexical constraints (ss_batch_mt_beam_cons; the rule stands in include/streamspeech_hip.h) ----
// The ordered constraint state of a hypothesis is one int.  The CONS variants of the two step kernels are chosen by their launchers,
// as OPT and LENPEN are: the top-2k kernel bans </s> for an unfinished row and notes the scores of the row's at most two next tokens
// while it fills the row; the merge kernel runs cons_select between the rank merge and the step logic.
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

// ---- what the step kernels take ----
// One lock-step index of the R = B * k rows: the logits and the reference's masks (unity/sequence_generator.py:290-327).
struct RowStep {
  const float* logits = nullptr;   // [R][V]
  int V = 0, k = 0, t_step = 0, min_len = 0;
  const int *max_len = nullptr, *npre = nullptr;   // [B]
  const int* done = nullptr;       // [B]; the sampling step alone takes null
  const float* cum = nullptr;      // [R] cumulative scores the rows enter the step with (top-2k; the sampling step takes null)
  int pad = 0, unk = 0, eos = 0;
  float unk_pen = 0.f;
};

// OPT of the top-2k kernel, and the sampling step: temperature and the no-repeat ban (beam_rows.hpp).
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

// ss_mt_sample_opts as the step kernel takes it: read_sample_opts fills the first three, the caller the rest
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

// ---- what a search call carries on the host ----
// ss_mt_search_opts as the search uses it; the defaults are the search without options.
struct SearchOpts {
  int ngram = 0;
  float len_penalty = 1.f, temp = 1.f;
};

// The layout beam_continue_plan makes (beam_host.hip)
struct BcPlan {
  int pm = 0, S = 0, Smax = 0, c0 = 0, Tn = 0, Lc = 0, Np = 0, np_max = 0, nseg = 0, R = 0;
  std::vector<int> tab, tok0;
  size_t o_lself = 0, o_rowpos = 0, o_row0 = 0, o_pself = 0, o_pcross = 0, o_ptok = 0, o_plast = 0;
};

// The arguments of one ss_batch_mt_* search call (include/streamspeech_hip.h names them): each entry point fills the record once,
// the entries and the driver read it.  h_prefix / h_n_prefix are null for a search with no prefix anywhere.
struct SearchCall {
  ss_model* m; void* stream; int B, beam; const float* d_enc_out;
  const int32_t *h_Tp, *h_prefix, *h_n_prefix, *h_max_len;
  int min_len; float unk_penalty; int normalize;
  int32_t* h_out_tokens; int out_stride; int32_t* h_n_out;
  float *h_scores, *h_pos_scores, *d_feats; int feat_rows;
  const ss_mt_search_opts* opts;
  const int32_t *h_cons = nullptr, *h_cons_off = nullptr, *h_cons_end = nullptr;   // ss_batch_mt_beam_cons; no offsets: no constraints
  SearchOpts so;                                  // `opts` once read_search_opts has taken them
  SampleArgs smp;                                 // sampling in place of the beam: topk / topp / seed ...
  const int64_t* h_keys = nullptr;                // ... and the utterances' keys; null: the beam search
  const std::vector<int>* cons_tab = nullptr;     // the constraint table (cons_table), or null
};

// ---- beam_host.hip ----
int read_search_opts(const ss_mt_search_opts* o, SearchOpts& so);
int read_sample_opts(const ss_mt_sample_opts* o, const int64_t* h_keys, SampleArgs& sp);
int cons_table(int B, const int32_t* h_cons, const int32_t* h_off, const int32_t* h_end, int V, int pad, int eos,
               const int32_t* h_max_len, std::vector<int>& tab);
int beam_continue_plan(int B, int beam, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix,
                       const int32_t* h_max_len, int min_len, int out_stride, int feat_rows, int max_tgt_pos, int vocab, int eos,
                       int pad, int pm, BcPlan& P, int ngram = 0);
// the one place a TopkOpts is filled; anc (where it changes by the step) and row_scores are the caller's
TopkOpts topk_opts(const SearchOpts& so, int R, int Lc, int c0, const int* tok, const int* anc, const int* ptok, const int* row0);
int sample_npad(const SampleArgs& sp, int V);   // SampleArgs::npad

// ---- beam_kernels.hip ----
// dynamic LDS of the top-2k launch, and its refusal: an option or constraint row with its history and bit map past 64 KiB
int beam_topk_lds(int V, const TopkOpts& o, const ConsArgs* ca, size_t& bytes);
int launch_beam_topk(hipStream_t s, int R, const RowStep& a, float* cand_s, int* cand_t, const TopkOpts& o, const ConsArgs* ca);
int launch_beam_merge(hipStream_t s, int B, const BeamState& st, int k, int Lc, int V, int t_step, int c0, int eos, int normalize,
                      float len_penalty, const ConsArgs* ca);
int launch_beam_prefix_score(hipStream_t s, int rows, const float* logits, int V, const int* ftok, int pad, int unk, float unk_pen,
                             float* lp, float temp);
int launch_beam_prefix_chain(hipStream_t s, const float* lp, const int* row0, const int* npre, int B, int k, float* cum0, float* pos);

// ---- beam_sample.hip ----
// dynamic LDS of the sampling step, and its refusal
int sample_step_lds(int V, const TopkOpts& o, const SampleArgs& sp, size_t& bytes);
int launch_sample_step(hipStream_t s, int R, const RowStep& a, const TopkOpts& o, const SampleArgs& sp);
int launch_sample_advance(hipStream_t s, int B, const BeamState& st, int k, int Lc, int t_step, int c0, int eos, int normalize,
                          float len_penalty);

}  // namespace ss
