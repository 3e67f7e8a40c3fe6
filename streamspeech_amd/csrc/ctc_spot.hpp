// Keyword spotting on the two text CTC heads (ctc_spot.hip): what the device kernels and the host twins (ss_ctc_spot_host,
// ss_ctc_spot_stream_advance_host) share -- the limits, the keyword set's table and its builder, the one step of the max-plus
// recursion and the one statement of the emission rule.  THE RULE is written out in include/streamspeech_hip.h at ss_batch_ctc_spot.
//
// A keyword of labels y[0..L) has the states [y0, 0, y1, 0, ..., y(L-1)], S = 2L - 1 (no leading or trailing blank): state s is label
// y[s / 2] for even s and the blank for odd s.  State s of the aligner's layout is state s - 1 here, so its transition code
// (ctc_align_best3, ctc_align_can_skip) is used as it stands.
#pragma once
#include <stdint.h>

#include <cmath>
#include <mutex>
#include <vector>

#include "../../include/streamspeech_hip.h"
#include "common.hpp"
#include "ctc_align.hpp"

namespace ss {

constexpr int CTC_SPOT_MAX_L = SS_CTC_SPOT_MAX_LABELS;      // labels per keyword: S <= 63, a keyword never straddles a wave
constexpr int CTC_SPOT_LANES = 256;                         // lanes (states) a workgroup of the DP kernel owns: four waves
constexpr int CTC_SPOT_STAGE = 16;                          // frames of the compact matrix a workgroup stages in LDS at a time
constexpr int CTC_SPOT_COLS = 260;                          // columns a workgroup can need (256 one-label keywords + the blank), padded

// One lane of the DP kernel.  kw < 0: an idle lane (the tail of a wave no further keyword fits in).
struct SpotLane {
  int32_t kw;        // keyword
  int32_t sidx;      // its state's place among all states of the set (state0[kw] + s): where a stream slot keeps it
  int16_t s, S;      // state, states of the keyword
  int16_t col;       // the state's column among its WORKGROUP's columns (SpotTable::cols)
  int16_t skip;      // 1: may be entered from s - 2
};
struct SpotKw {
  double thr;        // -(double)tau * L: a frame is a candidate when e >= thr
  int32_t L, state0;
};
// One utterance (session) of a call, as the kernels read it.
struct SpotSess {
  int32_t slot;      // stream slot (the one-shot calls: unused)
  int32_t row0;      // its first row in the compact matrix of the call
  int32_t f, upto;   // the frames [f, upto) move; f == 0: a fresh state
  int32_t fin;       // the utterance's last call: the pending candidate is emitted, nothing is kept
  int32_t reserved;
};
// A pending candidate and the end of the last emitted hit.  end < 0: none pending; last_end < 0: nothing emitted yet.
struct SpotPend {
  double score;
  int32_t start, end, last_end;
};

struct SpotView {
  const SpotKw* kws;
  const SpotLane* lanes;     // [G][CTC_SPOT_LANES]
  const int32_t* labels;     // [U] the set's distinct labels, ascending; labels[0] = 0, the blank
  const int32_t* cols;       // [G][CTC_SPOT_COLS] a workgroup's columns as indices into labels
  const int32_t* ncols;      // [G]
  int32_t K, U, G, NS;
};

struct SpotTable {
  std::vector<SpotKw> kws;
  std::vector<SpotLane> lanes;
  std::vector<int32_t> labels, cols, ncols;
  std::vector<int32_t> su;   // [NS] per state its index into labels (the host twin walks keywords, not lanes)
  std::vector<int32_t> tok, off;
  int K = 0, U = 0, G = 0, NS = 0;
  size_t table_bytes() const {
    return kws.size() * sizeof(SpotKw) + lanes.size() * sizeof(SpotLane) + (labels.size() + cols.size() + ncols.size()) * sizeof(int32_t);
  }
  SpotView view() const { return SpotView{kws.data(), lanes.data(), labels.data(), cols.data(), ncols.data(), K, U, G, NS}; }
};

// Every refusal of ss_ctc_spot_set_create, then the table.  Keywords are laid onto lanes in their given order: a keyword takes S
// consecutive lanes of one wave; where it does not fit in what is left of the wave it starts the next one.  Four waves are a
// workgroup.  What a lane computes depends on its own keyword's lanes alone, so the layout changes no result.
inline int spot_build(int n, const int32_t* tok, const int32_t* off, const float* tau, int V, int pad, int unk, SpotTable& t) {
  if (n <= 0 || n > SS_CTC_SPOT_MAX_KEYWORDS || !tok || !off || !tau || V <= 0 || pad < -1 || pad >= V || unk < -1 || unk >= V || off[0] != 0)
    return SS_ERR_ARG;
  for (int k = 0; k < n; ++k) {
    const int L = off[k + 1] - off[k];
    if (L < 1 || L > CTC_SPOT_MAX_L || !(tau[k] >= 0.f) || !std::isfinite(tau[k])) return SS_ERR_ARG;
    for (int j = off[k]; j < off[k + 1]; ++j)
      if (tok[j] <= 0 || tok[j] >= V || tok[j] == pad) return SS_ERR_ARG;
  }
  t.K = n;
  t.tok.assign(tok, tok + off[n]);
  t.off.assign(off, off + n + 1);
  std::vector<int32_t> u_of(V, -1);
  u_of[0] = 0;
  for (int32_t y : t.tok) u_of[y] = 0;
  t.labels.clear();
  for (int v = 0; v < V; ++v)
    if (u_of[v] == 0) { u_of[v] = (int32_t)t.labels.size(); t.labels.push_back(v); }
  t.U = (int)t.labels.size();
  t.kws.resize(n);
  int lane = 0;                                               // next free lane, counted over all workgroups
  for (int k = 0; k < n; ++k) {
    const int L = off[k + 1] - off[k], S = 2 * L - 1;
    const int32_t* y = tok + off[k];
    if ((lane & 63) + S > 64) lane = (lane + 63) & ~63;
    t.kws[k] = SpotKw{-(double)tau[k] * L, L, t.NS};
    t.lanes.resize((size_t)(lane + S + CTC_SPOT_LANES - 1) / CTC_SPOT_LANES * CTC_SPOT_LANES, SpotLane{-1, 0, 0, 0, 0, 0});
    for (int s = 0; s < S; ++s) {
      t.lanes[lane + s] = SpotLane{k, t.NS + s, (int16_t)s, (int16_t)S, 0, (int16_t)(ctc_align_can_skip(y, s + 1) ? 1 : 0)};
      t.su.push_back((s & 1) ? 0 : u_of[y[s >> 1]]);
    }
    lane += S;
    t.NS += S;
  }
  t.G = (int)(t.lanes.size() / CTC_SPOT_LANES);
  t.cols.assign((size_t)t.G * CTC_SPOT_COLS, 0);
  t.ncols.assign(t.G, 0);
  std::vector<int32_t> where(t.U);
  for (int g = 0; g < t.G; ++g) {
    std::fill(where.begin(), where.end(), -1);
    int nc = 0;
    for (int l = 0; l < CTC_SPOT_LANES; ++l) {
      SpotLane& ln = t.lanes[(size_t)g * CTC_SPOT_LANES + l];
      if (ln.kw < 0) continue;
      const int u = t.su[ln.sidx];
      if (where[u] < 0) { where[u] = nc; t.cols[(size_t)g * CTC_SPOT_COLS + nc] = u; ++nc; }
      ln.col = (int16_t)where[u];
    }
    t.ncols[g] = nc;                                           // <= 257: at most one new column per lane, and the blank
  }
  return SS_OK;
}

// The per-frame cost of a row on the host, as the gather kernel computes it: c[u] = row[labels[u]] - max(row), one float32
// subtraction.  -> the row is bad (a NaN in it, or its maximum is -inf): the utterance's status becomes 2.
inline bool spot_row_host(const float* r, int N, const SpotTable& t, float* c) {
  float mx = -INFINITY;
  bool nan = false;
  for (int n = 0; n < N; ++n) { nan |= r[n] != r[n]; mx = fmaxf(mx, r[n]); }
  for (int u = 0; u < t.U; ++u) c[u] = r[t.labels[u]] - mx;
  return nan || !(mx > -INFINITY);
}

// ONE STEP of the recursion for state s at frame t (absolute in the utterance).  (a0, b0), (a1, b1), (a2, b2): value and start frame
// of the states s, s - 1, s - 2 after frame t - 1 (-inf before the first frame; whatever for a state that does not exist: it is
// not read).  x = c[t][label(s)].  State 0 stays, or is entered with value 0.0 and start t; stay wins on equality, and as c <= 0
// that is only while the first label has been the arg-max since its start.
SS_HD void ctc_spot_step(int s, bool can_skip, double x, int t, double a0, int b0, double a1, int b1, double a2, int b2, double* na,
                         int* nb) {
  if (s == 0) {
    const bool stay = a0 >= 0.0;
    *na = (stay ? a0 : 0.0) + x;
    *nb = stay ? b0 : t;
    return;
  }
  int back = 0;
  const double v = ctc_align_best3(a0, a1, can_skip ? a2 : -INFINITY, &back);
  *na = v + x;
  *nb = back == 0 ? b0 : (back == 1 ? b1 : b2);
}

// THE EMISSION RULE of one keyword at frame t, after its step: e = a[t][S - 1] with start st, cand = e >= thr.  -> a hit left the
// pending slot (*out holds it: score, start, end).
SS_HD bool ctc_spot_emit(SpotPend& p, bool cand, double e, int st, int t, SpotPend* out) {
  if (cand && st <= p.last_end) return false;                 // it begins inside what was already reported: ignored, P stays
  if (cand && p.end >= 0 && st <= p.end) {                    // it overlaps P: the better of the two, the later on equality
    if (e >= p.score) { p.score = e; p.start = st; p.end = t; }
    return false;
  }
  const bool emit = p.end >= 0;
  if (emit) { *out = p; p.last_end = p.end; }
  if (cand) { p.score = e; p.start = st; p.end = t; } else p.end = -1;
  return emit;
}

SS_HD bool ctc_spot_hit_less(const ss_ctc_hit& x, const ss_ctc_hit& y) {
  if (x.end != y.end) return x.end < y.end;
  if (x.keyword != y.keyword) return x.keyword < y.keyword;
  return x.start < y.start;
}

// What a stream slot keeps on the device, carved from one buffer: per state a (float64) and start, per keyword P and last_end, and
// the slot's sticky status -- 12 NS + 20 K + 4 bytes per slot.
struct SpotState {
  double* a;         // [slots][NS]
  double* pscore;    // [slots][K]
  int32_t* b;        // [slots][NS]
  int32_t* pstart;   // [slots][K]
  int32_t* pend;
  int32_t* plast;
  int32_t* status;   // [slots]
};
inline size_t spot_state_bytes(int slots, int NS, int K) {
  return ((size_t)slots * (12 * (size_t)NS + 20 * (size_t)K + 4) + 7) & ~(size_t)7;
}
inline SpotState spot_state_carve(void* p, int slots, int NS, int K) {
  SpotState st;
  st.a = static_cast<double*>(p);
  st.pscore = st.a + (size_t)slots * NS;
  st.b = reinterpret_cast<int32_t*>(st.pscore + (size_t)slots * K);
  st.pstart = st.b + (size_t)slots * NS;
  st.pend = st.pstart + (size_t)slots * K;
  st.plast = st.pend + (size_t)slots * K;
  st.status = st.plast + (size_t)slots * K;
  return st;
}

// The same state on the host (the twins).
struct SpotHostState {
  std::vector<double> a;
  std::vector<int32_t> b;
  std::vector<SpotPend> p;
  int status = 0;
  void start(int NS, int K) {
    a.assign(NS, -INFINITY);
    b.assign(NS, -1);
    p.assign(K, SpotPend{0.0, -1, -1, -1});
    status = 0;
  }
};

// The frames [f, upto) of one utterance on the host: rows = its (upto - f) logits rows.  Appends the hits in emission order.
// tr_e / tr_s (may be NULL): [upto - f][K], every keyword's e_t and s_t after each frame.
inline void spot_host_run(const SpotTable& t, const float* rows, int ld, int V, int f, int upto, bool fin, SpotHostState& st,
                          std::vector<ss_ctc_hit>& hits, double* tr_e = nullptr, int32_t* tr_s = nullptr) {
  std::vector<float> c((size_t)(upto - f) * t.U);
  for (int i = 0; i < upto - f; ++i)
    if (spot_row_host(rows + (size_t)i * ld, V, t, c.data() + (size_t)i * t.U)) st.status = 2;
  if (st.status == 2) return;
  for (int fr = f; fr < upto; ++fr) {
    const float* cr = c.data() + (size_t)(fr - f) * t.U;
    for (int k = 0; k < t.K; ++k) {
      const SpotKw& kw = t.kws[k];
      const int S = 2 * kw.L - 1;
      double* a = st.a.data() + kw.state0;
      int32_t* b = st.b.data() + kw.state0;
      const int32_t* y = t.tok.data() + t.off[k];
      for (int s = S - 1; s >= 0; --s)                         // descending: a[s - 1], a[s - 2] are still frame fr - 1's
        ctc_spot_step(s, ctc_align_can_skip(y, s + 1), (double)cr[t.su[kw.state0 + s]], fr, a[s], b[s], s >= 1 ? a[s - 1] : -INFINITY,
                      s >= 1 ? b[s - 1] : -1, s >= 2 ? a[s - 2] : -INFINITY, s >= 2 ? b[s - 2] : -1, &a[s], &b[s]);
      if (tr_e) tr_e[(size_t)(fr - f) * t.K + k] = a[S - 1];
      if (tr_s) tr_s[(size_t)(fr - f) * t.K + k] = b[S - 1];
      SpotPend out;
      if (ctc_spot_emit(st.p[k], a[S - 1] >= kw.thr, a[S - 1], b[S - 1], fr, &out))
        hits.push_back(ss_ctc_hit{k, out.start, out.end, kw.L, out.score});
    }
  }
  if (fin)
    for (int k = 0; k < t.K; ++k)
      if (st.p[k].end >= 0) hits.push_back(ss_ctc_hit{k, st.p[k].start, st.p[k].end, t.kws[k].L, st.p[k].score});
}

}  // namespace ss

struct ss_ctc_spot_set {
  ss::SpotTable host;
  int V = 0, pad = -1, unk = -1;
  std::mutex mu;                  // guards the upload alone: everything else is read-only
  void* d_mem = nullptr;          // kws | lanes | labels | cols | ncols
  int device = -1;                // the device d_mem lives on: the one that was current at the first device call
  size_t d_bytes = 0;
  ss::SpotView dev{};
};

namespace ss {
int spot_device_view(const ss_ctc_spot_set* set, SpotView* out);   // the view over device pointers; uploads on the first call
size_t spot_work_bytes(const ss_ctc_spot_set* set, int rows, int n, int max_hits);   // compact matrix | sort copy | sessions | row table
// memset of the counts, the gather kernel over the call's `rows` logits rows, the DP kernel, the sort kernel.  state: a stream
// object's slots, or null pointers (the one-shot calls: every session fresh and final).
int launch_ctc_spot(const ss_ctc_spot_set* set, const float* logits, int ld, int rows, int n, const SpotSess* h_sess, void* d_work,
                    const SpotState& state, int max_hits, ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts, hipStream_t stream);
}
