// CTC forced alignment of a GIVEN label sequence on the two text heads (ctc_align.hip): what the device trellis and its host twin
// (ss_ctc_align_host) share -- the limits, the argument checks, the table of a ragged pack and the transition code.
//
// The extended sequence of labels y[0..L) is e = [0, y0, 0, y1, ..., y(L-1), 0], S = 2L + 1 states (blank = 0).  State s at frame t is
// reached from s (stay), s - 1 (advance) and, for a label state whose label differs from the label before it, s - 2 (skip the blank).
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#include "common.hpp"

namespace ss {

constexpr int CTC_ALIGN_MAX_T = 1500;                       // max_source_positions = 6000 fbank frames / 4
constexpr int CTC_ALIGN_MAX_L = 1500;                       // L <= T' (more labels than frames is legal, and infeasible, up to here)
constexpr int CTC_ALIGN_MAX_S = 2 * CTC_ALIGN_MAX_L + 1;    // two float64 state vectors of it + the labels: 54 024 bytes of LDS

// One utterance of a pack, as both kernels read it (device) and the host twin walks it.
struct CtcAlignSeg {
  long long lp_off;     // first float of its per-frame values lp[T][L + 1] (column 0 the blank, column 1 + j label j) in the work buffer
  long long bp_off;     // first byte of its back-pointers [T][(S + 3) / 4], 2 bits per state
  int row0, T;          // packed frame rows [row0, row0 + T)
  int lab0, L;          // packed labels [lab0, lab0 + L)
};

struct CtcAlignPlan {
  std::vector<CtcAlignSeg> segs;
  long long lp_floats = 0, bp_bytes = 0;
  int rows = 0, labels = 0, max_S = 0, max_L = 0;
  size_t work_bytes() const { return (size_t)lp_floats * sizeof(float) + (size_t)bp_bytes; }
};

// Every refusal of the three entry points past their pointers, before anything is launched or written: B <= 0, a T' outside
// [1, CTC_ALIGN_MAX_T], an L outside [0, CTC_ALIGN_MAX_L], a label that is blank (0), pad, negative or >= V.
inline int ctc_align_plan(int V, int pad, int B, const int32_t* h_T, const int32_t* h_targets, const int32_t* h_n, CtcAlignPlan& p) {
  if (V <= 0 || B <= 0 || !h_T || !h_n) return SS_ERR_ARG;
  p.segs.resize(B);
  for (int b = 0; b < B; ++b) {
    const int T = h_T[b], L = h_n[b];
    if (T < 1 || T > CTC_ALIGN_MAX_T || L < 0 || L > CTC_ALIGN_MAX_L || (L > 0 && !h_targets)) return SS_ERR_ARG;
    for (int j = 0; j < L; ++j) {
      const int y = h_targets[p.labels + j];
      if (y <= 0 || y >= V || y == pad) return SS_ERR_ARG;
    }
    const int S = 2 * L + 1;
    p.segs[b] = CtcAlignSeg{p.lp_floats, p.bp_bytes, p.rows, T, p.labels, L};
    p.lp_floats += (long long)T * (L + 1);
    p.bp_bytes += (long long)T * ((S + 3) / 4);
    p.rows += T; p.labels += L;
    if (S > p.max_S) p.max_S = S;
    if (L > p.max_L) p.max_L = L;
  }
  return SS_OK;
}

#define SS_HD __host__ __device__ __forceinline__

// log(e^a + e^b + e^c) in float64; -inf operands are exact zeros, three -inf give -inf.
SS_HD double ctc_align_logadd3(double a, double b, double c) {
  const double m = fmax(a, fmax(b, c));
  if (!(m > -INFINITY)) return m;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}

// The max-plus transition and its tie rule: stay beats advance, advance beats skip.  -> the best predecessor's value, *back = how
// many states below s it lies (0 stay, 1 advance, 2 skip).
SS_HD double ctc_align_best3(double stay, double adv, double skip, int* back) {
  double v = stay; int k = 0;
  if (adv > v) { v = adv; k = 1; }
  if (skip > v) { v = skip; k = 2; }
  *back = k;
  return v;
}

// May state s (odd, >= 3) be entered from s - 2: two different labels around the blank.
SS_HD bool ctc_align_can_skip(const int32_t* y, int s) { return (s & 1) && s >= 3 && y[s >> 1] != y[(s >> 1) - 1]; }

// The end of a path: the trailing blank state S - 1 beats the last label S - 2 on equality.
SS_HD int ctc_align_end_state(double v_blank, double v_label, int S) { return (S >= 2 && v_label > v_blank) ? S - 2 : S - 1; }

// Column of state s in an utterance's lp rows.
SS_HD int ctc_align_col(int s) { return (s & 1) ? 1 + (s >> 1) : 0; }

}  // namespace ss
