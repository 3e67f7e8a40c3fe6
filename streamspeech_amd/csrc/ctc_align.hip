// CTC forced alignment and scoring of a given label sequence on the two text CTC heads (blank = 0): where do these labels lie in
// this audio, and how likely does the model find them -- the complement of the scored greedy search (ctc_scores.hip), for a ragged
// pack.  Two kernels:
//   ctc_align_lp_kernel       per packed frame row the plain log-softmax (no pad / unk masking: the criterion's log_softmax, so a word
//                             mapped to <unk> can still be placed) gathered at the utterance's states, float32
//   ctc_align_trellis_kernel  one workgroup per utterance, threads over the 2L + 1 states: the forward sum (log p(y | x)), the
//                             max-plus pass with 2-bit back-pointers, the back-trace, and per label its run on the path
// plus the plain-C++ twin of both (ss_ctc_align_host) over the same transition code (ctc_align.hpp).
#include "ctc_align.hpp"

#include <cstring>

#include "../../include/streamspeech_hip.h"
#include "ctc_row.hpp"
#include "elementwise.hpp"

namespace ss {

// One logits row per workgroup.  The denominator is ctc_row.hpp's, the greedy search's and the beam search's -- so the suite's 2e-5
// bound against the float64 log-softmax holds for every value written here, and a row's values are a function of that row's bits
// and its utterance's labels alone.  lp[t][0] = blank, lp[t][1 + j] = label j; a row that holds a NaN gives NaN in
// every column (as torch.log_softmax), which is how the trellis learns of it.
__global__ __launch_bounds__(256) void ctc_align_lp_kernel(const float* __restrict__ logits, int ld, int N,
                                                           const CtcAlignSeg* __restrict__ segs, int B,
                                                           const int* __restrict__ labels, float* __restrict__ lp) {
  __shared__ float sm[4], ssum[4];
  __shared__ int sn[4];
  const int t = threadIdx.x;
  const int row = blockIdx.x;
  int lo = 0, hi = B - 1;                                      // the utterance of this row: row0 ascends strictly (every T >= 1)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs[mid].row0 <= row) lo = mid; else hi = mid - 1;
  }
  const CtcAlignSeg sg = segs[lo];
  const float* r = logits + (size_t)row * ld;
  float v[1];                                                  // (the re-reading form: any N)
  const float mx = ctc_row_max<0>(r, N, v, sm, sn);
  ctc_row_expsum<0>(r, N, v, mx, ssum);
  const float lt = ctc_row_logsum(ssum);
  const bool bad = ctc_row_nan(sn);
  float* out = lp + sg.lp_off + (long long)(row - sg.row0) * (sg.L + 1);
  const int* y = labels + sg.lab0;
  for (int j = t; j <= sg.L; j += 256) out[j] = bad ? __builtin_nanf("") : (r[j ? y[j - 1] : 0] - mx) - lt;
}

// One utterance per workgroup, thread i on states i, i + 256, ...  Dynamic LDS: two float64 state vectors [max_S] (double-buffered:
// frame t reads one and writes the other, one barrier per frame), the labels [max_L], the path's states [max_T].  Both passes read
// the same lp; every operation of an utterance happens in one fixed order inside its own workgroup, so its results are the same
// bits alone and at any place of any pack.  The back-pointer of (t, s) is how many states below s the best predecessor lies (tie
// rule: ctc_align_best3), four states to a byte, packed across lanes before the store.
__global__ __launch_bounds__(256) void ctc_align_trellis_kernel(const CtcAlignSeg* __restrict__ segs, const int* __restrict__ labels,
                                                                int max_S, int max_L, const float* __restrict__ lp_all,
                                                                unsigned char* __restrict__ bp_all, ss_ctc_align_result* results,
                                                                int* path, int* first, int* last, float* tok_lprob,
                                                                float* frame_lprob) {
  extern __shared__ double sh[];
  __shared__ int s_status;
  // the two state vectors are addressed as sh[o + s] with an integer offset o = 0 | max_S, never through a pointer picked at run
  // time: such a pointer is a generic one, its loads become FLAT instructions, and the hardware chooses a FLAT access's aperture
  // from the register address alone -- and the compiler keeps &vector[s - 2] as the base of all three loads, which lies below the LDS aperture for s < 2
  int* y = reinterpret_cast<int*>(sh + 2 * (size_t)max_S);
  int* st = y + max_L;
  const int tid = threadIdx.x;
  const CtcAlignSeg sg = segs[blockIdx.x];
  const int T = sg.T, L = sg.L, S = 2 * L + 1, W = L + 1, stride = (S + 3) / 4;
  const float* lp = lp_all + sg.lp_off;
  unsigned char* bp = bp_all + sg.bp_off;
  for (int j = tid; j < L; j += 256) y[j] = labels[sg.lab0 + j];
  for (int s = tid; s < S; s += 256) sh[s] = s < 2 ? (double)lp[ctc_align_col(s)] : -INFINITY;
  bool nan = tid == 0 && lp[0] != lp[0];
  __syncthreads();
  // ---- forward sum ----
  for (int t = 1; t < T; ++t) {
    const int po = ((t - 1) & 1) * max_S, no = (t & 1) * max_S;
    const float* row = lp + (long long)t * W;
    if (tid == 0) nan |= row[0] != row[0];
    for (int s = tid; s < S; s += 256) {
      const double adv = s >= 1 ? sh[po + s - 1] : -INFINITY;
      const double skip = ctc_align_can_skip(y, s) ? sh[po + s - 2] : -INFINITY;
      sh[no + s] = ctc_align_logadd3(sh[po + s], adv, skip) + (double)row[ctc_align_col(s)];
    }
    __syncthreads();
  }
  double score = 0.0;
  if (tid == 0) {
    const double* fin = sh + ((T - 1) & 1) * max_S;
    score = ctc_align_logadd3(fin[S - 1], S >= 2 ? fin[S - 2] : -INFINITY, -INFINITY);
  }
  __syncthreads();
  // ---- max-plus pass ----
  for (int s = tid; s < S; s += 256) sh[s] = s < 2 ? (double)lp[ctc_align_col(s)] : -INFINITY;
  __syncthreads();
  for (int t = 1; t < T; ++t) {
    const int po = ((t - 1) & 1) * max_S, no = (t & 1) * max_S;
    const float* row = lp + (long long)t * W;
    unsigned char* brow = bp + (long long)t * stride;
    for (int s0 = 0; s0 < S; s0 += 256) {                      // uniform trip count: the shuffles below need every lane
      const int s = s0 + tid;
      int back = 0;
      if (s < S) {
        const double adv = s >= 1 ? sh[po + s - 1] : -INFINITY;
        const double skip = ctc_align_can_skip(y, s) ? sh[po + s - 2] : -INFINITY;
        sh[no + s] = ctc_align_best3(sh[po + s], adv, skip, &back) + (double)row[ctc_align_col(s)];
      }
      const int four = back | (__shfl_down(back, 1, 64) << 2) | (__shfl_down(back, 2, 64) << 4) | (__shfl_down(back, 3, 64) << 6);
      if (s < S && (tid & 3) == 0) brow[s >> 2] = (unsigned char)four;
    }
    __syncthreads();                                           // (also orders the back-pointer stores before the back-trace's loads)
  }
  // ---- the end of the path, the record, the back-trace (thread 0 of wave 0 walks; the block writes) ----
  if (tid == 0) {
    const double* fin = sh + ((T - 1) & 1) * max_S;
    const int end = ctc_align_end_state(fin[S - 1], S >= 2 ? fin[S - 2] : -INFINITY, S);
    double vit = fin[end];
    const int status = nan ? 2 : (vit > -INFINITY ? 0 : 1);
    if (status == 2) score = vit = __builtin_nan("");
    if (status == 1) score = vit = -INFINITY;
    ss_ctc_align_result r;
    r.score = score; r.viterbi = vit; r.status = status; r.n_tokens = L;
    results[blockIdx.x] = r;
    s_status = status;
    if (status == 0) {
      int s = end;
      for (int t = T - 1; t >= 1; --t) {
        st[t] = s;
        s -= (bp[(long long)t * stride + (s >> 2)] >> ((s & 3) * 2)) & 3;
      }
      st[0] = s;
    }
  }
  __syncthreads();
  if (s_status != 0) {
    for (int t = tid; t < T; t += 256) {
      if (path) path[sg.row0 + t] = -1;
      if (frame_lprob) frame_lprob[sg.row0 + t] = __builtin_nanf("");
    }
    for (int j = tid; j < L; j += 256) { first[sg.lab0 + j] = -1; last[sg.lab0 + j] = -1; tok_lprob[sg.lab0 + j] = __builtin_nanf(""); }
    return;
  }
  for (int t = tid; t < T; t += 256) {
    const int s = st[t], c = ctc_align_col(s);
    if (path) path[sg.row0 + t] = (s & 1) ? y[s >> 1] : 0;
    if (frame_lprob) frame_lprob[sg.row0 + t] = lp[(long long)t * W + c];
    if ((s & 1) && (t == 0 || st[t - 1] != s)) {               // the first frame of label j's run: its thread sums the run in frame order
      const int j = s >> 1;
      float acc = lp[(long long)t * W + c];
      int e = t;
      while (e + 1 < T && st[e + 1] == s) { ++e; acc += lp[(long long)e * W + c]; }
      first[sg.lab0 + j] = t; last[sg.lab0 + j] = e; tok_lprob[sg.lab0 + j] = acc;
    }
  }
}

size_t ctc_align_table_bytes(const CtcAlignPlan& p) { return p.segs.size() * sizeof(CtcAlignSeg) + (size_t)p.labels * sizeof(int); }

int launch_ctc_align(const float* logits, int ld, int V, const CtcAlignPlan& p, const int32_t* h_targets, void* d_table, void* d_work,
                     ss_ctc_align_result* results, int* path, int* first, int* last, float* tok_lprob, float* frame_lprob,
                     hipStream_t stream) {
  const int B = (int)p.segs.size();
  if (!logits || ld < V || B <= 0 || !d_table || !d_work || !results || (p.labels > 0 && (!first || !last || !tok_lprob || !h_targets)))
    return SS_ERR_ARG;
  const size_t seg_bytes = (size_t)B * sizeof(CtcAlignSeg);
  std::vector<unsigned char> tab(ctc_align_table_bytes(p));
  memcpy(tab.data(), p.segs.data(), seg_bytes);
  if (p.labels) memcpy(tab.data() + seg_bytes, h_targets, (size_t)p.labels * sizeof(int));
  SS_HIP_CHECK(hipMemcpyAsync(d_table, tab.data(), tab.size(), hipMemcpyHostToDevice, stream));
  const CtcAlignSeg* d_segs = static_cast<const CtcAlignSeg*>(d_table);
  const int* d_labels = reinterpret_cast<const int*>(static_cast<const unsigned char*>(d_table) + seg_bytes);
  float* d_lp = static_cast<float*>(d_work);
  unsigned char* d_bp = static_cast<unsigned char*>(d_work) + (size_t)p.lp_floats * sizeof(float);
  hipLaunchKernelGGL(ctc_align_lp_kernel, dim3(p.rows), dim3(256), 0, stream, logits, ld, V, d_segs, B, d_labels, d_lp);
  SS_LAUNCH_CHECK();
  int max_T = 0;
  for (const CtcAlignSeg& s : p.segs) max_T = s.T > max_T ? s.T : max_T;
  const size_t lds = 2 * (size_t)p.max_S * sizeof(double) + ((size_t)p.max_L + max_T) * sizeof(int);   // <= 60 016 bytes at the limits
  hipLaunchKernelGGL(ctc_align_trellis_kernel, dim3(B), dim3(256), lds, stream, d_segs, d_labels, p.max_S, p.max_L, d_lp, d_bp, results,
                     path, first, last, tok_lprob, frame_lprob);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss

using namespace ss;

extern "C" int ss_ctc_align_host(const float* h_logits, int ld, int V, int pad, int B, const int32_t* h_T, const int32_t* h_targets,
                                 const int32_t* h_n_targets, ss_ctc_align_result* h_results, int32_t* h_path, int32_t* h_first,
                                 int32_t* h_last, float* h_tok_lprob, float* h_frame_lprob) {
  if (!h_logits || ld < V || !h_results) return SS_ERR_ARG;
  CtcAlignPlan p;
  RET(ctc_align_plan(V, pad, B, h_T, h_targets, h_n_targets, p));
  if (p.labels > 0 && (!h_first || !h_last || !h_tok_lprob)) return SS_ERR_ARG;
  for (int b = 0; b < B; ++b) {
    const CtcAlignSeg& sg = p.segs[b];
    const int T = sg.T, L = sg.L, S = 2 * L + 1, W = L + 1;
    const int32_t* y = h_targets + sg.lab0;
    std::vector<float> lp((size_t)T * W);
    bool nan = false;
    for (int t = 0; t < T; ++t) {
      const float* r = h_logits + (size_t)(sg.row0 + t) * ld;
      float mx, lt;
      const bool bad = ctc_row_den_host(r, V, &mx, &lt);
      for (int j = 0; j <= L; ++j) lp[(size_t)t * W + j] = bad ? __builtin_nanf("") : (r[j ? y[j - 1] : 0] - mx) - lt;
      nan |= lp[(size_t)t * W] != lp[(size_t)t * W];           // as the kernel learns of it: the blank column of the row
    }
    std::vector<double> a(S), v(S), na(S), nv(S);
    std::vector<unsigned char> bp((size_t)T * S, 0);
    for (int s = 0; s < S; ++s) a[s] = v[s] = s < 2 ? (double)lp[ctc_align_col(s)] : -INFINITY;
    for (int t = 1; t < T; ++t) {
      for (int s = 0; s < S; ++s) {
        const bool sk = ctc_align_can_skip(y, s);
        const double x = (double)lp[(size_t)t * W + ctc_align_col(s)];
        int back = 0;
        na[s] = ctc_align_logadd3(a[s], s >= 1 ? a[s - 1] : -INFINITY, sk ? a[s - 2] : -INFINITY) + x;
        nv[s] = ctc_align_best3(v[s], s >= 1 ? v[s - 1] : -INFINITY, sk ? v[s - 2] : -INFINITY, &back) + x;
        bp[(size_t)t * S + s] = (unsigned char)back;
      }
      a.swap(na); v.swap(nv);
    }
    double score = ctc_align_logadd3(a[S - 1], S >= 2 ? a[S - 2] : -INFINITY, -INFINITY);
    const int end = ctc_align_end_state(v[S - 1], S >= 2 ? v[S - 2] : -INFINITY, S);
    double vit = v[end];
    const int status = nan ? 2 : (vit > -INFINITY ? 0 : 1);
    if (status == 2) score = vit = __builtin_nan("");
    if (status == 1) score = vit = -INFINITY;
    h_results[b].score = score; h_results[b].viterbi = vit; h_results[b].status = status; h_results[b].n_tokens = L;
    if (status != 0) {
      for (int t = 0; t < T; ++t) {
        if (h_path) h_path[sg.row0 + t] = -1;
        if (h_frame_lprob) h_frame_lprob[sg.row0 + t] = __builtin_nanf("");
      }
      for (int j = 0; j < L; ++j) { h_first[sg.lab0 + j] = h_last[sg.lab0 + j] = -1; h_tok_lprob[sg.lab0 + j] = __builtin_nanf(""); }
      continue;
    }
    std::vector<int> st(T);
    int s = end;
    for (int t = T - 1; t >= 1; --t) { st[t] = s; s -= bp[(size_t)t * S + s]; }
    st[0] = s;
    for (int t = 0; t < T; ++t) {
      const int c = ctc_align_col(st[t]);
      if (h_path) h_path[sg.row0 + t] = (st[t] & 1) ? y[st[t] >> 1] : 0;
      if (h_frame_lprob) h_frame_lprob[sg.row0 + t] = lp[(size_t)t * W + c];
      if ((st[t] & 1) && (t == 0 || st[t - 1] != st[t])) {
        const int j = st[t] >> 1;
        float acc = lp[(size_t)t * W + c];
        int e = t;
        while (e + 1 < T && st[e + 1] == st[t]) { ++e; acc += lp[(size_t)e * W + c]; }
        h_first[sg.lab0 + j] = t; h_last[sg.lab0 + j] = e; h_tok_lprob[sg.lab0 + j] = acc;
      }
    }
  }
  return SS_OK;
}
