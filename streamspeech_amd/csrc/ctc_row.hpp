// The log-softmax denominator of one logits row, (max, log-sum), as the CTC side computes it: the greedy search's scores
// (masked_argmax_lprob_kernel, ctc_scores.hip), the aligner's lp (ctc_align_lp_kernel, ctc_align.hip) and the prefix beam search's
// den (ctc_beam_cand_kernel, ctc_beam.hip) are on one scale because all three, and the host twins, take it from here.
//
// THE ORDER, one workgroup of 256 threads per row, thread t on columns t, t + 256, ...:
//   1. max: each thread's f32 fmaxf over its columns in ascending stride, the xor-shuffle tree over the wave (offsets 32 .. 1), the
//      four wave maxima as fmaxf(fmaxf(w0, w1), fmaxf(w2, w3)); a NaN anywhere in the row raises the row's flag (fmaxf skips it)
//   2. sum: each thread's f32 sum of expf(x - max) in ascending stride from 0.f, the same xor tree with +, the four wave partials
//      as ((w0 + w1) + w2) + w3
//   3. one logf of that sum (ctc_row_logsum, by the threads that use the value)
// A flagged row gives NaN wherever the denominator is used (as torch.log_softmax); what is written then is the caller's.
// PER > 0: N <= 256 * PER, the row is read once and each thread keeps its PER values in registers for both passes (a column past
// the row is -inf: no maximum, and its exp is not added); PER == 0: any N, each pass reads the row again.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

namespace ss {

// The block's values from the [4] wave partials in LDS, after the barrier that follows their stores.
__device__ __forceinline__ float ctc_row_max4(const float* sm) { return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3])); }
__device__ __forceinline__ bool ctc_row_nan(const int* sn) { return sn[0] | sn[1] | sn[2] | sn[3]; }
__device__ __forceinline__ float ctc_row_logsum(const float* ssum) { return logf(((ssum[0] + ssum[1]) + ssum[2]) + ssum[3]); }

// Pass 1 for the kernels whose max pass does nothing else.  sm / sn: [4] wave partials in LDS; one barrier; then ctc_row_nan(sn).
template <int PER>
__device__ __forceinline__ float ctc_row_max(const float* r, int N, float (&v)[PER > 0 ? PER : 1], float* sm, int* sn) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float mx = -INFINITY;
  int nan = 0;
  if constexpr (PER > 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int n = t + 256 * i;
      v[i] = n < N ? r[n] : -INFINITY;
      nan |= (v[i] != v[i]);
      mx = fmaxf(mx, v[i]);
    }
  } else {
    for (int n = t; n < N; n += 256) { const float x = r[n]; nan |= (x != x); mx = fmaxf(mx, x); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); nan |= __shfl_xor(nan, o, 64); }
  if (lane == 0) { sm[wave] = mx; sn[wave] = nan; }
  __syncthreads();
  return ctc_row_max4(sm);
}

// Pass 2.  v: pass 1's registers (PER > 0).  ssum: [4] wave partials in LDS; one barrier; then ctc_row_logsum(ssum).
template <int PER>
__device__ __forceinline__ void ctc_row_expsum(const float* r, int N, const float (&v)[PER > 0 ? PER : 1], float mx,
                                               float* ssum) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float sum = 0.f;
  if constexpr (PER > 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const float e = expf(v[i] - mx);                          // the accurate forms, as row_max_logprob_kernel
      if (t + 256 * i < N) sum += e;
    }
  } else {
    for (int n = t; n < N; n += 256) sum += expf(r[n] - mx);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane == 0) ssum[wave] = sum;
  __syncthreads();
}

// The same on the host in the device's order: 256 strided partial sums, the xor tree inside each group of 64, the four group sums
// in index order.  Returns the row's NaN flag; *mx / *logsum are the values as computed.
inline bool ctc_row_den_host(const float* r, int N, float* mx_out, float* logsum_out) {
  float mx = -INFINITY;
  bool nan = false;
  for (int n = 0; n < N; ++n) { nan |= r[n] != r[n]; mx = fmaxf(mx, r[n]); }
  float part[256], tmp[256];
  for (int t = 0; t < 256; ++t) {
    float s = 0.f;
    for (int n = t; n < N; n += 256) s += expf(r[n] - mx);
    part[t] = s;
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int t = 0; t < 256; ++t) tmp[t] = part[t] + part[t ^ o];
    memcpy(part, tmp, sizeof(part));
  }
  *mx_out = mx;
  *logsum_out = logf(((part[0] + part[64]) + part[128]) + part[192]);
  return nan;
}

}  // namespace ss
