// Scored CTC greedy search of the two text heads: the per-frame arg-max WITH its log-probability, and the collapse WITH each kept
// token's last frame and summed log-probability -- what the reference's CTCDecoder.generate returns as `positional_scores`
// (`lprobs.max(dim=2)` after pad / unk are set to -inf, agent/ctc_decoder.py:52-62) and what word time spans and confidences are
// made of.  Twins of masked_argmax_kernel / ctc_collapse_kernel (elementwise.hip), which stay as they are: with scores off the
// library launches exactly what it launched before.
#include "ctc_row.hpp"
#include "elementwise.hpp"

namespace ss {

// One logits row per workgroup.  ids[row]: masked_argmax_kernel's rule bit for bit (masked columns skipped, NaN counts as -inf
// but stays a candidate, the lowest index wins a tie).  lprob[row] = (best - max) - log(sum exp(x - max)) over the FULL row:
// log-softmax first, masks after (agent/ctc_decoder.py:52-60), the quantity of row_max_logprob_kernel; any NaN in the row gives NaN
// as torch.log_softmax does.  PER > 0: N <= 256 * PER, the row is read from global memory once and each thread keeps its PER values
// in registers across the max pass and the sum pass.  PER == 0: any N, the sum pass reads the row again.
// The denominator and its fixed order: ctc_row.hpp (the max pass here shares its shuffle rounds with the arg-max and stays in this
// kernel; the sum pass is the header's), so a row's result is a function of that row's bits alone, never of M or of its position.
template <int PER>
__global__ __launch_bounds__(256) void masked_argmax_lprob_kernel(const float* __restrict__ logits, int ld, int N, int mask0,
                                                                  int mask1, int mask2, int* __restrict__ ids,
                                                                  float* __restrict__ lprob) {
  __shared__ float sb[4], sm[4], ssum[4];
  __shared__ int si[4], sn[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x;
  const float* r = logits + (size_t)row * ld;
  float v[PER > 0 ? PER : 1];
  float best = -INFINITY, mx = -INFINITY;
  int bi = 0x7fffffff, nan = 0;
  auto visit = [&](int n, float x) {
    nan |= (x != x);
    mx = fmaxf(mx, x);
    if (n == mask0 || n == mask1 || n == mask2) return;
    if (x != x) x = -INFINITY;                                 // NaN -> -inf, still a candidate (as masked_argmax_kernel)
    if (bi == 0x7fffffff || x > best) { best = x; bi = n; }    // n ascends per thread: first max wins
  };
  if constexpr (PER > 0) {
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int n = t + 256 * i;
      v[i] = n < N ? r[n] : -INFINITY;                         // past the row: exp(-inf - max) = 0 in the sum pass
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int n = t + 256 * i;
      if (n < N) visit(n, v[i]);
    }
  } else {
    for (int n = t; n < N; n += 256) visit(n, r[n]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    nan |= __shfl_xor(nan, o, 64);
  }
  if (lane == 0) { sb[wave] = best; si[wave] = bi; sm[wave] = mx; sn[wave] = nan; }
  __syncthreads();
  mx = ctc_row_max4(sm);
  ctc_row_expsum<PER>(r, N, v, mx, ssum);
  if (t == 0) {
    for (int w = 1; w < 4; ++w) {
      const float ob = sb[w]; const int oi = si[w];
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
    }
    ids[row] = bi;
    lprob[row] = ctc_row_nan(sn) ? __builtin_nanf("") : (best - mx) - ctc_row_logsum(ssum);
  }
}

int launch_masked_argmax_lprob(const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2, int* ids, float* lprob,
                               hipStream_t stream) {
  if (M < 0 || N <= 0 || ld < N || !logits || !ids || !lprob) return SS_ERR_ARG;
  if (M == 0) return SS_OK;
#define SS_AML(PER)                                                                                                               \
  hipLaunchKernelGGL(masked_argmax_lprob_kernel<PER>, dim3(M), dim3(256), 0, stream, logits, ld, N, mask0, mask1, mask2, ids, lprob)
  if (N <= 2048) SS_AML(8);
  else if (N <= 4096) SS_AML(16);
  else if (N <= 6144) SS_AML(24);
  else if (N <= 8192) SS_AML(32);
  else SS_AML(0);
#undef SS_AML
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ctc_collapse_kernel (elementwise.hip) with two more outputs per kept token j: last[j], the last frame of the run of equal raw ids
// that starts at index[j], and tok_lprob[j], the float32 sum of lprob[index[j] .. last[j]] added in ascending frame order by the
// one thread that keeps the token (deterministic).  The walk reads raw[] of the whole utterance, so a run that crosses the
// 1024-frame chunks of the compaction comes out like any other.  tokens / index / count: identical to ctc_collapse_kernel.
__global__ __launch_bounds__(1024) void ctc_collapse_spans_kernel(const int* __restrict__ raw, const float* __restrict__ lprob, int T,
                                                                  int blank, int pad, int* tokens, int* index, int* last,
                                                                  float* tok_lprob, int* count, const int* __restrict__ segs) {
  __shared__ int wave_tot[16];
  __shared__ int base_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (segs) {   // one workgroup per utterance: rows [start, start+len) of the packed arrays
    const int st = segs[2 * blockIdx.x];
    T = segs[2 * blockIdx.x + 1];
    raw += st; lprob += st; tokens += st; index += st; last += st; tok_lprob += st; count += blockIdx.x;
  }
  if (t == 0) base_s = 0;
  __syncthreads();
  for (int c0 = 0; c0 < T; c0 += 1024) {
    const int i = c0 + t;
    int v = 0, e = i;
    float acc = 0.f;
    bool keep = false;
    if (i < T) {
      v = raw[i];
      keep = (i == 0 || v != raw[i - 1]) && v != blank && v != pad;
    }
    if (keep) {
      acc = lprob[i];
      while (e + 1 < T && raw[e + 1] == v) { ++e; acc += lprob[e]; }
    }
    const unsigned long long bal = __ballot(keep);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[wave] = __popcll(bal);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    if (keep) { tokens[off + pre] = v; index[off + pre] = i; last[off + pre] = e; tok_lprob[off + pre] = acc; }
    __syncthreads();
    if (t == 0) { int s = 0; for (int w = 0; w < 16; ++w) s += wave_tot[w]; base_s += s; }
    __syncthreads();
  }
  if (t == 0) *count = base_s;
}

int launch_ctc_collapse_spans(const int* raw, const float* lprob, int T, int blank, int pad, int* tokens, int* index, int* last,
                              float* tok_lprob, int* count, hipStream_t stream, const int* segs, int nseg) {
  if (!raw || !lprob || !tokens || !index || !last || !tok_lprob || !count || nseg < 0 || (nseg > 0 && !segs) || T < 0) return SS_ERR_ARG;
  hipLaunchKernelGGL(ctc_collapse_spans_kernel, dim3(nseg > 0 ? nseg : 1), dim3(1024), 0, stream, raw, lprob, T, blank, pad, tokens,
                     index, last, tok_lprob, count, nseg > 0 ? segs : nullptr);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss
