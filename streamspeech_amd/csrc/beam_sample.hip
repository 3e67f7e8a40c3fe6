// ---- sampling (ss_batch_mt_sample; the rule stands in include/streamspeech_hip.h at ss_mt_sample_opts) ----
// The same frame as the beam search (beam.hip): B utterances x k slots in lockstep, the same decoder launches, the same state and
// finalised table.  Slot j of an utterance is chain j, an independent ancestral sample, so the ancestry is the identity after the
// prefix and is written once; per step
//   sample_step_kernel     one workgroup per chain row: the row phase of the top-2k kernel (beam_rows.hpp: temperature, log-softmax,
//                          masks, ban; no cumulative score), the kept set (top-k: a radix select of the K-th value over integer
//                          histograms; top-p: one bitonic sort of the row's ids in LDS, ordered by (value descending, id ascending),
//                          and a scan of the masses in that order), one fixed-order scan of the kept masses in id order, the draw
//   sample_advance_kernel  one workgroup per utterance: cumulative scores, finalisation of the chains that drew </s>, ignore flags,
//                          next tokens, done flag
// No float atomics anywhere: every sum is a per-thread sequential chain over a contiguous chunk, then one shuffle scan per wave and
// the four wave totals in order, so a row's bits depend on the row alone.
#include <cmath>

#include "beam_rows.hpp"

using namespace ss;

namespace {

// Philox4x32-10 (Salmon et al., SC'11): counter c[4], key (k0, k1) -> c
__host__ __device__ inline void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (unsigned)p1; c[2] = n2; c[3] = (unsigned)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// counter (step, j, key_lo, key_hi), key (seed_lo, seed_hi); u = (word 0 >> 8) * 2^-24
__device__ __forceinline__ float sample_uniform(unsigned long long seed, unsigned long long key, int step, int j, unsigned w[4]) {
  w[0] = (unsigned)step; w[1] = (unsigned)j; w[2] = (unsigned)key; w[3] = (unsigned)(key >> 32);
  philox4x32_10(w, (unsigned)seed, (unsigned)(seed >> 32));
  return (float)(w[0] >> 8) * 0x1p-24f;
}

__global__ __launch_bounds__(256) void sample_uniform_kernel(int n, const unsigned long long* __restrict__ seed,
                                                             const unsigned long long* __restrict__ key, const int* __restrict__ step,
                                                             const int* __restrict__ j, float* __restrict__ u,
                                                             unsigned* __restrict__ words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  unsigned w[4];
  u[i] = sample_uniform(seed[i], key[i], step[i], j[i], w);
  for (int q = 0; q < 4; ++q) words[4 * i + q] = w[q];
}

constexpr size_t kSampleLdsMax = 144 * 1024;   // of the CU's 160 KiB; a row of 16384 with its ids is 128 KiB

// exclusive prefix of x over the 256 threads in thread order, and the total; sw [4]
__device__ __forceinline__ float block_excl_scan(float x, float* sw, float& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  float ex = __shfl_up(inc, 1, 64);
  if (lane == 0) ex = 0.f;
  __syncthreads();                                 // earlier readers of sw are done
  if (lane == 63) sw[wave] = inc;
  __syncthreads();
  float base = 0.f;
  for (int w = 0; w < wave; ++w) base += sw[w];
  total = ((sw[0] + sw[1]) + sw[2]) + sw[3];
  return base + ex;
}

// the same over ints
__device__ __forceinline__ int block_excl_scan_int(int x, int* si, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  __syncthreads();
  if (lane == 63) si[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += si[w];
  total = si[0] + si[1] + si[2] + si[3];
  return base + inc - x;
}

// a float as an unsigned that orders as the float does (-0 counts as +0; no NaN comes here)
__device__ __forceinline__ unsigned order_key(float v) {
  const unsigned b = v == 0.f ? 0u : __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// OP: 0 sum, 1 min, 2 max over the 256 threads; si [4]
template <int OP>
__device__ __forceinline__ int block_reduce_int(int x, int* si) {
  auto f = [](int a, int b) { return OP == 0 ? a + b : OP == 1 ? min(a, b) : max(a, b); };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = f(x, __shfl_xor(x, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) si[threadIdx.x >> 6] = x;
  __syncthreads();
  return f(f(si[0], si[1]), f(si[2], si[3]));
}

__global__ __launch_bounds__(256) void sample_step_kernel(const float* __restrict__ logits, int V, int k, int t_step, int min_len,
                                                          const int* __restrict__ max_len, const int* __restrict__ npre,
                                                          const int* __restrict__ done, int pad, int unk, int eos, float unk_pen,
                                                          TopkOpts o, SampleArgs sp) {
  extern __shared__ float vals[];                  // [V] the row's candidate values v[n]
  __shared__ float sa[4];
  __shared__ int si[4];
  const int t = threadIdx.x;
  const int row = blockIdx.x, b = row / k, j = sp.row_j ? sp.row_j[row] : row - b * k;
  if ((done && done[b]) || (sp.ignore && sp.ignore[row])) return;
  const int step = t_step + npre[b];
  // first free step: every chain draws from the row of slot 0 (lprobs[:, ::beam_size] of Sampling.step)
  const float* r = logits + (size_t)(t_step == 0 ? b * k : row) * V;
  auto logit = [&](int n) -> float { return r[n] / o.temp; };
  int* ids = reinterpret_cast<int*>(vals + V);     // [npad], behind the ban's arrays when there is a ban
  RowMask m{pad, unk, eos, unk_pen};
  if (o.ngram >= 2) {
    m.banned = row_ban_map(o, vals, V, row, b, step, npre[b]);
    ids += o.Lc + (V + 31) / 32;
  }
  const float mx = row_max_sums(logit, V, sa);
  const float lse = row_lse(sa);
  m.at_max = step >= max_len[b]; m.below_min = step < min_len;
  int nfin = 0;
  for (int n = t; n < V; n += 256) {
    const float v = row_masked_lprob(logit, n, mx, lse, m);
    vals[n] = v;
    nfin += v > -INFINITY ? 1 : 0;
  }
  nfin = block_reduce_int<0>(nfin, si);            // its barriers also publish vals
  // ---- the kept set: every token that stands at or before (vt, it) in the order (value descending, id ascending) ----
  bool thr = false;                                // a threshold (vt, it) applies; without one every finite token is kept
  float vt = -INFINITY;
  int it = -1, nk = nfin;
  if (sp.topk > 0 && sp.topk < nfin) {
    // top-k: a radix select of the K-th largest value, eight bits a pass, over integer histograms in LDS (exact); then the ties at
    // that value are taken in ascending id order
    __shared__ int hist[256];
    __shared__ unsigned sel[2];
    unsigned prefix = 0;
    int rem = sp.topk;                             // the ranks still to pass inside the current prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
      hist[t] = 0;
      __syncthreads();
      const unsigned himask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
      for (int n = t; n < V; n += 256) {
        const unsigned key = order_key(vals[n]);
        if ((key & himask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      const int c = hist[255 - t];                 // thread t owns bin 255 - t: the scan runs from the largest values down
      int tot;
      const int ex = block_excl_scan_int(c, si, tot);
      if (ex < rem && rem <= ex + c) { sel[0] = 255u - t; sel[1] = (unsigned)ex; }
      __syncthreads();
      prefix |= sel[0] << shift;
      rem -= (int)sel[1];
      __syncthreads();                             // sel and hist are written again in the next pass
    }
    vt = __uint_as_float((prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix);
    const int C = (V + 255) / 256, n0 = min(t * C, V), n1 = min(n0 + C, V);
    int c = 0;
    for (int n = n0; n < n1; ++n) c += order_key(vals[n]) == prefix ? 1 : 0;
    int tot;
    const int ex = block_excl_scan_int(c, si, tot);
    if (ex < rem && rem <= ex + c) {
      int q = ex;
      for (int n = n0; n < n1; ++n)
        if (order_key(vals[n]) == prefix && ++q == rem) { sel[0] = (unsigned)n; break; }
    }
    __syncthreads();
    it = (int)sel[0];
    nk = sp.topk;
    thr = true;
  } else if (sp.topp > 0.f) {
    const int N = sp.npad;
    for (int i = t; i < N; i += 256) ids[i] = i < V ? i : -1;
    __syncthreads();
    auto before = [&](int a, int c) -> bool {      // a stands before c; ids < 0 are the padding and stand last
      if (c < 0) return a >= 0;
      if (a < 0) return false;
      const float va = vals[a], vc = vals[c];
      return va > vc || (va == vc && a < c);
    };
    for (int size = 2; size <= N; size <<= 1)
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = t; i < (N >> 1); i += 256) {
          const int lo = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), hi = lo + stride;
          const int a = ids[lo], c = ids[hi];
          if ((lo & size) == 0 ? before(c, a) : before(a, c)) { ids[lo] = c; ids[hi] = a; }
        }
        __syncthreads();
      }
    // _sample_topp: position i of the order is kept while the mass before it is < P; one fixed-order scan over the positions
    const int C = (N + 255) / 256, i0 = t * C, i1 = min(i0 + C, nfin);
    float loc = 0.f;
    for (int i = i0; i < i1; ++i) loc += expf(vals[ids[i]]);
    float tot;
    const float ex = block_excl_scan(loc, sa, tot);
    int first = nfin;
    float run = 0.f;
    for (int i = i0; i < i1; ++i) {
      if (!(ex + run < sp.topp)) { first = i; break; }
      run += expf(vals[ids[i]]);
    }
    nk = block_reduce_int<1>(first, si);
    if (nk > 0) { it = ids[nk - 1]; vt = vals[it]; thr = true; }
  }
  auto kept = [&](int n, float v) -> bool {
    if (!(v > -INFINITY)) return false;
    return !thr || v > vt || (v == vt && n <= it);
  };
  // ---- the draw: the kept masses in ascending id order, one scan; the first id whose cumulative mass exceeds u * Z ----
  unsigned w[4];
  const float u = sample_uniform(sp.seed, sp.keys[b], step, j, w);
  const int C = (V + 255) / 256, n0 = min(t * C, V), n1 = min(n0 + C, V);
  float loc = 0.f;
  int cnt = 0, last = -1;
  for (int n = n0; n < n1; ++n) {
    const float v = vals[n];
    if (kept(n, v)) { loc += expf(v); ++cnt; last = n; }
  }
  float Z;
  const float ex = block_excl_scan(loc, sa, Z);
  const float target = u * Z;
  int pick = 0x7fffffff;
  float run = 0.f;
  for (int n = n0; n < n1; ++n) {
    const float v = vals[n];
    if (!kept(n, v)) continue;
    run += expf(v);
    if (ex + run > target) { pick = n; break; }
  }
  pick = block_reduce_int<1>(pick, si);
  last = block_reduce_int<2>(last, si);
  cnt = block_reduce_int<0>(cnt, si);
  if (pick == 0x7fffffff) pick = last >= 0 ? last : eos;   // u * Z rounded up to the last sum: the last kept id; nothing kept: </s>
  if (t == 0) {
    sp.tok_out[(size_t)row * sp.out_ld] = pick;
    sp.score_out[(size_t)row * sp.out_ld] = vals[pick];
    if (sp.u_out) sp.u_out[row] = u;
    if (sp.kept_out) sp.kept_out[row] = cnt;
  }
}

// One workgroup per utterance, after sample_step_kernel: chain j = slot j takes its drawn token.  Its cumulative score is the
// in-order float32 sum of the positional scores (behind a prefix, on top of the prefix' sum, which slot 0 holds at lock-step index
// 0).  A chain that drew </s> is finalised into entry j of the utterance's table -- score as beam_merge_body forms it -- and is
// ignored from then on; the utterance is done when all k chains are.  Tokens and positional scores go to entry j step by step; the
// ancestry never changes (both halves of st.anc hold it from the start), so a finalised entry copies its row.
__global__ __launch_bounds__(64) void sample_advance_kernel(BeamState st, int k, int R, int Lc, int t_step, int c0, int eos,
                                                            int normalize, float len_penalty) {
  const int t = threadIdx.x, b = blockIdx.x, r0 = b * k, r = r0 + t;
  int* tok_nxt = st.tok + (size_t)(t_step + 1) * R;
  float* cum_nxt = st.cum + (size_t)(t_step + 1) * R;
  if (st.done[b]) {                  // finished utterance: its rows keep decoding (lockstep)
    if (t < k) { tok_nxt[r] = eos; cum_nxt[r] = 0.f; }
    return;
  }
  const int step = t_step + st.npre[b], ci = c0 + t_step;
  bool fin = false, now = false;
  if (t < k) {
    fin = st.ignore[r] != 0;
    int tk = eos;
    float c = 0.f;
    if (!fin) {
      tk = st.cand_t[(size_t)r * kMaxCand];
      const float v = st.cand_s[(size_t)r * kMaxCand];
      const float prv = st.cum[(size_t)t_step * R + (t_step == 0 ? r0 : r)];
      c = step > 0 ? v + prv : v;
      const size_t o = (size_t)r * Lc;
      st.fin_tok[o + t_step] = tk;
      st.fin_pos[o + t_step] = v;
      if (tk == eos) {
        float s = c;
        if (normalize)
          s = len_penalty != 1.f ? c / (float)pow((double)(step + 1), (double)len_penalty) : c / (float)(step + 1);
        st.fin_score[r] = s;
        st.fin_len[r] = t_step + 1;
        st.ignore[r] = 1;
        fin = now = true;
        c = 0.f;
      }
    }
    tok_nxt[r] = tk;
    cum_nxt[r] = c;
  }
  const unsigned long long fm = __ballot(fin), nm = __ballot(now);
  const int cnt = __popcll(fm);
  if (t == 0) {
    st.fin_cnt[b] = cnt;
    st.done[b] = cnt == k || step >= st.max_len[b];
  }
  const int* anc_cur = st.anc + (size_t)(t_step & 1) * R * Lc;
  for (int q = 0; q < k; ++q)
    if ((nm >> q) & 1ull)
      for (int p = t; p <= ci; p += 64) st.fin_anc[(size_t)(r0 + q) * Lc + p] = anc_cur[(size_t)(r0 + q) * Lc + p];
}

}  // namespace

namespace ss {

// the row | with a ban the history and the bit map (as the top-2k kernel) | the ids the sort orders
int sample_step_lds(int V, const TopkOpts& o, const SampleArgs& sp, size_t& bytes) {
  bytes = topk_lds_bytes(V, o.ngram, o.Lc) + (size_t)sp.npad * sizeof(int);
  return bytes > kSampleLdsMax ? SS_ERR_ARG : SS_OK;
}

int launch_sample_step(hipStream_t s, int R, const RowStep& a, const TopkOpts& o, const SampleArgs& sp) {
  size_t lds;
  RET(sample_step_lds(a.V, o, sp, lds));
  SS_MAX_LDS_ONCE(sample_step_kernel, kSampleLdsMax);
  hipLaunchKernelGGL(sample_step_kernel, dim3(R), dim3(256), lds, s, a.logits, a.V, a.k, a.t_step, a.min_len, a.max_len, a.npre, a.done,
                     a.pad, a.unk, a.eos, a.unk_pen, o, sp);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_sample_advance(hipStream_t s, int B, const BeamState& st, int k, int Lc, int t_step, int c0, int eos, int normalize,
                          float len_penalty) {
  hipLaunchKernelGGL(sample_advance_kernel, dim3(B), dim3(64), 0, s, st, k, B * k, Lc, t_step, c0, eos, normalize ? 1 : 0, len_penalty);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss

// ---- op-level entry points (ss_mt_sample_opts; tests/test_sampling_ops_gpu.py) ----
extern "C" int ss_op_sample_step(void* stream, const float* logits, int R, int V, int t_step, int min_len, const int32_t* max_len,
                                 const int32_t* npre, int pad, int unk, int eos, float unk_pen, float temperature, int no_repeat_ngram,
                                 const int32_t* tok, const int32_t* anc, int Lc, int c0, const int32_t* ptok, const int32_t* row0,
                                 const int32_t* row_j, const int64_t* keys, const ss_mt_sample_opts* sample, int32_t* out_tok,
                                 float* out_score, float* out_u, int32_t* out_kept) {
  SampleArgs sa;
  RET(read_sample_opts(sample, keys, sa));
  if (sa.topk > V) return SS_ERR_ARG;
  const ss_mt_search_opts o{(int32_t)sizeof(ss_mt_search_opts), no_repeat_ngram, 1.f, temperature};
  SearchOpts so;
  RET(read_search_opts(&o, so));
  if (R <= 0 || V < 1 || (size_t)V * sizeof(float) > 65536 || t_step < 0 || eos < 0 || eos >= V) return SS_ERR_ARG;
  if (!logits || !max_len || !npre || !row_j || !out_tok || !out_score) return SS_ERR_ARG;
  if (so.ngram >= 2 && (!tok || !anc || c0 < 0 || c0 + t_step >= Lc)) return SS_ERR_ARG;
  const TopkOpts to = topk_opts(so, R, Lc, c0, tok, anc, ptok, row0);
  sa.npad = sample_npad(sa, V); sa.keys = reinterpret_cast<const unsigned long long*>(keys); sa.row_j = row_j;
  sa.out_ld = 1; sa.tok_out = out_tok; sa.score_out = out_score; sa.u_out = out_u; sa.kept_out = out_kept;
  RowStep a{logits, V, 1, t_step, min_len, max_len, npre, nullptr, nullptr, pad, unk, eos, unk_pen};
  return launch_sample_step((hipStream_t)stream, R, a, to, sa);
}

extern "C" int ss_op_sample_uniform(void* stream, int n, const uint64_t* seed, const int64_t* key, const int32_t* step,
                                    const int32_t* j, float* u, uint32_t* words) {
  if (n <= 0 || !seed || !key || !step || !j || !u || !words) return SS_ERR_ARG;
  hipLaunchKernelGGL(sample_uniform_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n,
                     reinterpret_cast<const unsigned long long*>(seed), reinterpret_cast<const unsigned long long*>(key), step, j, u,
                     words);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
