// The back-off n-gram language model of the CTC prefix beam search's shallow fusion (ngram_lm.hpp: the table, the scoring rule and
// the host builder): the object of the C ABI -- built on the host, uploaded once, read-only afterwards, so one object serves every
// context and stream -- the plain-C++ scorer (ss_ngram_score_host) and the score kernel behind ss_op_ngram_score, the op-level
// handle on the device lookup that the fused search (ctc_beam.hip) runs inside its frame loop.
#include "ngram_lm.hpp"

#include <cstring>
#include <mutex>
#include <new>

#include "../../include/streamspeech_hip.h"
#include "elementwise.hpp"

namespace ss {

// One wave per sequence, four per block; the walk is a chain of dependent lookups, so lane 0 of the wave makes it.
// seq[b] = {first token, first output, tokens}: the outputs of sequence b are n + with_eos values from its first output on.
__global__ __launch_bounds__(256) void ngram_score_kernel(NgramView lm, int B, const int32_t* __restrict__ tokens,
                                                          const long long* __restrict__ seq, int with_eos, double* __restrict__ lp,
                                                          int32_t* __restrict__ state) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B || (threadIdx.x & 63) != 0) return;
  const long long t0 = seq[3 * (size_t)b], o0 = seq[3 * (size_t)b + 1];
  const int n = (int)seq[3 * (size_t)b + 2];
  ngram_score_seq(lm, tokens + t0, n, with_eos, lp + o0, state ? state + o0 : nullptr);
}

// The one upload, made by the first device call that needs the table (ss_ngram_lm_create itself touches no device, so the host
// twins serve a machine without one): keys | entries | vals in one buffer, 8-, 4- and 4-byte items in that order.
int ngram_device_view(const ss_ngram_lm* clm, NgramView* out) {
  ss_ngram_lm* lm = const_cast<ss_ngram_lm*>(clm);
  std::lock_guard<std::mutex> lk(lm->mu);
  if (!lm->d_mem) {
    const NgramTable& t = lm->host;
    const size_t nk = t.keys.size() * 8, ne = t.ent.size() * sizeof(NgramEntry), nv = t.vals.size() * 4;
    std::vector<unsigned char> img(nk + ne + nv);
    memcpy(img.data(), t.keys.data(), nk);
    memcpy(img.data() + nk, t.ent.data(), ne);
    memcpy(img.data() + nk + ne, t.vals.data(), nv);
    void* d_mem = nullptr;
    SS_HIP_CHECK(hipMalloc(&d_mem, img.size()));
    const hipError_t e = hipMemcpy(d_mem, img.data(), img.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_mem); SS_HIP_CHECK(e); }
    unsigned char* d = static_cast<unsigned char*>(d_mem);
    lm->dev = NgramView{reinterpret_cast<const unsigned long long*>(d), reinterpret_cast<const int*>(d + nk + ne),
                        reinterpret_cast<const NgramEntry*>(d + nk), t.mask, t.start, t.unk_entry, t.eos, (double)t.oov_logp};
    lm->d_mem = d_mem;
  }
  *out = lm->dev;
  return SS_OK;
}

size_t ngram_score_table_bytes(int B) { return (size_t)B * 3 * sizeof(long long); }

int launch_ngram_score(const ss_ngram_lm* lm, int B, const int32_t* d_tokens, const int32_t* h_n, int with_eos, double* d_lp,
                       int32_t* d_state, void* d_table, hipStream_t stream) {
  if (!lm || B <= 0 || !h_n || !d_lp || !d_table || (with_eos && lm->host.eos < 0)) return SS_ERR_ARG;
  std::vector<long long> seq(3 * (size_t)B);
  long long t0 = 0, o0 = 0;
  for (int b = 0; b < B; ++b) {
    if (h_n[b] < 0) return SS_ERR_ARG;
    seq[3 * (size_t)b] = t0; seq[3 * (size_t)b + 1] = o0; seq[3 * (size_t)b + 2] = h_n[b];
    t0 += h_n[b]; o0 += h_n[b] + (with_eos ? 1 : 0);
  }
  if (t0 > 0 && !d_tokens) return SS_ERR_ARG;
  if (o0 == 0) return SS_OK;
  NgramView dev;
  RET(ngram_device_view(lm, &dev));
  SS_HIP_CHECK(hipMemcpyAsync(d_table, seq.data(), ngram_score_table_bytes(B), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(ngram_score_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, dev, B, d_tokens,
                     static_cast<const long long*>(d_table), with_eos, d_lp, d_state);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss

using namespace ss;

extern "C" int ss_ngram_lm_create(int order, const int64_t* h_counts, const int32_t* h_tokens, const float* h_logp,
                                  const float* h_backoff, int V, int bos, int eos, int unk, float oov_logp, ss_ngram_lm** out) {
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  ss_ngram_lm* lm = new (std::nothrow) ss_ngram_lm();
  if (!lm) return SS_ERR_ARG;
  const int rc = ngram_build(order, h_counts, h_tokens, h_logp, h_backoff, V, bos, eos, unk, oov_logp, lm->host);
  if (rc != SS_OK) { delete lm; return rc; }
  const NgramTable& t = lm->host;
  lm->d_bytes = t.keys.size() * 12 + t.ent.size() * sizeof(NgramEntry);
  *out = lm;
  return SS_OK;
}

extern "C" void ss_ngram_lm_destroy(ss_ngram_lm* lm) {
  if (!lm) return;
  if (lm->d_mem) (void)hipFree(lm->d_mem);
  delete lm;
}

extern "C" int ss_ngram_lm_info(const ss_ngram_lm* lm, int32_t* order, int64_t* entries, int64_t* slots, int64_t* device_bytes) {
  if (!lm) return SS_ERR_ARG;
  if (order) *order = lm->host.order;
  if (entries) *entries = lm->host.entries;
  if (slots) *slots = (int64_t)lm->host.mask + 1;
  if (device_bytes) *device_bytes = (int64_t)lm->d_bytes;
  return SS_OK;
}

extern "C" int ss_ngram_score_host(const ss_ngram_lm* lm, int B, const int32_t* h_tokens, const int32_t* h_n, int with_eos,
                                   double* h_lp, int32_t* h_state) {
  if (!lm || B <= 0 || !h_n || !h_lp || (with_eos && lm->host.eos < 0)) return SS_ERR_ARG;
  long long total = 0;
  for (int b = 0; b < B; ++b) {
    if (h_n[b] < 0) return SS_ERR_ARG;
    total += h_n[b];
  }
  if (total > 0 && !h_tokens) return SS_ERR_ARG;
  const NgramView v = lm->host.view();
  long long t0 = 0, o0 = 0;
  for (int b = 0; b < B; ++b) {
    ngram_score_seq(v, h_tokens + t0, h_n[b], with_eos, h_lp + o0, h_state ? h_state + o0 : nullptr);
    t0 += h_n[b]; o0 += h_n[b] + (with_eos ? 1 : 0);
  }
  return SS_OK;
}
