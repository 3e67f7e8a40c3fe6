// The hotword set of the CTC prefix beam search (ctc_bias.hpp: the automaton, the scoring rule and the host builder): the object of
// the C ABI -- built on the host, uploaded once, read-only afterwards, so one object serves every context and stream -- the
// plain-C++ scorer (ss_ctc_bias_score_host) and the score kernel behind ss_op_ctc_bias_score, the op-level handle on the device
// step that the biased search (ctc_beam.hip) runs inside its frame loop.
#include "ctc_bias.hpp"

#include <cstring>
#include <mutex>
#include <new>

#include "../../include/streamspeech_hip.h"
#include "elementwise.hpp"

namespace ss {

// One wave per sequence, four per block; the walk is a chain of dependent steps, so lane 0 of the wave makes it.
// seq[b] = {first token (and first delta / state), tokens}.
__global__ __launch_bounds__(256) void bias_score_kernel(BiasView bv, int B, const int32_t* __restrict__ tokens,
                                                         const long long* __restrict__ seq, int finish, double* __restrict__ delta,
                                                         int32_t* __restrict__ state, double* __restrict__ sum) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B || (threadIdx.x & 63) != 0) return;
  const long long t0 = seq[2 * (size_t)b];
  const int n = (int)seq[2 * (size_t)b + 1];
  bias_score_seq(bv, tokens + t0, n, finish, delta + t0, state ? state + t0 : nullptr, sum + b);
}

// The one upload, made by the first device call that needs the table (ss_ctc_bias_create itself touches no device, so the host
// twins serve a machine without one): keys | nodes | vals in one buffer, 8-, 8- and 4-byte items in that order.
int bias_device_view(const ss_ctc_bias* cbias, BiasView* out) {
  ss_ctc_bias* bias = const_cast<ss_ctc_bias*>(cbias);
  std::lock_guard<std::mutex> lk(bias->mu);
  if (!bias->d_mem) {
    const BiasTable& t = bias->host;
    const size_t nk = t.keys.size() * 8, ne = t.node.size() * sizeof(BiasNode), nv = t.vals.size() * 4;
    std::vector<unsigned char> img(nk + ne + nv);
    memcpy(img.data(), t.keys.data(), nk);
    memcpy(img.data() + nk, t.node.data(), ne);
    memcpy(img.data() + nk + ne, t.vals.data(), nv);
    void* d_mem = nullptr;
    SS_HIP_CHECK(hipMalloc(&d_mem, img.size()));
    const hipError_t e = hipMemcpy(d_mem, img.data(), img.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_mem); SS_HIP_CHECK(e); }
    unsigned char* d = static_cast<unsigned char*>(d_mem);
    bias->dev = BiasView{reinterpret_cast<const unsigned long long*>(d), reinterpret_cast<const int*>(d + nk + ne),
                         reinterpret_cast<const BiasNode*>(d + nk), t.mask, 0};
    bias->d_mem = d_mem;
  }
  *out = bias->dev;
  return SS_OK;
}

size_t bias_score_table_bytes(int B) { return (size_t)B * 2 * sizeof(long long); }

int launch_bias_score(const ss_ctc_bias* bias, int B, const int32_t* d_tokens, const int32_t* h_n, int finish, double* d_delta,
                      int32_t* d_state, double* d_sum, void* d_table, hipStream_t stream) {
  if (!bias || B <= 0 || !h_n || !d_sum || !d_table) return SS_ERR_ARG;
  std::vector<long long> seq(2 * (size_t)B);
  long long t0 = 0;
  for (int b = 0; b < B; ++b) {
    if (h_n[b] < 0) return SS_ERR_ARG;
    seq[2 * (size_t)b] = t0; seq[2 * (size_t)b + 1] = h_n[b];
    t0 += h_n[b];
  }
  if (t0 > 0 && (!d_tokens || !d_delta)) return SS_ERR_ARG;
  BiasView dev;
  RET(bias_device_view(bias, &dev));
  SS_HIP_CHECK(hipMemcpyAsync(d_table, seq.data(), bias_score_table_bytes(B), hipMemcpyHostToDevice, stream));
  hipLaunchKernelGGL(bias_score_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, dev, B, d_tokens,
                     static_cast<const long long*>(d_table), finish ? 1 : 0, d_delta, d_state, d_sum);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss

using namespace ss;

extern "C" int ss_ctc_bias_create(int n_phrases, const int32_t* h_tokens, const int32_t* h_off, const float* h_boost, int V, int pad,
                                  int unk, ss_ctc_bias** out) {
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  BiasTable t;                                                 // (the object is made only of a set that passed every check)
  RET(bias_build(n_phrases, h_tokens, h_off, h_boost, V, pad, unk, t));
  ss_ctc_bias* bias = new (std::nothrow) ss_ctc_bias();
  if (!bias) return SS_ERR_ARG;
  bias->host = std::move(t);
  bias->d_bytes = bias->host.table_bytes();
  *out = bias;
  return SS_OK;
}

extern "C" void ss_ctc_bias_destroy(ss_ctc_bias* bias) {
  if (!bias) return;
  if (bias->d_mem) (void)hipFree(bias->d_mem);
  delete bias;
}

extern "C" int ss_ctc_bias_info(const ss_ctc_bias* bias, int32_t* n_phrases, int64_t* nodes, int64_t* slots, int64_t* device_bytes) {
  if (!bias) return SS_ERR_ARG;
  if (n_phrases) *n_phrases = bias->host.phrases;
  if (nodes) *nodes = bias->host.nodes;
  if (slots) *slots = (int64_t)bias->host.mask + 1;
  if (device_bytes) *device_bytes = (int64_t)bias->d_bytes;
  return SS_OK;
}

extern "C" int ss_ctc_bias_score_host(const ss_ctc_bias* bias, int B, const int32_t* h_tokens, const int32_t* h_n, int finish,
                                      double* h_delta, int32_t* h_state, double* h_sum) {
  if (!bias || B <= 0 || !h_n || !h_sum) return SS_ERR_ARG;
  long long total = 0;
  for (int b = 0; b < B; ++b) {
    if (h_n[b] < 0) return SS_ERR_ARG;
    total += h_n[b];
  }
  if (total > 0 && (!h_tokens || !h_delta)) return SS_ERR_ARG;
  const BiasView v = bias->host.view();
  long long t0 = 0;
  for (int b = 0; b < B; ++b) {
    bias_score_seq(v, h_tokens + t0, h_n[b], finish, h_delta + t0, h_state ? h_state + t0 : nullptr, h_sum + b);
    t0 += h_n[b];
  }
  return SS_OK;
}
