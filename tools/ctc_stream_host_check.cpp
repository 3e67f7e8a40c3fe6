// Stand-alone check of the resumable CTC prefix beam search's host twin (ss_ctc_stream_advance_host, csrc/ctc_stream.hip over the
// twin of csrc/ctc_beam_host.hip) for a sanitizer build of the host code: (T, V, beam, cand) = (40, 64, 8, 8) and (12, 6, 4, 3),
// plain and with a small bigram model, two slots, cut into calls of every size from 1 to 7 frames and a call without rows, in an
// object made for exactly T frames (the trie and the table are filled to their ends) and with exactly sized outputs; the last
// call's records must be ss_ctc_beam_host's / ss_ctc_beam_lm_host's bytes.  Host code only; nothing here touches a device.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/ctc_stream_host_check.cpp streamspeech_amd/csrc/ctc_stream.hip streamspeech_amd/csrc/ctc_beam_host.hip \
//         streamspeech_amd/csrc/ctc_beam.hip streamspeech_amd/csrc/ngram_lm.hip -Lstreamspeech_amd -lstreamspeech_hip \
//         -o ctc_stream_host_check -fsanitize=address,undefined
//   LD_LIBRARY_PATH=streamspeech_amd ./ctc_stream_host_check
// (the four translation units under test are compiled into the program with the sanitizers; the rest of the library, which
// ss_ctc_stream_advance's model path refers to and this program never calls, comes from the built shared object)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/streamspeech_hip.h"

static std::vector<float> rows(uint32_t seed, int T, int V, float scale) {
  std::vector<float> x((size_t)T * V);
  uint32_t s = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < x.size(); ++i) {
    float u = 0.f;
    for (int k = 0; k < 4; ++k) { s = s * 1664525u + 1013904223u; u += (float)(s >> 8) / 16777216.f; }
    x[i] = (u - 2.f) * 1.7320508f * scale;                     // about normal
  }
  return x;
}

// unigrams for every id >= 2 and <s>, and one bigram per id: enough for a hit, a back-off and the eos term
static ss_ngram_lm* small_lm(int V) {
  std::vector<int32_t> tok;
  std::vector<float> logp, bo;
  int64_t counts[2] = {0, 0};
  for (int i = 0; i < V; ++i) {
    if (i == 1 || i == 3) continue;
    tok.push_back(i); logp.push_back(-1.f - 0.01f * (float)i); bo.push_back(-0.3f); ++counts[0];
  }
  for (int i = 4; i < V; ++i) { tok.push_back(i); tok.push_back(4 + (i * 7) % (V - 4)); logp.push_back(-0.5f); bo.push_back(0.f); ++counts[1]; }
  ss_ngram_lm* lm = nullptr;
  if (ss_ngram_lm_create(2, counts, tok.data(), logp.data(), bo.data(), V, 0, 2, -1, -20.f, &lm) != 0) return nullptr;
  return lm;
}

template <class Hyp>
static int check(const char* name, int T, int V, int beam, int cand, const ss_ngram_lm* lm) {
  const int nbest = beam;
  const ss_ctc_lm_opts opts{0.5, -0.1, 1};
  std::vector<float> x[2] = {rows(11, T, V, 2.f), rows(12, T, V, 6.f)};
  std::vector<Hyp> want[2];
  std::vector<int32_t> want_tok[2];
  for (int u = 0; u < 2; ++u) {
    want[u].assign(nbest, Hyp{});
    want_tok[u].assign((size_t)nbest * T, -7);
    const int32_t T1 = T;
    int rc;
    if constexpr (sizeof(Hyp) == sizeof(ss_ctc_beam_hyp))
      rc = ss_ctc_beam_host(x[u].data(), V, V, 1, 3, 1, &T1, beam, cand, nbest, want[u].data(), want_tok[u].data(), T, nullptr, nullptr);
    else
      rc = ss_ctc_beam_lm_host(x[u].data(), V, V, 1, 3, 1, &T1, beam, cand, nbest, want[u].data(), want_tok[u].data(), T, nullptr, nullptr,
                               lm, &opts);
    if (rc != 0) { printf("%s: one-shot rc %d\n", name, rc); return 1; }
  }
  ss_ctc_stream* cs = nullptr;
  if (ss_debug_ctc_stream_create(V, 1, 3, 0, 2, T, beam, cand, nbest, lm, lm ? &opts : nullptr, &cs) != 0) { printf("%s: create\n", name); return 1; }
  int bad = 0;
  for (int round = 0; round < 2 && !bad; ++round) {            // the second round reuses the slots the final calls reset
    int f[2] = {0, 0}, step = 0, prev_stable[2] = {0, 0};
    while (f[0] < T || f[1] < T) {
      const int32_t slots[2] = {1, 0};
      int32_t upto[2], fin[2];
      std::vector<float> stacked;
      int n = 0, who[2];
      for (int u = 0; u < 2; ++u) {
        if (f[u] >= T) continue;
        const int k = u == 1 && step % 3 == 2 ? 0 : 1 + (step + 3 * u) % 7;      // a call without rows now and then
        upto[n] = f[u] + k > T ? T : f[u] + k;
        fin[n] = upto[n] == T;
        stacked.insert(stacked.end(), x[u].begin() + (size_t)f[u] * V, x[u].begin() + (size_t)upto[n] * V);
        who[n++] = u;
      }
      if (stacked.empty()) stacked.push_back(0.f);
      int stride = 1;
      for (int i = 0; i < n; ++i) stride = upto[i] > stride ? upto[i] : stride;
      std::vector<Hyp> hyps((size_t)n * nbest);
      std::vector<int32_t> toks((size_t)n * nbest * stride, -7);         // exactly sized: a write past the end is the sanitizer's to find
      std::vector<ss_ctc_stream_part> part(n);
      int32_t sl[2];
      for (int i = 0; i < n; ++i) sl[i] = slots[who[i]];
      const int rc = ss_ctc_stream_advance_host(cs, n, sl, stacked.data(), V, upto, fin, hyps.data(), toks.data(), stride, part.data());
      if (rc != 0) { printf("%s: advance rc %d at step %d\n", name, rc, step); bad = 1; break; }
      for (int i = 0; i < n; ++i) {
        const int u = who[i];
        if (part[i].frames != upto[i] || part[i].status != 0 || part[i].n_stable < prev_stable[u] || part[i].n_alive < 1) { printf("%s: part\n", name); bad = 1; }
        prev_stable[u] = part[i].n_stable;
        f[u] = upto[i];
        if (!fin[i]) continue;
        for (int k = 0; k < nbest; ++k) {
          const Hyp &a = hyps[(size_t)i * nbest + k], &b = want[u][k];
          if (memcmp(&a, &b, sizeof(Hyp)) != 0 ||
              memcmp(&toks[((size_t)i * nbest + k) * stride], &want_tok[u][(size_t)k * T], (size_t)b.n_tokens * 4) != 0) {
            printf("%s: utterance %d hypothesis %d differs from the one-shot twin\n", name, u, k);
            bad = 1;
          }
        }
      }
      ++step;
    }
  }
  ss_ctc_stream_destroy(cs);
  printf("%s: %s\n", name, bad ? "FAILED" : "ok");
  return bad;
}

int main() {
  int bad = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const int T = pass ? 12 : 40, V = pass ? 6 : 64, beam = pass ? 4 : 8, cand = pass ? 3 : 8;
    ss_ngram_lm* lm = small_lm(V);
    if (!lm) { printf("model\n"); return 1; }
    bad |= check<ss_ctc_beam_hyp>(pass ? "plain 12/6/4/3" : "plain 40/64/8/8", T, V, beam, cand, nullptr);
    bad |= check<ss_ctc_beam_lm_hyp>(pass ? "lm 12/6/4/3" : "lm 40/64/8/8", T, V, beam, cand, lm);
    ss_ngram_lm_destroy(lm);
  }
  return bad;
}
