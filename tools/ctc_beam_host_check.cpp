// Stand-alone check of the CTC prefix beam search's host twin (ss_ctc_beam_host, csrc/ctc_beam_host.hip) for a sanitizer build of the
// host code: two small cases, (T, V, beam, cand) = (12, 6, 4, 3) and (40, 64, 8, 8), in one ragged pack and alone, with guarded
// outputs.  Host code only; nothing here touches a device.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/ctc_beam_host_check.cpp streamspeech_amd/csrc/ctc_beam_host.hip -o ctc_beam_host_check -fsanitize=address,undefined
//   ./ctc_beam_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/streamspeech_hip.h"

static std::vector<float> rows(uint32_t seed, int T, int ld, int V, float scale) {
  std::vector<float> x((size_t)T * ld);
  uint32_t s = seed * 2654435761u + 12345u;
  for (int t = 0; t < T; ++t)
    for (int n = 0; n < ld; ++n) {
      float u = 0.f;
      for (int k = 0; k < 4; ++k) { s = s * 1664525u + 1013904223u; u += (float)(s >> 8) / 16777216.f; }
      x[(size_t)t * ld + n] = n < V ? (u - 2.f) * 1.7320508f * scale : 1e9f;      // about normal; past V: never read
    }
  return x;
}

static int run(const char* name, const std::vector<float>& x, int ld, int V, int B, const int32_t* T, int beam, int cand, int nbest,
               std::vector<ss_ctc_beam_hyp>& hyps, std::vector<int32_t>& toks) {
  int rows_n = 0, stride = 1;
  for (int b = 0; b < B; ++b) { rows_n += T[b]; stride = T[b] > stride ? T[b] : stride; }
  hyps.assign((size_t)B * nbest, ss_ctc_beam_hyp{0.0, -7, -7});
  toks.assign((size_t)B * nbest * stride, -7);                 // exactly sized: a write past the end is the sanitizer's to find
  std::vector<float> den(2 * (size_t)rows_n);
  std::vector<int32_t> cid((size_t)rows_n * cand);
  const int rc = ss_ctc_beam_host(x.data(), ld, V, 1, 3, B, T, beam, cand, nbest, hyps.data(), toks.data(), stride, den.data(), cid.data());
  if (rc != 0) { printf("%s: rc %d\n", name, rc); return 1; }
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < nbest; ++k) {
      const ss_ctc_beam_hyp& h = hyps[(size_t)b * nbest + k];
      if (h.status != 0 || h.n_tokens < 0 || h.n_tokens > T[b] || !(h.score <= 0.0) || (k && h.score > hyps[(size_t)b * nbest + k - 1].score)) {
        printf("%s: utterance %d slot %d: status %d n %d score %g\n", name, b, k, h.status, h.n_tokens, h.score);
        return 1;
      }
      for (int j = 0; j < h.n_tokens; ++j) {
        const int c = toks[((size_t)b * nbest + k) * stride + j];
        if (c < 2 || c == 3 || c >= V) { printf("%s: token %d\n", name, c); return 1; }
      }
    }
  printf("%s: ok, best %.6f (%d tokens)\n", name, hyps[0].score, hyps[0].n_tokens);
  return 0;
}

int main() {
  const int ld = 70;
  std::vector<float> a = rows(1, 12, ld, 6, 2.f), b = rows(2, 40, ld, 64, 6.f);
  std::vector<ss_ctc_beam_hyp> h1, h2, hp;
  std::vector<int32_t> t1, t2, tp;
  const int32_t Ta[1] = {12}, Tb[1] = {40};
  int bad = run("T12_V6_beam4_cand3", a, ld, 6, 1, Ta, 4, 3, 4, h1, t1);
  bad |= run("T40_V64_beam8_cand8", b, ld, 64, 1, Tb, 8, 8, 8, h2, t2);
  // the two as one ragged pack (V = 6 columns of both): the first utterance's records are the bytes it has alone
  std::vector<float> pack(a);
  pack.insert(pack.end(), b.begin(), b.end());
  const int32_t Tpk[2] = {12, 40};
  bad |= run("pack", pack, ld, 6, 2, Tpk, 4, 3, 4, hp, tp);
  if (!bad && memcmp(hp.data(), h1.data(), h1.size() * sizeof(ss_ctc_beam_hyp)) != 0) { printf("pack: records differ from the single call\n"); bad = 1; }
  int32_t T0[1] = {0};
  if (ss_ctc_beam_host(a.data(), ld, 6, 1, 3, 1, T0, 4, 3, 4, h1.data(), t1.data(), 12, nullptr, nullptr) != 2) { printf("refusal\n"); bad = 1; }
  printf(bad ? "FAILED\n" : "all ok\n");
  return bad;
}
