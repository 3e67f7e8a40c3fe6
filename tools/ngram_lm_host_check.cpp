// Stand-alone check of the n-gram model's host table builder (csrc/ngram_lm.hpp: the checks, the trie, the two suffix links, the
// slot placement) and of the lookup over it, for a sanitizer build of the host code: seeded models of order 1 .. 6 (sparse, so
// that suffixes are missing), a one-entry model, entry counts at and just past a power of two, every refused input, and
// sequences scored through the shared lookup against a std::map scorer written from the ARPA definition.  Host code only: the
// header has no kernel and makes no HIP call, and nothing here touches a device.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/ngram_lm_host_check.cpp -o ngram_lm_host_check -fsanitize=address,undefined
//   ./ngram_lm_host_check
#include <cstdio>
#include <map>
#include <vector>

#include "../streamspeech_amd/csrc/ngram_lm.hpp"

using namespace ss;
typedef std::vector<int32_t> Gram;

struct Model {
  int order = 0, V = 0;
  std::vector<int64_t> counts;
  std::vector<int32_t> tokens;
  std::vector<float> logp, backoff;
  std::map<Gram, std::pair<float, float>> grams;
  std::map<Gram, int> entry;
};

static uint32_t g_s = 1;
static uint32_t rnd(uint32_t n) { g_s = g_s * 1664525u + 1013904223u; return (g_s >> 8) % n; }
static float val(float lo, float hi) { return lo + (hi - lo) * (float)rnd(10000) / 10000.f; }

// Unigrams for the ids [2, V) but `skip`; order k: up to n random extensions of random (k - 1)-grams.  exact > 0: stop at that
// many n-grams in all.
static Model make(uint32_t seed, int order, int V, int n, int skip, long long exact = 0) {
  g_s = seed * 2654435761u + 7u;
  Model m;
  m.order = order; m.V = V;
  std::vector<std::vector<Gram>> by(order + 1);
  long long total = 0;
  auto add = [&](const Gram& g, int k) {
    m.grams[g] = {val(-7.f, -0.2f), k < order ? val(-2.f, 0.f) : 0.f};
    by[k].push_back(g);
    m.tokens.insert(m.tokens.end(), g.begin(), g.end());
    m.logp.push_back(m.grams[g].first); m.backoff.push_back(m.grams[g].second);
    m.entry[g] = (int)++total;
  };
  add(Gram{0}, 1);
  for (int c = 2; c < V; ++c)
    if (c != skip && (!exact || total < exact)) add(Gram{c}, 1);
  m.counts.push_back((int64_t)by[1].size());
  for (int k = 2; k <= order; ++k) {
    for (int tries = 0; tries < 20 * n && (int)by[k].size() < n && (!exact || total < exact); ++tries) {
      Gram g = by[k - 1][rnd((uint32_t)by[k - 1].size())];
      g.push_back(2 + (int32_t)rnd((uint32_t)(V - 2)));
      if (!m.grams.count(g)) add(g, k);
    }
    m.counts.push_back((int64_t)by[k].size());
  }
  return m;
}

static int build(const Model& m, NgramTable& t, int bos = 0, int eos = 2, int unk = 3, float oov = -20.f) {
  return ngram_build(m.order, m.counts.data(), m.tokens.data(), m.logp.data(), m.backoff.data(), m.V, bos, eos, unk, oov, t);
}

// p(c | h) from the ARPA definition over the map; *hist becomes the history after c.
static double ref_lp(const Model& m, Gram* hist, int c, int unk, double oov) {
  Gram h;
  const int keep = m.order - 1 < (int)hist->size() ? m.order - 1 : (int)hist->size();
  h.assign(hist->end() - keep, hist->end());
  double acc = 0.0;
  for (;;) {
    Gram g(h);
    g.push_back(c);
    auto it = m.grams.find(g);
    if (it != m.grams.end()) { hist->push_back(c); return acc + (double)it->second.first; }
    if (h.empty()) break;
    auto ih = m.grams.find(h);
    if (ih != m.grams.end()) acc += (double)ih->second.second;
    h.erase(h.begin());
  }
  auto iu = m.grams.find(Gram{unk});
  if (unk >= 0 && iu != m.grams.end()) { *hist = Gram{unk}; return acc + (double)iu->second.first; }
  hist->clear();
  return acc + oov;
}

static int check_model(const char* name, const Model& m, int unk) {
  NgramTable t;
  if (build(m, t, 0, 2, unk) != SS_OK) { printf("%s: refused\n", name); return 1; }
  long long n = 1;
  for (int64_t c : m.counts) n += c;
  if (t.entries != n || (t.mask + 1) < 2 * n || ((t.mask + 1) & t.mask) || (t.mask + 1 > 2 && (t.mask + 1) / 2 >= 2 * n)) { printf("%s: sizes\n", name); return 1; }
  int missing_suffix = 0;
  for (const auto& kv : m.entry) {                               // the links against a plain search for the longest suffix
    const Gram& g = kv.first;
    int suf = 0;
    for (size_t j = 1; j < g.size() && !suf; ++j) {
      auto it = m.entry.find(Gram(g.begin() + j, g.end()));
      if (it != m.entry.end()) suf = it->second; else ++missing_suffix;
    }
    const NgramEntry& e = t.ent[kv.second];
    if (ngram_walk(t, g.data(), (int)g.size()) != kv.second || e.backoff_state != suf ||
        e.next_state != ((int)g.size() < m.order ? kv.second : suf)) { printf("%s: links of entry %d\n", name, kv.second); return 1; }
  }
  const NgramView v = t.view();
  int checked = 0;
  for (int s = 0; s < 60; ++s) {
    const int len = s < 4 ? s : 1 + (int)rnd(40);
    std::vector<int32_t> seq(len);
    for (int j = 0; j < len; ++j) seq[j] = 2 + (int32_t)rnd((uint32_t)(m.V - 2));
    std::vector<double> lp(len + 1);
    std::vector<int32_t> st(len + 1);
    ngram_score_seq(v, seq.data(), len, 1, lp.data(), st.data());
    Gram hist;
    if (m.grams.count(Gram{0})) hist.push_back(0);
    for (int j = 0; j <= len; ++j) {
      const double want = ref_lp(m, &hist, j < len ? seq[j] : 2, unk, -20.0);
      if (lp[j] != want) { printf("%s: sequence %d token %d: %.17g, want %.17g\n", name, s, j, lp[j], want); return 1; }
      ++checked;
    }
  }
  printf("%s: ok, %d entries in %d slots, %d missing suffixes skipped, %d values equal\n", name, t.entries, t.mask + 1, missing_suffix, checked);
  return 0;
}

static int refused(const char* what, int rc, const NgramTable& t) {
  if (rc == SS_ERR_ARG && t.entries == 0 && t.keys.empty() && t.ent.empty()) return 0;
  printf("not refused: %s (rc %d)\n", what, rc);
  return 1;
}

int main() {
  int bad = 0;
  char name[64];
  for (int order = 1; order <= NGRAM_MAX_ORDER; ++order) {
    snprintf(name, sizeof(name), "order%d_unk", order);
    bad |= check_model(name, make(order, order, 40, 90, 5), 3);
    snprintf(name, sizeof(name), "order%d_oov", order);
    bad |= check_model(name, make(10 + order, order, 40, 90, 3), 3);      // no unigram for unk: oov_logp
  }
  bad |= check_model("entries_64", make(31, 3, 40, 20, -1, 63), 3);
  bad |= check_model("entries_65", make(31, 3, 40, 20, -1, 64), 3);
  {
    Model m;
    m.order = 1; m.V = 8; m.counts = {0};
    NgramTable t;
    if (build(m, t) != SS_OK || t.entries != 1 || t.mask != 1) { printf("one entry\n"); bad = 1; }
    int nx = -1;
    if (ngram_lp(t.view(), 0, 5, &nx) != -20.0 || nx != 0) { printf("one entry: lp\n"); bad = 1; }
  }
  // ---- every refusal, each on exactly sized arrays ----
  const Model g = make(77, 3, 16, 12, -1);
  NgramTable t;
  Model m = g;
  m.order = 0; bad |= refused("order 0", build(m, t), t);
  m = g; m.order = 7; m.counts.resize(7, 0); bad |= refused("order 7", build(m, t), t);
  m = g; m.tokens[(size_t)g.counts[0] + 1] = -1; bad |= refused("id -1", build(m, t), t);
  m = g; m.tokens[(size_t)g.counts[0] + 1] = 16; bad |= refused("id V", build(m, t), t);
  m = g; m.tokens[(size_t)g.counts[0] + 2] = m.tokens[(size_t)g.counts[0]]; m.tokens[(size_t)g.counts[0] + 3] = m.tokens[(size_t)g.counts[0] + 1];
  bad |= refused("duplicate", build(m, t), t);
  m = g; m.tokens[(size_t)g.counts[0]] = 1; bad |= refused("context not an entry", build(m, t), t);
  m = g; m.logp[4] = NAN; bad |= refused("logp NaN", build(m, t), t);
  m = g; m.backoff[4] = INFINITY; bad |= refused("backoff inf", build(m, t), t);
  bad |= refused("oov NaN", build(g, t, 0, 2, 3, NAN), t);
  bad |= refused("bos V", build(g, t, 16), t);
  bad |= refused("eos -2", build(g, t, 0, -2), t);
  m = g; m.counts[1] = -1; bad |= refused("negative count", build(m, t), t);
  m = g; m.order = 1; m.counts = {1LL << 30}; bad |= refused("2^30 + 1 entries", build(m, t), t);
  bad |= refused("no counts", ngram_build(1, nullptr, nullptr, nullptr, nullptr, 8, 0, 2, 3, -1.f, t), t);
  if (build(g, t) != SS_OK) { printf("the unchanged model\n"); bad = 1; }
  printf(bad ? "FAILED\n" : "all ok\n");
  return bad;
}
