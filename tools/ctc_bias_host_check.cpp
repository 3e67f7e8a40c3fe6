// Stand-alone check of the hotword set's host builder (csrc/ctc_bias.hpp: the checks, the trie, held / floor, the fail links, the
// occurrence rule, the slot placement) and of the step over it, for a sanitizer build of the host code: seeded phrase sets over
// small and large alphabets (prefix nesting, suffixes that are other phrases' prefixes), an empty set, node counts at and just
// past a power of two, the caps, every refused input, and sequences walked through bias_step against a naive scorer that finds
// the state as the longest suffix in a std::map, with no fail links.  Host code only: the header has no kernel and makes no HIP
// call, and nothing here touches a device.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/ctc_bias_host_check.cpp -o ctc_bias_host_check -fsanitize=address,undefined
//   ./ctc_bias_host_check
#include <cstdio>
#include <map>
#include <vector>

#include "../streamspeech_amd/csrc/ctc_bias.hpp"

using namespace ss;
typedef std::vector<int32_t> Str;

struct Set {
  int V = 0;
  std::vector<Str> phrases;
  std::vector<float> boost;
  std::vector<int32_t> tokens, off;
  void pack() {
    tokens.clear(); off.assign(1, 0);
    for (const Str& p : phrases) { tokens.insert(tokens.end(), p.begin(), p.end()); off.push_back((int32_t)tokens.size()); }
  }
};

static uint32_t g_s = 1;
static uint32_t rnd(uint32_t n) { g_s = g_s * 1664525u + 1013904223u; return (g_s >> 8) % n; }
static float val(float lo, float hi) { return lo + (hi - lo) * (float)rnd(10000) / 10000.f; }

static bool inside(const Str& p, const Str& q) {                 // p occurs in q at a position other than its start
  for (size_t i = 1; i + p.size() <= q.size(); ++i)
    if (std::equal(p.begin(), p.end(), q.begin() + i)) return true;
  return false;
}

static bool admissible(const std::vector<Str>& ps, const Str& p) {
  for (const Str& q : ps)
    if (q == p || inside(p, q) || inside(q, p)) return false;
  return true;
}

// Up to n phrases of 1 .. max_len labels from [lo, V); every third extends an earlier one; a phrase that breaks a rule is drawn again.
static Set make(uint32_t seed, int V, int lo, int n, int max_len, int exact_nodes = 0) {
  g_s = seed * 2654435761u + 7u;
  Set s;
  s.V = V;
  std::map<Str, int> nodes;
  for (int tries = 0; tries < 40 * n && (int)s.phrases.size() < n; ++tries) {
    Str p;
    if (!s.phrases.empty() && s.phrases.size() % 3 == 2) p = s.phrases[rnd((uint32_t)s.phrases.size())];
    const int more = 1 + (int)rnd(p.empty() ? (uint32_t)max_len : 2u);
    for (int j = 0; j < more; ++j) p.push_back(lo + (int32_t)rnd((uint32_t)(V - lo)));
    if ((int)p.size() > CTC_BIAS_MAX_LEN || !admissible(s.phrases, p)) continue;
    if (exact_nodes) {
      std::map<Str, int> t = nodes;
      for (size_t k = 1; k <= p.size(); ++k) t[Str(p.begin(), p.begin() + k)] = 1;
      if ((int)t.size() + 1 > exact_nodes) continue;
      nodes = t;
    }
    s.phrases.push_back(p);
    s.boost.push_back(val(-1.f, 3.f));
    if (exact_nodes && (int)nodes.size() + 1 == exact_nodes) break;
  }
  s.pack();
  return s;
}

static int build(const Set& s, BiasTable& t, int pad = 1, int unk = 3) {
  return bias_build((int)s.phrases.size(), s.tokens.data(), s.off.data(), s.boost.data(), s.V, pad, unk, t);
}

struct Naive {
  std::map<Str, double> held, floor_;
  std::map<Str, float> boost;
  std::map<Str, bool> end;
  explicit Naive(const Set& s) {
    for (size_t p = 0; p < s.phrases.size(); ++p) {
      for (size_t k = 1; k <= s.phrases[p].size(); ++k) {
        const Str pre(s.phrases[p].begin(), s.phrases[p].begin() + k);
        auto it = boost.find(pre);
        if (it == boost.end() || s.boost[p] > it->second) boost[pre] = s.boost[p];
      }
      end[s.phrases[p]] = true;
    }
    held[Str()] = 0.0; floor_[Str()] = 0.0;
    for (int len = 1; len <= CTC_BIAS_MAX_LEN; ++len)
      for (const auto& kv : boost) {
        if ((int)kv.first.size() != len) continue;
        const Str par(kv.first.begin(), kv.first.end() - 1);
        held[kv.first] = held[par] + (double)kv.second;
        floor_[kv.first] = end.count(kv.first) ? held[kv.first] : floor_[par];
      }
  }
  Str state(const Str& y) const {                                // the longest suffix of y that is a node
    const size_t most = y.size() < (size_t)CTC_BIAS_MAX_LEN ? y.size() : (size_t)CTC_BIAS_MAX_LEN;
    for (size_t k = most;; --k) {
      const Str suf(y.end() - k, y.end());
      if (held.count(suf)) return suf;
    }
  }
};

static int check_set(const char* name, const Set& s) {
  BiasTable t;
  if (build(s, t) != SS_OK) { printf("%s: refused\n", name); return 1; }
  const Naive nv(s);
  const long long n = (long long)nv.held.size();
  if (t.nodes != n || t.phrases != (int)s.phrases.size() || (t.mask + 1) < 2 * n || ((t.mask + 1) & t.mask) ||
      (t.mask + 1 > 2 && (t.mask + 1) / 2 >= 2 * n) || (long long)t.node.size() != n) { printf("%s: sizes\n", name); return 1; }
  std::map<int, Str> str_of;                                     // node id -> its string, by walking every phrase through the table
  str_of[0] = Str();
  for (const Str& p : s.phrases) {
    int st = 0;
    for (size_t k = 0; k < p.size(); ++k) {
      st = ctc_beam_find(t.keys.data(), t.vals.data(), t.mask, st, p[k]);
      if (st < 0) { printf("%s: a phrase prefix is not a node\n", name); return 1; }
      str_of[st] = Str(p.begin(), p.begin() + k + 1);
    }
    if (!t.node[st].terminal) { printf("%s: terminal\n", name); return 1; }
  }
  if ((long long)str_of.size() != n) { printf("%s: node count\n", name); return 1; }
  for (const auto& kv : str_of) {                                // every field against the definition
    const BiasNode& e = t.node[kv.first];
    const Str& y = kv.second;
    Str fail;
    if (!y.empty()) fail = nv.state(Str(y.begin() + 1, y.end()));
    if (e.held != nv.held.at(y) || e.floor != nv.floor_.at(y) || str_of.at(e.fail) != fail || (e.terminal != 0) != (nv.end.count(y) != 0)) {
      printf("%s: fields of node %d\n", name, kv.first);
      return 1;
    }
  }
  const BiasView v = t.view();
  int checked = 0;
  for (int q = 0; q < 80; ++q) {
    Str y;
    const int parts = q < 2 ? q : 1 + (int)rnd(8);
    for (int k = 0; k < parts; ++k) {
      if (!s.phrases.empty() && rnd(4) != 0) {
        const Str& p = s.phrases[rnd((uint32_t)s.phrases.size())];
        const size_t take = rnd(3) == 0 ? 1 + rnd((uint32_t)p.size()) : p.size();
        y.insert(y.end(), p.begin(), p.begin() + take);
      } else {
        y.push_back(2 + (int32_t)rnd((uint32_t)(s.V - 2)));
      }
    }
    std::vector<double> delta(y.size() + 1);
    std::vector<int32_t> st(y.size() + 1);
    for (int finish = 0; finish < 2; ++finish) {
      double sum = -1.0;
      bias_score_seq(v, y.data(), (int)y.size(), finish, delta.data(), st.data(), &sum);
      Str cur;
      double acc = 0.0;
      for (size_t j = 0; j < y.size(); ++j) {
        const Str nx = nv.state(Str(y.begin(), y.begin() + j + 1));
        Str direct(cur);
        direct.push_back(y[j]);
        double want = nv.held.at(nx) - nv.held.at(cur);
        if (nx != direct) want = want + nv.floor_.at(cur);
        if (delta[j] != want || str_of.at(st[j]) != nx) { printf("%s: sequence %d token %d\n", name, q, (int)j); return 1; }
        acc += want;
        cur = nx;
        ++checked;
      }
      const double want_sum = finish ? acc - (nv.held.at(cur) - nv.floor_.at(cur)) : acc;
      if (sum != want_sum) { printf("%s: sequence %d sum %.17g, want %.17g\n", name, q, sum, want_sum); return 1; }
    }
  }
  printf("%s: ok, %d phrases, %d nodes in %d slots, %d steps equal\n", name, t.phrases, t.nodes, t.mask + 1, checked);
  return 0;
}

static int refused(const char* what, int rc, const BiasTable& t) {
  if (rc == SS_ERR_ARG && t.nodes == 0 && t.keys.empty() && t.node.empty()) return 0;
  printf("not refused: %s (rc %d)\n", what, rc);
  return 1;
}

int main() {
  int bad = 0;
  char name[64];
  for (int k = 0; k < 12; ++k) {
    snprintf(name, sizeof(name), "small_%d", k);
    bad |= check_set(name, make(k + 1, 6 + k % 3, 4, 3 + k % 5, 4));
    snprintf(name, sizeof(name), "wide_%d", k);
    bad |= check_set(name, make(100 + k, 400, 4, 60, 6));
  }
  bad |= check_set("nodes_32", make(31, 50, 4, 40, 4, 32));
  bad |= check_set("nodes_33", make(31, 50, 4, 40, 4, 33));
  {
    Set s;
    s.V = 8;
    s.pack();
    BiasTable t;
    if (bias_build(0, nullptr, nullptr, nullptr, 8, 1, 3, t) != SS_OK || t.nodes != 1 || t.mask != 1) { printf("empty set\n"); bad = 1; }
    int nx = -1;
    if (bias_step(t.view(), 0, 5, &nx) != 0.0 || nx != 0 || bias_open(t.view(), 0) != 0.0) { printf("empty set: step\n"); bad = 1; }
  }
  {                                                              // the caps: 4096 phrases of 32 tokens that share nothing but the head
    Set s;
    s.V = 5000;
    for (int p = 0; p < CTC_BIAS_MAX_PHRASES; ++p) {
      Str y(1, 4 + p);
      for (int j = 1; j < CTC_BIAS_MAX_LEN; ++j) y.push_back(4500 + (p * 7 + j * 13) % 400);
      s.phrases.push_back(y);
      s.boost.push_back(1.f + (float)(p % 5));
    }
    s.pack();
    BiasTable t;
    if (build(s, t) != SS_OK || t.nodes != 1 + CTC_BIAS_MAX_PHRASES * CTC_BIAS_MAX_LEN) { printf("caps\n"); bad = 1; }
    s.phrases.push_back(Str{4999, 4998}); s.boost.push_back(1.f); s.pack();
    bad |= refused("4097 phrases", build(s, t), t);
  }
  // ---- every refusal, each on exactly sized arrays ----
  Set g;
  g.V = 16;
  g.phrases = {Str{4, 5}, Str{4, 5, 6}, Str{7}, Str{8, 9, 10}};
  g.boost = {1.f, 2.f, -1.f, 0.5f};
  g.pack();
  BiasTable t;
  Set m = g;
  m.phrases[2].clear(); m.pack(); bad |= refused("an empty phrase", build(m, t), t);
  m = g; m.phrases[0][1] = -1; m.pack(); bad |= refused("id -1", build(m, t), t);
  m = g; m.phrases[0][1] = 16; m.pack(); bad |= refused("id V", build(m, t), t);
  m = g; m.phrases[0][1] = 0; m.pack(); bad |= refused("blank", build(m, t), t);
  m = g; m.phrases[0][1] = 1; m.pack(); bad |= refused("pad", build(m, t), t);
  m = g; m.phrases[2][0] = 3; m.pack(); bad |= refused("unk", build(m, t), t);
  m = g; m.phrases[3] = Str{4, 5}; m.pack(); bad |= refused("duplicate", build(m, t), t);
  m = g; m.boost[1] = NAN; bad |= refused("boost NaN", build(m, t), t);
  m = g; m.boost[3] = -INFINITY; bad |= refused("boost -inf", build(m, t), t);
  m = g; m.phrases[3] = Str(33, 11); m.pack(); bad |= refused("33 tokens", build(m, t), t);
  m = g; m.phrases[3] = Str{8, 7, 10}; m.pack(); bad |= refused("a phrase inside another", build(m, t), t);
  m = g; m.phrases[3] = Str{8, 4, 5}; m.pack(); bad |= refused("a phrase at the end of another", build(m, t), t);
  m = g; m.phrases[2] = Str{5, 6}; m.pack(); bad |= refused("a phrase inside a prefix-nested one", build(m, t), t);
  m = g; m.off[0] = 1; bad |= refused("offsets from 1", build(m, t), t);
  m = g; m.off[2] = m.off[1]; bad |= refused("offsets that do not ascend", build(m, t), t);
  m = g; m.V = 0; bad |= refused("V 0", build(m, t), t);
  bad |= refused("pad V", build(g, t, 16), t);
  bad |= refused("unk -2", build(g, t, 1, -2), t);
  bad |= refused("no tokens", bias_build(2, nullptr, g.off.data(), g.boost.data(), 16, 1, 3, t), t);
  bad |= refused("negative count", bias_build(-1, nullptr, nullptr, nullptr, 16, 1, 3, t), t);
  if (build(g, t) != SS_OK) { printf("the unchanged set\n"); bad = 1; }
  bad |= check_set("the unchanged set", g);
  printf(bad ? "FAILED\n" : "all ok\n");
  return bad;
}
