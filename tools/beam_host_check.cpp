// Stand-alone check of the text search's host stage (csrc/beam_host.hip: the planner of a call behind forced prefixes, the constraint
// table and the serial twin of the constraint selection) for a sanitizer build of the host code.  Every output buffer is sized
// exactly, so a write past an end is the sanitizer's to find.  Host code only; nothing here touches a device.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/beam_host_check.cpp streamspeech_amd/csrc/beam_host.hip -o beam_host_check -fsanitize=address,undefined
//   ./beam_host_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/streamspeech_hip.h"

static const int OK = 0, ERR_ARG = 2, ERR_CAPACITY = 4;
static int bad = 0;
#define CHECK(cond) do { if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); bad = 1; } } while (0)

static const int32_t Tp[3] = {9, 14, 11}, n_prefix[3] = {0, 2, 5}, max_len[3] = {8, 9, 12};
static const int32_t prefix_toks[7] = {10, 11, 20, 21, 22, 23, 24};
static const int V = 300, EOS = 2, PAD = 1;

// the plan of B = 3 behind prefixes of 0 / 2 / 5 tokens: dims first, then the tables into a buffer of exactly their size
static void plan(int beam, const ss_mt_search_opts* opts) {
  int32_t dims[8];
  int64_t n = -1;
  CHECK(ss_batch_mt_beam_continue_plan_opts(3, beam, Tp, prefix_toks, n_prefix, max_len, 1, 13, 13, 64, V, EOS, PAD, dims, nullptr, 0, &n,
                                            opts) == OK);
  const int pm = beam == 1 ? 1 : 0, R = 3 * beam, Tn = 8, Np = 7 + 3 * pm, nseg = 2 + pm;
  CHECK(dims[0] == 5 && dims[1] == Tn && dims[2] == 5 + Tn + 2 && dims[3] == Np && dims[4] == R && dims[5] == 5 && dims[6] == nseg &&
        dims[7] == pm);
  CHECK(n == 4 * R + (Tn + 1) * 4 * R + R + 3 + 8 * nseg + 5 * Np + 3);
  if (n < 0) return;
  std::vector<int32_t> tab((size_t)n, -7);
  CHECK(ss_batch_mt_beam_continue_plan_opts(3, beam, Tp, prefix_toks, n_prefix, max_len, 1, 13, 13, 64, V, EOS, PAD, dims, tab.data(), n,
                                            nullptr, opts) == OK);
  const int32_t* row0 = tab.data() + 4 * R + (Tn + 1) * 4 * R + R;
  CHECK(row0[0] == 0 && row0[1] == pm && row0[2] == 2 + 2 * pm);
  const int32_t* ptok = row0 + 3 + 8 * nseg;                     // </s> first, then the forced tokens but the last (pm = 0)
  const int32_t* ftok = ptok + 4 * Np;
  CHECK(ptok[row0[1]] == EOS && ptok[row0[1] + 1] == 10 && ftok[row0[1]] == 10 && ftok[row0[1] + 1] == 11);
  CHECK(ptok[row0[2]] == EOS && ptok[row0[2] + 4] == 23 && ftok[row0[2] + 4] == 24);
  for (int r = 0; r < R; ++r) CHECK(tab[4 * r] == r && tab[4 * r + 3] == Tp[r / beam]);
  if (n > 0)
    CHECK(ss_batch_mt_beam_continue_plan_opts(3, beam, Tp, prefix_toks, n_prefix, max_len, 1, 13, 13, 64, V, EOS, PAD, dims, tab.data(),
                                              n - 1, nullptr, opts) == ERR_CAPACITY);
}

static void plan_refusals() {
  int32_t dims[8];
  ss_mt_search_opts o{(int32_t)sizeof(ss_mt_search_opts), 2, 1.f, 1.f};
  plan(4, &o);                                                   // the prefixes above repeat no bigram
  const int32_t rep[4] = {7, 8, 7, 8}, n4[1] = {4}, ml[1] = {9};
  CHECK(ss_batch_mt_beam_continue_plan_opts(1, 4, Tp, rep, n4, ml, 1, 13, 13, 64, V, EOS, PAD, dims, nullptr, 0, nullptr, &o) == ERR_ARG);
  CHECK(ss_batch_mt_beam_continue_plan_opts(1, 4, Tp, rep, n4, ml, 1, 13, 13, 64, V, EOS, PAD, dims, nullptr, 0, nullptr, nullptr) == OK);
  ss_mt_search_opts shrt = o;
  shrt.size = (int32_t)sizeof(ss_mt_search_opts) - 4;            // a short struct is refused before the planner's row limit
  CHECK(ss_batch_mt_beam_continue_plan_opts(300, 1, Tp, rep, n4, ml, 1, 13, 13, 64, V, EOS, PAD, dims, nullptr, 0, nullptr, &shrt) == ERR_ARG);
  CHECK(ss_batch_mt_beam_continue_plan_opts(300, 1, Tp, rep, n4, ml, 1, 13, 13, 64, V, EOS, PAD, dims, nullptr, 0, nullptr, &o) == ERR_CAPACITY);
  CHECK(ss_batch_mt_beam_continue_plan(1, 33, Tp, rep, n4, ml, 1, 13, 13, 64, V, EOS, PAD, dims, nullptr, 0, nullptr) == ERR_ARG);
  CHECK(ss_batch_mt_beam_continue_plan(3, 4, Tp, prefix_toks, n_prefix, max_len, 1, 12, 13, 64, V, EOS, PAD, dims, nullptr, 0, nullptr) ==
        ERR_CAPACITY);                                           // out_stride below max_len + 1
  CHECK(ss_batch_mt_beam_continue_plan(3, 4, Tp, prefix_toks, nullptr, max_len, 1, 13, 13, 64, V, EOS, PAD, dims, nullptr, 0, nullptr) ==
        ERR_ARG);
}

// utterances of 0, 1 and 64 constraint tokens: the last a chain of 32 two-token phrases over 64 distinct ids
static void cons_table() {
  std::vector<int32_t> toks(65), end(65), off = {0, 0, 1, 65}, ml = {70, 70, 70};
  toks[0] = 9; end[0] = 1;
  for (int i = 0; i < 64; ++i) { toks[1 + i] = 100 + i; end[1 + i] = i & 1; }
  std::vector<int32_t> tab((size_t)3 * SS_MT_CONS_TABLE_LD, -7);
  CHECK(ss_mt_cons_table_host(3, toks.data(), off.data(), end.data(), V, PAD, EOS, ml.data(), tab.data()) == OK);
  const int32_t *r0 = tab.data(), *r1 = r0 + SS_MT_CONS_TABLE_LD, *r2 = r1 + SS_MT_CONS_TABLE_LD;
  CHECK(r0[SS_MT_CONS_MAX_TOKENS] == 0 && r0[SS_MT_CONS_MAX_TOKENS + 1] == 0);
  CHECK(r1[0] == 9 && r1[SS_MT_CONS_MAX_TOKENS] == 1 && r1[SS_MT_CONS_MAX_TOKENS + 1] == 1 && r1[SS_MT_CONS_MAX_TOKENS + 2] == 1);
  CHECK(r2[63] == 163 && r2[SS_MT_CONS_MAX_TOKENS] == 64 && r2[SS_MT_CONS_MAX_TOKENS + 1] == 64);
  CHECK((uint32_t)r2[SS_MT_CONS_MAX_TOKENS + 2] == 0xAAAAAAAAu && (uint32_t)r2[SS_MT_CONS_MAX_TOKENS + 3] == 0xAAAAAAAAu);
  ml[2] = 63;                                                    // more constraint tokens than the utterance may hold
  CHECK(ss_mt_cons_table_host(3, toks.data(), off.data(), end.data(), V, PAD, EOS, ml.data(), tab.data()) == ERR_ARG);
  end[64] = 0;                                                   // the last phrase is open
  CHECK(ss_mt_cons_table_host(3, toks.data(), off.data(), end.data(), V, PAD, EOS, nullptr, nullptr) == ERR_ARG);
  const int32_t off65[2] = {0, 65};
  std::vector<int32_t> t65(65, 50), e65(65, 1);
  CHECK(ss_mt_cons_table_host(1, t65.data(), off65, e65.data(), V, PAD, EOS, nullptr, nullptr) == ERR_ARG);
}

// k = 2, V = 7, one phrase (4, 5): the selection of step 0 from the root row, and of step 1 from one started and one idle row
static void cons_select() {
  const int k = 2, Vs = 7;
  const int32_t cons[2] = {4, 5}, end[2] = {0, 1};
  const float lp0[7] = {-9.f, -INFINITY, -2.5f, -1.f, -3.f, -0.5f, -2.f}, cum0[2] = {0.f, 0.f};
  const int32_t st0[2] = {-1, -1};
  std::vector<float> s(2 * k, NAN);
  std::vector<int32_t> t(2 * k, -7), b(2 * k, -7), ns(2 * k, -7);
  CHECK(ss_mt_cons_select_host(lp0, cum0, k, Vs, 0, EOS, st0, cons, 2, end, s.data(), t.data(), b.data(), ns.data()) == OK);
  bool started = false;
  for (int q = 0; q < 2 * k; ++q) {
    CHECK(t[q] >= 0 && t[q] < Vs && b[q] == 0 && ns[q] >= -1 && ns[q] <= 1 && s[q] == lp0[t[q]]);
    CHECK((ns[q] == 0) == (t[q] == 4));
    started = started || t[q] == 4;
  }
  CHECK(started && t[0] == 4);                                   // the phrase's first token leads: the highest bank first
  const float lp1[14] = {-9.f, -INFINITY, -0.1f, -1.f, -3.f, -2.5f, -2.f, -9.f, -INFINITY, -0.2f, -1.5f, -3.f, -0.5f, -2.f};
  const float cum1[2] = {-3.f, -0.5f};
  const int32_t st1[2] = {0, -1};
  CHECK(ss_mt_cons_select_host(lp1, cum1, k, Vs, 1, EOS, st1, cons, 2, end, s.data(), t.data(), b.data(), ns.data()) == OK);
  bool finished = false;
  for (int q = 0; q < 2 * k; ++q) {
    CHECK(t[q] >= 0 && t[q] < Vs && b[q] >= 0 && b[q] < k && ns[q] >= -1 && ns[q] <= 1);
    if (t[q] == EOS) CHECK(s[q] == -INFINITY);                   // no row has met the constraint: </s> is banned in both
    else CHECK(s[q] == lp1[b[q] * Vs + t[q]] + cum1[b[q]]);
    finished = finished || (b[q] == 0 && t[q] == 5 && ns[q] == 1);
  }
  CHECK(finished && ns[0] == 1);
  const int32_t st_bad[2] = {2, -1};
  CHECK(ss_mt_cons_select_host(lp1, cum1, k, Vs, 1, EOS, st_bad, cons, 2, end, s.data(), t.data(), b.data(), ns.data()) == ERR_ARG);
  CHECK(ss_mt_cons_select_host(lp1, cum1, k, 4, 1, EOS, st1, cons, 2, end, s.data(), t.data(), b.data(), ns.data()) == ERR_ARG);
}

int main() {
  plan(4, nullptr);
  plan(1, nullptr);                                              // beam 1: the pm = 1 layout, one more prefix-pass row per utterance
  plan_refusals();
  cons_table();
  cons_select();
  printf(bad ? "FAILED\n" : "all ok\n");
  return bad;
}
