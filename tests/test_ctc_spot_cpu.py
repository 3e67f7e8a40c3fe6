"""Keyword spotting on the CTC heads without a device: the host twin (ss_ctc_spot_host, ss_debug_ctc_spot_trace_host,
ss_ctc_spot_stream_advance_host) against the two float64 references of tests/ctc_spot_ref.py -- e_t equal to the brute force over
every (start, end), hits, starts and order byte-equal to the restated rule -- on random and on constructed logits, every refusal,
the resumable twin on every composition of a 12-frame utterance, and the Python layers that need no device.  The check_*
functions and the cases run again on the kernels in tests/test_ctc_spot_gpu.py."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from tests import ctc_spot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, UNK = 1, 3
A, B_, C_, D_ = 2, 4, 5, 3                                    # labels of the constructed cases (D_ is unk: legal in a keyword)


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def random_logits(seed, T, V, scale=2.0):
    return (np.random.default_rng(seed).standard_normal((T, V)) * scale).astype(np.float32)


def quarter_logits(seed, T, V):
    """Multiples of 0.25 in [-2, 0]: sums are exact, so equal scores are real ties."""
    return (np.random.default_rng(seed).integers(-8, 1, (T, V)) * 0.25).astype(np.float32)


def labels_of(V):
    return [v for v in range(2, V) if v != PAD]


def keyword_set(name, V):
    """-> (phrases, taus) of a named set over a head of V columns."""
    rng = np.random.default_rng(sum(map(ord, name)) + V)
    lab = labels_of(V)
    pick = lambda n: [int(x) for x in rng.choice(lab, n)]     # noqa: E731
    if name == "one":
        return [pick(2)], [4.0]
    if name == "five":                                        # shared labels: L = 1, a repeated label (no skip), L = 32, two equal
        a, b, c = lab[0], lab[1], lab[2]
        return [[a], [a, a], pick(32), [a, b, c], [a, b, c]], [3.0, 3.0, 5.0, 2.5, 4.0]
    if name == "disjoint":
        p = [int(x) for x in rng.permutation(lab)[:10]]
        return [p[0:1], p[1:3], p[3:6], p[6:10]], [3.0, 3.0, 4.0, 4.0]
    if name == "300":
        return [pick(int(rng.integers(1, 7))) for _ in range(300)], [float(t) for t in rng.choice([2.0, 3.0, 4.0], 300)]
    if name == "257x1":                                       # one keyword more than a workgroup of the DP kernel owns
        return [[lab[i % len(lab)]] for i in range(257)], [1.0 + 0.01 * (i % 50) for i in range(256)] + [50.0]   # (the last one always hits)
    raise KeyError(name)


CASES = [(name, V, T, kind) for name, V, T, kind in
         [("one", 37, 1, "q"), ("one", 37, 2, "r"), ("one", 37, 40, "r"),
          ("five", 37, 1, "r"), ("five", 37, 2, "q"), ("five", 37, 3, "q"), ("five", 37, 40, "r"), ("five", 37, 40, "q"),
          ("disjoint", 37, 40, "r"), ("disjoint", 37, 3, "r"),
          ("300", 37, 40, "q"), ("257x1", 37, 3, "r"),
          ("five", 6004, 40, "r")]]
BRUTE = {("one", 37), ("five", 37), ("disjoint", 37)}        # where reference (a) runs as well


def case_logits(name, V, T, kind):
    seed = 100 + T + len(name)
    return quarter_logits(seed, T, V) if kind == "q" else random_logits(seed, T, V)


def check_one_shot(lib, x, phrases, taus, V, gpu=False, max_hits=4096):
    """The call's records against reference (b), byte for byte -> the records."""
    status, want = R.spot(x, phrases, taus)
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks:
        assert ks.rc == 0
        rc, hits, counts = R.run(lib, ks, [x], max_hits, gpu=gpu)
    assert rc == 0
    assert (int(counts["n_hits"][0]), int(counts["status"][0]), int(counts["overflow"][0]), int(counts["frames"][0])) == \
        (len(want), status, 0, x.shape[0])
    got = R.written(hits, counts)
    assert got.tobytes() == want.tobytes()
    return got


@pytest.mark.parametrize("name,V,T,kind", CASES)
def test_host_twin_against_the_restated_rule(lib, name, V, T, kind):
    phrases, taus = keyword_set(name, V)
    got = check_one_shot(lib, case_logits(name, V, T, kind), phrases, taus, V)
    if T == 40 and name in ("five", "300", "disjoint"):
        assert len(got) > 0                                   # the case is not empty
    if name == "five" and T < 32:
        assert not (got["keyword"] == 2).any()                # a keyword that cannot fit in T


@pytest.mark.parametrize("name,V,T,kind", [c for c in CASES if (c[0], c[1]) in BRUTE])
def test_trace_against_brute_force(lib, name, V, T, kind):
    """e_t of the twin == max over start of the pinned Viterbi, exactly, for every t; its start is one of the maximisers; and both
    are reference (b)'s (which on multiples of 0.25 pins the tie rules)."""
    phrases, taus = keyword_set(name, V)
    x = case_logits(name, V, T, kind)
    c, bad = R.costs(x)
    assert not bad.any()
    tr = {}
    R.spot(x, phrases, taus, trace=tr)
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks:
        rc, e, s = R.trace(lib, ks, x)
    assert rc == 0
    finite = 0
    for k, y in enumerate(phrases):
        P = R.brute(c, y)
        for t in range(T):
            assert e[t, k] == P[:, t].max()
            assert (e[t, k], s[t, k]) == tr[k][t]
            if e[t, k] > R.NEG:
                assert P[s[t, k], t] == e[t, k]
                finite += 1
    assert finite > 0 or T < 3


# ---- constructed logits: multiples of 0.25 ----------------------------------------------------------------------------------------
def rows(V, spec, low=-2.0):
    """One row per entry of spec: {column: value} over a floor of `low`."""
    x = np.full((len(spec), V), low, np.float32)
    for t, d in enumerate(spec):
        for v, val in d.items():
            x[t, v] = val
    return x


def spans(rec):
    return [(int(r["keyword"]), int(r["start"]), int(r["end"]), float(r["score"])) for r in rec]


def constructed():
    """name -> (logits, phrases, taus, the hits expected as (keyword, start, end, score))."""
    V = 6
    out = {}
    # a phrase that occurs twice gives two hits
    out["twice"] = (rows(V, [{A: 0}, {B_: 0}, {0: 0}, {C_: 0}, {C_: 0}, {A: 0}, {B_: 0}]), [[A, B_]], [0.5],
                    [(0, 0, 1, 0.0), (0, 5, 6, 0.0)])
    # overlapping candidates give one hit, the best: the later frame scores lower and does not replace it
    out["best"] = (rows(V, [{A: 0}, {B_: 0}, {C_: 0, B_: -0.25}, {C_: 0}]), [[A, B_]], [1.0], [(0, 0, 1, 0.0)])
    # ... and a later EQUAL one wins: the span covers the last label's run
    out["later_equal"] = (rows(V, [{A: 0}, {C_: 0, B_: -0.25}, {B_: 0}, {C_: 0}]), [[A, B_]], [1.0], [(0, 0, 2, -0.25)])
    # a first label that stays the arg-max for several frames keeps the early start
    out["early_start"] = (rows(V, [{C_: 0}, {A: 0}, {A: 0}, {A: 0}, {B_: 0}, {C_: 0}]), [[A, B_], [A]], [0.5, 0.5],
                          [(1, 1, 3, 0.0), (0, 1, 4, 0.0)])
    # a candidate whose start lies inside an emitted hit is ignored (frame 3: e = -2 from start 0, after (0, 1) was emitted)
    out["inside"] = (rows(V, [{A: 0}, {B_: 0}, {0: 0, A: -3, B_: -3, C_: -3, D_: -3, PAD: -3}, {B_: 0}]), [[A, B_]], [1.25],
                     [(0, 0, 1, 0.0)])
    # per-phrase tau is honoured: the same phrase at 0.25 and at 1.0 per label, on a path that costs 1.0
    out["tau"] = (rows(V, [{A: 0}, {C_: 0, B_: -1.0}, {C_: 0}]), [[A, B_], [A, B_]], [0.25, 1.0], [(1, 0, 1, -1.0)])
    # unk is not masked
    out["unk"] = (rows(V, [{D_: 0}, {A: 0}, {C_: 0}]), [[D_, A]], [0.5], [(0, 0, 1, 0.0)])
    return V, out


@pytest.mark.parametrize("name", sorted(constructed()[1]))
def test_constructed_logits(lib, name):
    V, cases = constructed()
    x, phrases, taus, want = cases[name]
    assert spans(check_one_shot(lib, x, phrases, taus, V)) == want


def check_bad_rows(lib, gpu=False):
    V = 37
    phrases, taus = keyword_set("five", V)
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks:
        xs = [random_logits(5, 20, V), random_logits(6, 20, V), random_logits(7, 20, V), random_logits(8, 1, V)]
        rc, h0, c0 = R.run(lib, ks, xs, 64, gpu=gpu)
        assert rc == 0 and c0["n_hits"][0] > 0 and (c0["status"] == 0).all()
        xs[1][13, 5] = np.nan
        xs[2][0, :] = -np.inf
        xs[3][0, V - 1] = np.nan
        rc, h1, c1 = R.run(lib, ks, xs, 64, gpu=gpu)
        assert rc == 0
        assert c1["status"].tolist() == [0, 2, 2, 2] and c1["n_hits"][1:].tolist() == [0, 0, 0]
        assert R.written(h1, c1, 0).tobytes() == R.written(h0, c0, 0).tobytes()     # the neighbour is untouched by them
        xs[0][3, 2] = -np.inf                                                        # a -inf entry is no bad row
        rc, h2, c2 = R.run(lib, ks, xs[:1], 64, gpu=gpu)
        assert rc == 0 and c2["status"][0] == 0
        assert R.written(h2, c2).tobytes() == R.spot(xs[0], phrases, taus)[1].tobytes()


def test_bad_rows(lib):
    check_bad_rows(lib)


def check_overflow(lib, gpu=False):
    V = 6
    x = rows(V, [{A: 0}, {C_: 0}, {A: 0}, {C_: 0}, {A: 0}])
    with R.KeywordSet(lib, [[A]], [0.5], V, PAD, UNK) as ks:
        rc, hits, counts = R.run(lib, ks, [x], 8, gpu=gpu)
        assert rc == 0 and counts["n_hits"][0] == 3 and counts["overflow"][0] == 0
        three = [h.tobytes() for h in hits[0, :3]]
        rc, hits, counts = R.run(lib, ks, [x], 1, gpu=gpu)
        assert rc == 0 and counts["n_hits"][0] == 3 and counts["overflow"][0] == 1
        assert hits[0, 0].tobytes() in three


def test_overflow(lib):
    check_overflow(lib)


def check_pack(lib, gpu=False):
    """An utterance's records are the same bytes alone, in a pack and in the reversed pack."""
    V = 37
    phrases, taus = keyword_set("300", V)
    xs = [random_logits(40 + i, T, V) for i, T in enumerate((23, 1, 40, 7, 17))]
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks:
        alone = []
        for x in xs:
            rc, h, c = R.run(lib, ks, [x], 4096, gpu=gpu)
            assert rc == 0 and c["overflow"][0] == 0          # (past max_hits WHICH records are written is unspecified)
            alone.append((R.written(h, c).tobytes(), c[0].tobytes()))
        for order in (list(range(5)), list(range(4, -1, -1))):
            rc, h, c = R.run(lib, ks, [xs[i] for i in order], 4096, gpu=gpu, ld=V + 3)
            assert rc == 0
            for j, i in enumerate(order):
                assert (R.written(h, c, j).tobytes(), c[j].tobytes()) == alone[i]
    assert sum(len(a[0]) for a in alone) > 0


def test_pack(lib):
    check_pack(lib)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_set_refusals(lib):
    V = 37
    ok = [[5, 6], [7]]
    bad_sets = [([], []), ([[]], [1.0]), ([list(range(4, 37))], [1.0]), ([[5, 0]], [1.0]), ([[PAD]], [1.0]), ([[-1]], [1.0]),
                ([[V]], [1.0]), (ok, [1.0, -0.5]), (ok, [float("nan"), 1.0]), (ok, [1.0, float("inf")])]
    for phrases, taus in bad_sets:
        ks = R.KeywordSet(lib, phrases, taus, V, PAD, UNK)
        assert ks.rc == 2 and not ks.h, (phrases, taus)
    for V_, pad, unk in ((0, -1, -1), (37, 37, -1), (37, -2, -1), (37, -1, 37)):
        assert R.KeywordSet(lib, ok, [1.0, 1.0], V_, pad, unk).rc == 2
    with R.KeywordSet(lib, ok + [[UNK] * 32], [1.0, 0.0, 1.0], V, PAD, UNK) as ks:       # unk, L = 32 and tau = 0 are legal
        assert ks.rc == 0
        assert ks.info() == {"keywords": 3, "labels": 5, "states": 3 + 1 + 63, "workgroups": 1, "bytes": ks.info()["bytes"]}
    with R.KeywordSet(lib, *keyword_set("257x1", V), V, PAD, UNK) as ks:
        assert ks.info()["workgroups"] == 2


def check_call_refusals(lib, gpu=False):
    V = 37
    x = random_logits(1, 9, V)
    with R.KeywordSet(lib, [[5, 6]], [1.0], V, PAD, UNK) as ks:
        fill = bytes([R.FILL])
        for kw in (dict(xs=[], max_hits=4), dict(xs=[x], max_hits=0), dict(xs=[x], max_hits=16385), dict(xs=[x], max_hits=4, T=[0]),
                   dict(xs=[x, x], max_hits=4, T=[9, 1501]), dict(xs=[x], max_hits=4, ld=V - 1)):
            rc, hits, counts = R.run(lib, ks, gpu=gpu, **kw)
            assert rc == 2, kw
            assert hits.tobytes() == fill * hits.nbytes and counts.tobytes() == fill * counts.nbytes
    if not gpu:
        assert lib.ss_ctc_spot_host(None, V, 1, (C.c_int32 * 1)(9), None, 4, None, None) == 2


def test_call_refusals(lib):
    check_call_refusals(lib)


# ---- the resumable twin -----------------------------------------------------------------------------------------------------------
def stream_case():
    V = 8
    phrases = [[A], [A, B_], [B_, B_], [C_, A, B_], [A, B_]]
    taus = [0.5, 0.75, 1.0, 1.0, 0.25]
    x = quarter_logits(12, 12, V)
    x[np.arange(12), [A, A, B_, 0, B_, C_, A, B_, B_, A, 6, B_]] = 0.0        # an arg-max path with the phrases on it
    return V, phrases, taus, x


def check_splits(lib, V, phrases, taus, x, cut_sets, gpu=False):
    status, want = R.spot(x, phrases, taus)
    assert status == 0 and len(want) >= 3
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks:
        rc, hits, counts = R.run(lib, ks, [x], 64, gpu=gpu)
        assert rc == 0 and R.written(hits, counts).tobytes() == want.tobytes()
        with R.Stream(lib, ks, 2, gpu=gpu) as st:
            assert st.rc == 0
            for n, cuts in enumerate(cut_sets):
                got, cnts = R.stream_utterance(st, x, cuts, slot=n & 1)
                assert got.tobytes() == want.tobytes(), cuts
                assert [int(c["frames"]) for c in cnts] == list(cuts) + [x.shape[0]]


def test_every_composition_of_12_frames(lib):
    V, phrases, taus, x = stream_case()
    cut_sets = [c for r in range(12) for c in itertools.combinations(range(1, 12), r)]
    assert len(cut_sets) == 2048
    check_splits(lib, V, phrases, taus, x, cut_sets)


def check_stream_rules(lib, gpu=False):
    V, phrases, taus, x = stream_case()
    want = R.spot(x, phrases, taus)[1]
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks, R.Stream(lib, ks, 3, gpu=gpu) as st:
        # a call without rows reports, moves nothing
        rc, h, c = st.advance([1], [x[:0]], [0], [False])
        assert rc == 0 and (c["n_hits"][0], c["status"][0], c["frames"][0]) == (0, 0, 0)
        # a reset mid-utterance starts over
        rc, h, c = st.advance([0], [x[:7]], [7], [False])
        assert rc == 0
        assert st.reset(0) == 0
        got, _ = R.stream_utterance(st, x, [5], slot=0)
        assert got.tobytes() == want.tobytes()
        # refusals leave the object and the outputs as they were: a slot twice, a slot outside, upto below the frames consumed
        rc, h, c = st.advance([2], [x[:4]], [4], [False])
        assert rc == 0
        fill = bytes([R.FILL])
        for slots, up in (([2, 2], [6, 6]), ([3], [6]), ([-1], [6]), ([2], [3]), ([2], [1501])):
            rc, h, c = st.advance(slots, [x[4:6]] * len(slots), up, [False] * len(slots))
            assert rc == 2 and h.tobytes() == fill * h.nbytes and c.tobytes() == fill * c.nbytes
        assert st.advance([2], [x[4:6]], [6], [False], max_hits=0)[0] == 2
        assert st.reset(3) == 2
        rc, h1, c1 = st.advance([2], [x[4:]], [12], [True])
        assert rc == 0
        # two sessions in one call, one of them final
        rc, h, c = st.advance([1, 0], [x[:12], x[:3]], [12, 3], [True, False])
        assert rc == 0 and R.written(h, c, 0).tobytes() == want.tobytes()
        # the sticky NaN: status 2 and no hits until the slot is reset; the final call resets it by itself
        y = x.copy()
        y[4, 2] = np.nan
        st.reset(0)
        rc, h, c = st.advance([0], [y[:3]], [3], [False])
        assert rc == 0 and c["status"][0] == 0
        rc, h, c = st.advance([0], [y[3:6]], [6], [False])
        assert rc == 0 and (c["status"][0], c["n_hits"][0]) == (2, 0)
        rc, h, c = st.advance([0], [y[6:9]], [9], [False])
        assert rc == 0 and (c["status"][0], c["n_hits"][0]) == (2, 0)
        rc, h, c = st.advance([0], [y[9:]], [12], [True])
        assert rc == 0 and (c["status"][0], c["n_hits"][0]) == (2, 0)
        got, _ = R.stream_utterance(st, x, [6], slot=0)
        assert got.tobytes() == want.tobytes()


def test_stream_rules(lib):
    check_stream_rules(lib)


# ---- the Python layers that need no device ----------------------------------------------------------------------------------------
class _Dict:
    def __init__(self, syms):
        self.syms = ["<s>", "<pad>", "</s>", "<unk>"] + list(syms)

    def __len__(self):
        return len(self.syms)

    def __getitem__(self, i):
        return self.syms[i]

    def index(self, s):
        return self.syms.index(s) if s in self.syms else 3

    def pad(self):
        return 1

    def unk(self):
        return 3


def test_read_keywords_and_handle(tmp_path, lib):
    from streamspeech_amd import keywords as K
    d = _Dict(["▁new", "▁york", "▁city", "s"])
    f = tmp_path / "kw.txt"
    f.write_text("# names\n▁new ▁york\t0.5\n\n▁city s\n", encoding="utf-8")
    phrases, taus = K.read_keywords(str(f), d)
    assert phrases == [[4, 5], [6, 7]] and taus == [0.5, K.DEFAULT_THRESHOLD] and K.DEFAULT_THRESHOLD == 1.0
    assert K.read_keywords(str(f), d, threshold=2.0)[1] == [0.5, 2.0]
    f.write_text("▁new\t-1\n", encoding="utf-8")
    with pytest.raises(ValueError):
        K.read_keywords(str(f), d)
    f.write_text("▁boston\n", encoding="utf-8")
    with pytest.raises(ValueError):
        K.read_keywords(str(f), d)
    f.write_text("▁new ▁york\t0.5\n▁city s\n", encoding="utf-8")
    with K.CtcKeywords.from_file(str(f), d) as kw:
        assert (kw.n_keywords, kw.n_labels, kw.states, kw.workgroups) == (2, 5, 6, 1)
        assert kw.texts == ["▁new ▁york", "▁city s"] and kw.thresholds == [0.5, 1.0]
        x = rows(len(d), [{4: 0}, {5: 0}, {0: 0}])
        hits, counts = kw.spot_host(x, [3])
        assert counts["n_hits"][0] == 1
        assert K.hits_from_records(hits[0, :1]) == [K.CtcHit(0, 0, 1, 0.0, 0.0)]
    with pytest.raises(Exception):
        K.CtcKeywords([[0]], 1.0, len(d), 1, 3)


def test_abi_of_the_new_symbols(lib):
    from streamspeech_amd import lib as L
    assert C.sizeof(L.SSCtcHit) == 24 == R.HIT.itemsize and C.sizeof(L.SSCtcSpotCount) == 16 == R.COUNT.itemsize
    header = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    names = ["ss_ctc_spot_set_create", "ss_ctc_spot_set_info", "ss_ctc_spot_set_destroy", "ss_batch_ctc_spot", "ss_op_ctc_spot",
             "ss_ctc_spot_host", "ss_ctc_spot_stream_create", "ss_ctc_spot_stream_reset", "ss_ctc_spot_stream_destroy",
             "ss_ctc_spot_stream_advance", "ss_ctc_spot_stream_advance_host", "ss_debug_ctc_spot_stream_create",
             "ss_op_ctc_spot_stream_advance", "ss_debug_ctc_spot_trace_host", "ss_debug_ctc_spot_phases"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header) and n in L.SIGNATURES and hasattr(lib, n)
    assert "#define SS_ABI_VERSION 2 " in header and lib.ss_abi_version() == 2
    assert (L.CTC_SPOT_MAX_LABELS, L.CTC_SPOT_MAX_KEYWORDS, L.CTC_SPOT_MAX_HITS) == tuple(
        int(re.search(r"#define SS_CTC_SPOT_MAX_%s (\d+)" % k, header).group(1)) for k in ("LABELS", "KEYWORDS", "HITS"))


def test_agent_keyword_flags():
    """--ctc-keywords is the ASR agent's: the other agents refuse it instead of ignoring it; the threshold needs the file."""
    from argparse import Namespace
    from streamspeech_amd.text_policy import ctc_keyword_flags
    assert ctc_keyword_flags(Namespace()) is None
    assert ctc_keyword_flags(Namespace(ctc_keywords=None, ctc_keyword_threshold=1.0), "S2ST") is None
    assert ctc_keyword_flags(Namespace(ctc_keywords="kw.txt", ctc_keyword_threshold=0.0)) == "kw.txt"
    for agent in ("S2TT", "S2ST"):
        with pytest.raises(ValueError, match="ASR agent"):
            ctc_keyword_flags(Namespace(ctc_keywords="kw.txt", ctc_keyword_threshold=1.0), agent)
    with pytest.raises(ValueError, match="needs --ctc-keywords"):
        ctc_keyword_flags(Namespace(ctc_keywords=None, ctc_keyword_threshold=2.0))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            ctc_keyword_flags(Namespace(ctc_keywords="kw.txt", ctc_keyword_threshold=bad))
