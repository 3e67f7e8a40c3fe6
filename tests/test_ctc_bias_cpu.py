"""The hotword set of the CTC prefix beam search, without a device: the library's automaton and its plain-C++ scorer
(ss_ctc_bias_create, ss_ctc_bias_score_host: csrc/ctc_bias.hpp) against tests/ctc_bias_ref.py -- the naive automaton that finds a
state as the longest suffix by search, state and delta exact; the closed form, which knows nothing of states, within 1e-12 --
every refusal of create, the struct sizes, the new symbols, and the Python layer over it (hotwords.read_hotwords, CtcBias)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ctc_bias_ref as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ss_ctc_bias_create", "ss_ctc_bias_info", "ss_ctc_bias_score_host", "ss_op_ctc_bias_score", "ss_batch_ctc_beam_bias",
       "ss_ctc_beam_bias_host", "ss_op_ctc_beam_bias", "ss_ctc_stream_create_bias", "ss_debug_ctc_stream_create_bias"]


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


def score_host(lib, bias, seqs, finish=True):
    """ss_ctc_bias_score_host -> per sequence (deltas, states, sum)."""
    n = [len(s) for s in seqs]
    tok = np.asarray([t for s in seqs for t in s] or [0], np.int32)
    delta = np.full(max(sum(n), 1) + 1, -7.0)
    state = np.full(max(sum(n), 1) + 1, -7, np.int32)
    total = np.full(len(seqs) + 1, -7.0)
    rc = lib.ss_ctc_bias_score_host(bias.h, len(seqs), tok.ctypes.data, (C.c_int32 * len(seqs))(*n), int(finish), delta.ctypes.data,
                                    state.ctypes.data, total.ctypes.data)
    assert rc == 0 and total[-1] == -7.0 and delta[max(sum(n), 1)] == -7.0 and state[max(sum(n), 1)] == -7
    out, o = [], 0
    for b, k in enumerate(n):
        out.append((delta[o:o + k].tolist(), state[o:o + k].tolist(), float(total[b])))
        o += k
    return out


def node_strings(lib, bias, phrases):
    """The library's node id -> its string, from the states a phrase's own tokens lead through."""
    ids = {0: ()}
    for p, (_, st, _) in zip(phrases, score_host(lib, bias, phrases, False)):
        for k, s in enumerate(st):
            assert ids.setdefault(s, tuple(p[:k + 1])) == tuple(p[:k + 1])
    return ids


def test_score_host_is_the_naive_automaton_exactly(lib):
    """Random admissible sets over V = 2 .. 6 (labels 1 .. V - 1, up to 6 phrases of up to 4 tokens, boosts in [-1, 3)), 40 sets
    per V with 20 strings of 0 .. 14 labels each: every delta and every finished and unfinished sum is the naive walk's float64
    value bit for bit, every state is the node of the naive state's string, and the object reports the naive automaton's size."""
    from streamspeech_amd.hotwords import CtcBias
    checked = nested = 0
    for V in range(2, 7):
        labels = list(range(1, V))
        for seed in range(40):
            rng = np.random.default_rng(1000 * V + seed)
            phrases, boosts = RB.random_set(rng, labels, int(rng.integers(1, 7)), 4)
            naive = RB.Naive(phrases, boosts)
            nested += any(tuple(p) == tuple(q[:len(p)]) for p in phrases for q in phrases if p is not q)
            seqs = [[int(rng.choice(labels)) for _ in range(int(rng.integers(0, 15)))] for _ in range(20)]
            with CtcBias(phrases, boosts, V) as bias:
                assert (bias.n_phrases, bias.states) == (len(phrases), len(naive.held))
                assert bias.slots >= 2 * bias.states and bias.slots & (bias.slots - 1) == 0 and (bias.slots == 2 or bias.slots < 4 * bias.states)
                assert bias.device_bytes == 12 * bias.slots + 32 * bias.states
                ids = node_strings(lib, bias, phrases)
                for fin in (True, False):
                    for y, (d, st, total) in zip(seqs, score_host(lib, bias, seqs, fin)):
                        wd, ws, wt = naive.walk(y, fin)
                        assert d == wd and [ids[s] for s in st] == ws and total == wt, (V, seed, y)
                        checked += len(y)
    print(f"ctc_bias naive: {checked} tokens exact, {nested} sets with prefix nesting")
    assert nested >= 20


def test_finished_sums_are_the_closed_form(lib):
    """Sets built to nest and to overlap -- "new" / "new york" shapes, and phrases whose suffix is another's prefix -- and random
    ones: the finished sum of ss_ctc_bias_score_host is within 1e-12 of the sum of held[end(p)] over the occurrences that are not
    a proper prefix of another occurrence at the same place, on strings made of the phrases themselves, cut and glued."""
    from streamspeech_amd.hotwords import CtcBias
    sets = [([[1, 2], [1, 2, 3], [4]], [1.5, 0.75, 2.0]),                      # prefix nesting
            ([[1, 2, 3], [3, 4, 5], [5, 1]], [1.0, 2.5, -0.5]),                # a suffix that is another's prefix
            ([[1, 1, 2], [2, 2, 1], [1, 2, 2, 2, 3]], [0.5, 1.25, 3.0]),       # self-overlap, and a long phrase through both
            ([[2], [2, 3], [2, 3, 4], [2, 3, 4, 5], [1, 1]], [1.0, -1.0, 2.0, 0.25, 1.5])]
    for seed in range(30):
        rng = np.random.default_rng(seed)
        sets.append(RB.random_set(rng, [1, 2, 3, 4, 5], 6, 5))
    worst = 0.0
    for k, (phrases, boosts) in enumerate(sets):
        assert RB.admissible(phrases)
        rng = np.random.default_rng(100 + k)
        seqs = []
        for _ in range(30):
            y = []
            for _ in range(int(rng.integers(1, 6))):
                p = phrases[int(rng.integers(len(phrases)))]
                y += p[:int(rng.integers(1, len(p) + 1))] if rng.random() < 0.4 else p
                if rng.random() < 0.3:
                    y.append(int(rng.integers(1, 6)))
            seqs.append(y)
        with CtcBias(phrases, boosts, 6) as bias:
            for y, (_, _, total) in zip(seqs, score_host(lib, bias, seqs, True)):
                want = RB.closed_form(phrases, boosts, y)
                worst = max(worst, abs(total - want))
                assert abs(total - want) <= 1e-12, (phrases, boosts, y, total, want)
    print(f"ctc_bias closed form: max |sum - closed form| = {worst:.3e} on {len(sets)} sets")


def create(lib, phrases, boosts, V=8, pad=1, unk=3, off=None):
    tok = np.asarray([t for p in phrases for t in p] or [0], np.int32)
    off = np.asarray(off if off is not None else np.cumsum([0] + [len(p) for p in phrases]), np.int32)
    bo = np.asarray(boosts or [0.0], np.float32)
    h = C.c_void_p(0x1234)
    rc = lib.ss_ctc_bias_create(len(phrases), tok.ctypes.data, off.ctypes.data, bo.ctypes.data, V, pad, unk, C.byref(h))
    return rc, h


def test_create_refusals_allocate_nothing(lib):
    from streamspeech_amd import lib as L
    ok = [[4, 5], [4, 5, 6], [7]]
    bad = {"an empty phrase": ([[4, 5], []], [1.0, 1.0]),
           "an id >= V": ([[4, 8]], [1.0]),
           "a negative id": ([[4, -1]], [1.0]),
           "blank": ([[4, 0, 5]], [1.0]),
           "pad": ([[4, 1]], [1.0]),
           "unk": ([[3]], [1.0]),
           "a duplicate": ([[4, 5], [6], [4, 5]], [1.0, 1.0, 2.0]),
           "a NaN boost": (ok, [1.0, np.nan, 1.0]),
           "an infinite boost": (ok, [1.0, 1.0, -np.inf]),
           "33 tokens": ([[4 + k % 2 for k in range(33)]], [1.0]),
           "a phrase inside another": ([[4, 5, 6], [5]], [1.0, 1.0]),
           "a phrase at the end of another": ([[4, 5, 6], [5, 6]], [1.0, 1.0]),
           "a phrase inside a longer one, given first": ([[6, 7], [4, 6, 7, 5]], [1.0, 1.0])}
    for what, (phrases, boosts) in bad.items():
        rc, h = create(lib, phrases, boosts)
        assert rc == L.SS_ERR_ARG and h.value is None, what
    many = [[4 + (k // 4 ** j) % 4 for j in range(7)] + [2] for k in range(4097)]   # distinct, one length, each ends in its only 2
    assert create(lib, many, [1.0] * 4097)[0] == L.SS_ERR_ARG
    rc, h = create(lib, many[:4096], [1.0] * 4096)
    assert rc == 0 and h.value
    lib.ss_ctc_bias_destroy(h)
    for kw in ({"V": 0}, {"pad": 8}, {"unk": -2}, {"off": [0, 2, 1, 6]}, {"off": [1, 2, 5, 6]}):
        rc, h = create(lib, ok, [1.0] * 3, **kw)
        assert rc == L.SS_ERR_ARG and h.value is None, kw
    assert lib.ss_ctc_bias_create(1, None, None, None, 8, 1, 3, C.byref(h)) == L.SS_ERR_ARG and h.value is None
    assert lib.ss_ctc_bias_create(-1, None, None, None, 8, 1, 3, C.byref(h)) == L.SS_ERR_ARG
    assert lib.ss_ctc_bias_create(0, None, None, None, 8, 1, 3, None) == L.SS_ERR_ARG
    rc, h = create(lib, ok, [1.0, 2.0, 3.0])                     # "new" / "new york" is legal
    assert rc == 0 and h.value
    assert lib.ss_ctc_bias_score_host(None, 1, None, (C.c_int32 * 1)(0), 1, None, None, (C.c_double * 1)()) == L.SS_ERR_ARG
    assert lib.ss_ctc_bias_score_host(h, 0, None, (C.c_int32 * 1)(0), 1, None, None, (C.c_double * 1)()) == L.SS_ERR_ARG
    assert lib.ss_ctc_bias_score_host(h, 1, None, (C.c_int32 * 1)(-1), 1, None, None, (C.c_double * 1)()) == L.SS_ERR_ARG
    assert lib.ss_ctc_bias_score_host(h, 1, None, (C.c_int32 * 1)(2), 1, None, None, (C.c_double * 1)()) == L.SS_ERR_ARG
    total = (C.c_double * 1)(5.0)
    assert lib.ss_ctc_bias_score_host(h, 1, None, (C.c_int32 * 1)(0), 1, None, None, total) == 0 and total[0] == 0.0
    assert lib.ss_ctc_bias_info(None, None, None, None, None) == L.SS_ERR_ARG
    lib.ss_ctc_bias_destroy(h)
    lib.ss_ctc_bias_destroy(None)
    rc, h = create(lib, [], [])                                  # an empty set is a set: the root alone
    assert rc == 0 and h.value
    lib.ss_ctc_bias_destroy(h)


def test_struct_sizes_symbols_and_prototypes(lib):
    from streamspeech_amd import lib as L
    assert C.sizeof(L.SSCtcBiasOpts) == 16 and C.sizeof(L.SSCtcBeamBiasHyp) == 40 == RB.BHYP.itemsize
    assert (L.CTC_BIAS_MAX_LEN, L.CTC_BIAS_MAX_PHRASES) == (32, 4096)
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    assert "#define SS_CTC_BIAS_MAX_LEN 32" in header and "#define SS_CTC_BIAS_MAX_PHRASES 4096" in header
    assert "#define SS_ABI_VERSION 2" in header and lib.ss_abi_version() == 2
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} has no prototype in the header"
        assert name in L.SIGNATURES
    assert hasattr(lib, "ss_ctc_bias_destroy") and re.search(r"\bvoid\s+ss_ctc_bias_destroy\s*\(", header)


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
class Dict:
    """Stand-in for the head's dictionary: ids 0 .. 3 are <s> <pad> </s> <unk>, then the pieces."""

    def __init__(self, pieces):
        self.symbols = ["<s>", "<pad>", "</s>", "<unk>"] + list(pieces)

    def index(self, s):
        return self.symbols.index(s) if s in self.symbols else 3

    def unk(self):
        return 3

    def pad(self):
        return 1

    def __len__(self):
        return len(self.symbols)


def test_read_hotwords_format_and_errors(tmp_path):
    from streamspeech_amd.hotwords import CtcBias, read_hotwords
    d = Dict(["▁new", "▁york", "▁ac", "me"])
    p = tmp_path / "hot.txt"
    p.write_text("# names\n▁new ▁york\t2.5\n\n▁new\n   \n▁ac me\t-0.5\n  # indented comment\n", encoding="utf-8")
    phrases, boosts = read_hotwords(str(p), d)
    assert phrases == [[4, 5], [4], [6, 7]] and boosts == [2.5, 1.5, -0.5]
    assert read_hotwords(str(p), d, boost=3.0)[1] == [2.5, 3.0, -0.5]
    with CtcBias(phrases, boosts, len(d), d.pad(), d.unk()) as bias:
        assert (bias.n_phrases, bias.states, bias.V, bias.pad, bias.unk) == (3, 5, 8, 1, 3)
    with CtcBias(phrases, 2.0, len(d)) as bias:                  # one boost for all
        assert bias.n_phrases == 3
    for text, line, what in (("▁new\n▁old ▁york\n", 2, "▁old"), ("▁new\tx\n", 1, "boost"), ("▁new\tnan\n", 1, "finite"),
                             ("▁new\n\n\t2.0\n", 3, "phrase"), ("<unk>\n", 1, "<unk>")):
        p.write_text(text, encoding="utf-8")
        with pytest.raises(ValueError) as e:
            read_hotwords(str(p), d)
        assert f":{line}:" in str(e.value) and what in str(e.value), (text, str(e.value))
    from streamspeech_amd.lib import StreamSpeechHipError
    with pytest.raises(StreamSpeechHipError):
        CtcBias([[4, 5], [5]], [1.0, 1.0], len(d), 1, 3)
    with pytest.raises(ValueError):
        CtcBias([[4, 5]], [1.0, 2.0], len(d))
