"""The back-off n-gram model without a device: the ABI of the new entry points, the library's host scorer (ss_ngram_score_host: the
table builder, the suffix links and the lookup that the kernels share) against tests/ngram_ref.py -- exactly equal float64 values
and equal states -- every refusal of ss_ngram_lm_create, and streamspeech_amd.ngram.read_arpa."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

from tests import arpa_writer as W
from tests.ngram_ref import Ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 24


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


def model(order, counts, seed, V=V, **kw):
    """-> (arrays, removed suffixes) of a generated model over the symbols 4 .. V - 1."""
    syms, index = W.int_symbols(V)
    drop = kw.get("drop_suffix", False)
    grams = W.generate(syms, order, counts, seed, **kw)
    grams, removed = grams if drop else (grams, [])
    return W.arrays(grams, index, V), [tuple(index[s] for s in g) for g in removed]


def sequences(order, V=V, seed=0):
    """Lengths 0, 1, order - 1, order and 40 (twice), tokens over every id 2 .. V - 1 (</s> and <unk> in a history too)."""
    rng = np.random.default_rng(1000 + seed)
    return [rng.integers(2, V, n).tolist() for n in (0, 1, max(order - 1, 0), order, 40, 40)]


def host_score(lib, lm, seqs, eos):
    n = [len(s) for s in seqs]
    tot = sum(n) + (len(seqs) if eos else 0)
    tok = np.asarray([t for s in seqs for t in s] or [0], np.int32)
    lp = np.full(tot + 3, -7.0, np.float64)
    st = np.full(tot + 3, -7, np.int32)
    rc = lib.ss_ngram_score_host(lm.h, len(seqs), tok.ctypes.data, (C.c_int32 * len(seqs))(*n), int(eos), lp.ctypes.data, st.ctypes.data)
    assert rc == 0 and (lp[tot:] == -7.0).all() and (st[tot:] == -7).all()
    return lp[:tot], st[:tot]


def check_against_ref(score, a, seqs):
    """score(seqs, eos) -> (lp, state) packed; exactly the reference's float64 values, and its states."""
    ref = Ref(a)
    for eos in (True, False):
        lp, st = score(seqs, eos)
        want = [ref.score(s, eos) for s in seqs]
        wl = [v for w in want for v in w[0]]
        ws = [ref.entry[g] for w in want for g in w[1]]
        assert lp.tolist() == wl, (a["order"], eos)
        assert st.tolist() == ws, (a["order"], eos)


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
NEW = (("ss_ngram_lm_create", 11), ("ss_ngram_lm_destroy", 1), ("ss_ngram_lm_info", 5), ("ss_ngram_score_host", 7),
       ("ss_op_ngram_score", 8), ("ss_ctc_beam_lm_host", 17), ("ss_op_ctc_beam_lm", 18), ("ss_batch_ctc_beam_lm", 14))


def test_lm_entry_points_are_declared_and_bound(lib):
    from streamspeech_amd import lib as L
    from tests.ctc_beam_lm_ref import LMHYP
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in NEW:
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"
    assert lib.ss_abi_version() == 2
    assert C.sizeof(L.SSCtcBeamLmHyp) == LMHYP.itemsize == 32
    assert [f[0] for f in L.SSCtcBeamLmHyp._fields_] == list(LMHYP.names) == ["score", "ctc_score", "lm_score", "n_tokens", "status"]
    assert [f[0] for f in L.SSCtcLmOpts._fields_] == ["lm_weight", "word_score", "eos_term"]
    assert "#define SS_NGRAM_MAX_ORDER %d" % L.NGRAM_MAX_ORDER in header and L.NGRAM_MAX_ORDER == 6


# ---- the scorer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3, 5])
@pytest.mark.parametrize("unk", [False, True])
def test_host_scores_equal_the_arpa_definition(lib, order, unk):
    """Orders 1, 2, 3, 5; lengths 0, 1, order - 1, order, 40; the symbols 4 and 5 without a unigram (so they score as <unk>, or as
    oov_logp), sparse higher orders (most contexts back off, many twice or more)."""
    from streamspeech_amd.ngram import NgramLM
    a, _ = model(order, [0, 60, 80, 60, 40][:order], 11 + order, unk=unk, skip_unigrams=("4", "5"))
    with NgramLM(a) as lm:
        assert (lm.order, lm.entries) == (order, 1 + sum(a["counts"])) and lm.slots >= 2 * lm.entries and lm.slots & (lm.slots - 1) == 0
        assert lm.device_bytes == 12 * lm.slots + 16 * lm.entries
        check_against_ref(lambda s, e: host_score(lib, lm, s, e), a, sequences(order) + [[4, 5, 4, 9, 5]])


def test_a_context_reachable_only_after_two_back_offs(lib):
    """Hand-made, order 3: in the state (7, 8) the token 9 is found neither after (7, 8) nor after (8): two back-off weights, then
    the unigram.  The value is bo(7 8) + bo(8) + p(9), summed in that order."""
    from streamspeech_amd.ngram import NgramLM
    f = lambda x: float(np.float32(x))  # noqa: E731
    a = {"order": 3, "counts": [5, 2, 1], "tokens": np.asarray([0, 2, 7, 8, 9, 7, 8, 8, 7, 7, 8, 7], np.int32),
         "logp": np.asarray([-9, -1.5, -2.25, -1.125, -3.0625, -0.7, -0.9, -0.3], np.float32),
         "backoff": np.asarray([-0.1, 0, -0.2, -0.4, -0.8, -0.55, -0.35, 0], np.float32), "V": 12, "bos": 0, "eos": 2, "unk": 3, "oov_logp": -20.0}
    with NgramLM(a) as lm:
        lp, st = host_score(lib, lm, [[7, 8, 9]], False)
        assert lp[2] == (0.0 + f(-0.55)) + f(-0.4) + f(-3.0625) and lp[1] == f(-0.7) and st.tolist() == [3, 6, 5]
        check_against_ref(lambda s, e: host_score(lib, lm, s, e), a, [[7, 8, 9], [7, 8, 7, 8, 9], [9, 9], []])


def test_a_dropped_suffix_and_small_tables(lib):
    """An LM with n-grams whose proper suffix is missing (the links skip it); a one-entry LM (the root alone: everything is
    oov_logp); entry counts of exactly a power of two, and one more."""
    from streamspeech_amd.ngram import NgramLM
    a, removed = model(3, [0, 150, 200], 5, drop_suffix=True)
    assert len(removed) >= 3
    ref = Ref(a)
    assert all(g not in ref.logp for g in removed) and any(len(g) == 2 for g in removed)
    with NgramLM(a) as lm:
        seqs = sequences(3) + [list(g[::-1]) + list(g) for g in ref.logp if len(g) == 3][:40]
        check_against_ref(lambda s, e: host_score(lib, lm, s, e), a, seqs)
    empty = {"order": 1, "counts": [0], "tokens": np.zeros(0, np.int32), "logp": np.zeros(0, np.float32), "backoff": np.zeros(0, np.float32),
             "V": V, "bos": 0, "eos": 2, "unk": 3, "oov_logp": -3.5}
    with NgramLM(empty) as lm:
        assert (lm.entries, lm.slots) == (1, 2)
        lp, st = host_score(lib, lm, [[5, 6, 7]], True)
        assert lp.tolist() == [-3.5] * 4 and st.tolist() == [0] * 4
    for extra in (0, 1):                                       # 64 entries (the root + 63), then 65
        a, _ = model(2, [0, 63 - (V - 2) + extra], 9)
        assert 1 + sum(a["counts"]) == 64 + extra
        with NgramLM(a) as lm:
            assert lm.slots == (128 if extra == 0 else 256)
            check_against_ref(lambda s, e: host_score(lib, lm, s, e), a, sequences(2))


def test_create_refusals(lib):
    from streamspeech_amd import lib as L
    from streamspeech_amd.ngram import NgramLM
    good, _ = model(3, [0, 30, 30], 3)

    def refused(**change):
        a = dict(good, **change)
        with pytest.raises(L.StreamSpeechHipError) as e:
            NgramLM(a)
        assert e.value.code == L.SS_ERR_ARG, change
    NgramLM(good).close()
    n1 = good["counts"][0]
    tok, lp, bo = good["tokens"].copy(), good["logp"].copy(), good["backoff"].copy()
    refused(order=0)
    refused(order=7, counts=good["counts"] + [0] * 4)
    for bad in (-1, V):                                        # an id outside [0, V)
        t = tok.copy()
        t[n1 + 1] = bad
        refused(tokens=t)
    refused(bos=V), refused(eos=-2), refused(unk=V)
    t = tok.copy()
    t[n1 + 2:n1 + 4] = t[n1:n1 + 2]                            # the second bigram repeats the first
    refused(tokens=t)
    t = tok.copy()
    t[n1] = 1                                                  # a bigram whose context (<pad>) is not a unigram
    refused(tokens=t)
    for arr, name in ((lp, "logp"), (bo, "backoff")):
        for v in (np.nan, np.inf, -np.inf):
            x = arr.copy()
            x[5] = v
            refused(**{name: x})
    refused(oov_logp=float("nan")), refused(oov_logp=float("-inf"))
    # more than 2^30 entries: refused by the counts alone, before anything is read or allocated
    h = C.c_void_p(1)
    counts = (C.c_int64 * 1)(1 << 30)
    assert lib.ss_ngram_lm_create(1, counts, tok.ctypes.data, lp.ctypes.data, bo.ctypes.data, V, 0, 2, 3, -1.0, C.byref(h)) == L.SS_ERR_ARG
    assert h.value is None
    assert lib.ss_ngram_lm_create(1, counts, tok.ctypes.data, lp.ctypes.data, bo.ctypes.data, V, 0, 2, 3, -1.0, None) == L.SS_ERR_ARG
    # the scorer's own refusals
    with NgramLM(dict(good, eos=-1)) as lm:
        out = np.zeros(4)
        n = (C.c_int32 * 1)(1)
        assert lib.ss_ngram_score_host(lm.h, 1, tok.ctypes.data, n, 1, out.ctypes.data, None) == L.SS_ERR_ARG
        assert lib.ss_ngram_score_host(None, 1, tok.ctypes.data, n, 0, out.ctypes.data, None) == L.SS_ERR_ARG
        assert lib.ss_ngram_score_host(lm.h, 0, tok.ctypes.data, n, 0, out.ctypes.data, None) == L.SS_ERR_ARG
        assert lib.ss_ngram_score_host(lm.h, 1, tok.ctypes.data, (C.c_int32 * 1)(-1), 0, out.ctypes.data, None) == L.SS_ERR_ARG
        assert not out.any()
        assert lib.ss_ngram_score_host(lm.h, 1, tok.ctypes.data, n, 0, out.ctypes.data, None) == 0 and out[0] != 0


# ---- read_arpa ----------------------------------------------------------------------------------------------------------------------
def test_read_arpa_plain_gzipped_dropped_and_missing(tmp_path):
    from streamspeech_amd.modules import Dictionary
    from streamspeech_amd.ngram import read_arpa
    d = Dictionary.placeholder(14)                             # ▁w0 .. ▁w9
    syms = [d[i] for i in range(4, 14)]
    grams = W.generate(syms, 3, [0, 25, 25], 21, unk=True)
    want = W.arrays(grams, d.index, len(d))
    plain, gz = tmp_path / "lm.arpa", tmp_path / "lm.arpa.gz"
    plain.write_text(W.text(grams), encoding="utf-8")
    with gzip.open(gz, "wt", encoding="utf-8") as f:
        f.write(W.text(grams))
    for path in (plain, gz):
        a = read_arpa(str(path), d)
        assert (a["order"], a["counts"], a["V"], a["bos"], a["eos"], a["unk"], a["dropped"]) == (3, want["counts"], 14, 0, 2, 3, 0)
        for k in ("tokens", "logp", "backoff"):
            assert a[k].dtype == want[k].dtype and a[k].tobytes() == want[k].tobytes(), k
    assert a["logp"][1] == np.float32(np.float64(f"{grams[1][1][1]:.4f}") * np.log(10)) and a["backoff"][-1] == 0
    # a dictionary without ▁w9 and ▁w8: their n-grams are dropped and counted
    small = Dictionary.placeholder(12)
    lost = sum(any(s in ("▁w8", "▁w9") for s in g[0]) for k in grams for g in grams[k])
    a = read_arpa(str(plain), small)
    assert a["dropped"] == lost > 2 and sum(a["counts"]) == sum(want["counts"]) - lost and a["tokens"].max() < 12
    # neither every unigram nor <unk>: an error that names the first missing symbol, unless oov_logp is given
    grams = W.generate(syms, 2, [0, 10], 22, skip_unigrams=("▁w3", "▁w7"))
    plain.write_text(W.text(grams), encoding="utf-8")
    with pytest.raises(ValueError, match="▁w3"):
        read_arpa(str(plain), d)
    assert read_arpa(str(plain), d, oov_logp=-12.5)["oov_logp"] == -12.5
    grams = W.generate(syms, 2, [0, 10], 22, skip_unigrams=("▁w3", "▁w7"), unk=True)
    plain.write_text(W.text(grams), encoding="utf-8")
    assert read_arpa(str(plain), d)["counts"][0] == 11
