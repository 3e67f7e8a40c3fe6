"""The CTC prefix beam search with an n-gram model, without a device: the library's host twin (ss_ctc_beam_lm_host: the kernels'
step code with the fused order) against tests/ctc_beam_lm_ref.py -- against every labelling of a tiny case by brute force, with
zero weights against the plain twin bit for bit, on the 600 small cases of tests/test_ctc_beam_cpu.py with the reference run on
the twin's own den -- its refusals, and the Python layers over it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import arpa_writer as W
from tests import ctc_align_ref as A
from tests import ctc_beam_lm_ref as RL
from tests import ctc_beam_ref as R
from tests.ngram_ref import Ref
from tests.test_ctc_beam_cpu import PAD, SCALES, SHAPES, UNK, small_case

LM_SEED = 4                   # the order-3 models of the small cases (chosen on the reference alone: see the test's docstring)


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


def small_lm(V, seed=LM_SEED, order=3):
    """-> (arrays, reference scorer) of a model over the labels 4 .. V - 1 and </s> (a hypothesis may hold it)."""
    syms, index = W.int_symbols(V)
    n = 4 * (V - 2)
    a = W.arrays(W.generate(syms, order, [0, n, n, n, n][:order], seed, logp_range=(-0.8, -0.05)), index, V)
    return a, Ref(a)


@pytest.fixture(scope="module")
def lms():
    from streamspeech_amd.ngram import NgramLM
    out = {}
    for V in sorted({s[1] for s in SHAPES}):
        a, ref = small_lm(V)
        out[V] = (NgramLM(a), ref)
    yield out
    for lm, _ in out.values():
        lm.close()


def one(lib, x, V, beam, cand, lm, w, ws, eos=True, nbest=None, pad=PAD, unk=UNK, gpu=False):
    rc, recs = RL.run(lib, [x], V, pad, unk, beam, cand, beam if nbest is None else nbest, lm.h, w, ws, eos, gpu=gpu)
    assert rc == 0
    return recs[0]


# ---- every labelling of a tiny case -------------------------------------------------------------------------------------------------
def test_every_labelling_with_an_lm_against_brute_force(lib):
    """The tiny case of tests/test_ctc_beam_cpu.py (V = 4, T = 5, cand = 3, the twin's cap raised so that nothing is pruned) with an
    order-2 model over its three labels, lm_weight 0.7, word_score 0.3, eos on: all 148 labellings come back, ctc_score within
    1e-9 of the brute-force CTC sum, score within 1e-9 of ctc + 0.7 lm + 0.3 |y| by tests/ngram_ref.py, in the brute-force order
    wherever neighbouring scores differ by more than 1e-9."""
    from streamspeech_amd.lib import CTC_BEAM_MAX_BEAM
    from streamspeech_amd.ngram import NgramLM
    V, T = 4, 5
    x = R.scaled_logits(9, T, V, 2)
    index = {W.BOS: 0, "1": 1, W.EOS: 2, "3": 3}               # the label 2 is the model's </s> as well
    a = W.arrays(W.generate(["1", "3"], 2, [0, 7], 4), index, V, unk=-1)
    ref = Ref(a)
    with NgramLM(a) as lm:
        assert lib.ss_debug_ctc_beam_host_max(256) == CTC_BEAM_MAX_BEAM
        try:
            rec = one(lib, x, V, 256, 3, lm, 0.7, 0.3, pad=-1, unk=-1)
        finally:
            assert lib.ss_debug_ctc_beam_host_max(CTC_BEAM_MAX_BEAM) == 256
    lp = R.frame_values(x, V, -1, -1, rec["den"])
    every = R.labelling_scores(lp)
    assert len(rec["hyps"]) == len(every) == 148 and {h[0] for h in rec["hyps"]} == set(every)
    want = {}
    worst = worst_f = 0.0
    for y, fin, ctc, lms_ in rec["hyps"]:
        tot, _ = A.brute_force(lp, list(y))
        lm_sum = sum(ref.score(y, True)[0])
        want[y] = tot + 0.7 * lm_sum + 0.3 * len(y)
        worst, worst_f = max(worst, abs(ctc - tot)), max(worst_f, abs(fin - want[y]))
        assert abs(lms_ - lm_sum) <= 1e-9
    print(f"ctc_beam_lm exhaustive: max |ctc_score - brute force| = {worst:.3e}, max |score - fused brute force| = {worst_f:.3e}")
    assert worst <= 1e-9 and worst_f <= 1e-9
    order = sorted(want, key=lambda y: -want[y])
    for k, (y, fin, _, _) in enumerate(rec["hyps"]):
        near = [want[order[j]] for j in (k - 1, k + 1) if 0 <= j < len(order)]
        if all(abs(want[order[k]] - v) > 1e-9 for v in near):
            assert y == order[k], k


# ---- zero weights: the plain search ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_zero_weights_are_the_plain_twin_bit_for_bit(lib, lms, shape, scale):
    """lm_weight = 0, word_score = 0, eos off on the 600 small cases: tokens, n_tokens, status and score == ctc_score are the
    bits of ss_ctc_beam_host's records."""
    T, V, beam, cand = shape
    lm, _ = lms[V]
    for seed in range(100):
        x = small_case(shape, scale, seed)
        rec = one(lib, x, V, beam, cand, lm, 0.0, 0.0, eos=False)
        rc, plain = R.run(lib, [x], V, PAD, UNK, beam, cand, beam)
        assert rc == 0
        raw = np.frombuffer(rec["raw"][:32 * beam], RL.LMHYP)
        praw = np.frombuffer(plain[0]["raw"][:16 * beam], R.HYP)
        for k in ("score", "n_tokens", "status"):
            assert raw[k].tobytes() == praw[k].tobytes(), (seed, k)
        assert raw["ctc_score"].tobytes() == praw["score"].tobytes(), seed
        assert rec["raw"][32 * beam:] == plain[0]["raw"][16 * beam:], seed
        assert rec["den"].tobytes() == plain[0]["den"].tobytes() and rec["cand_id"].tobytes() == plain[0]["cand_id"].tobytes()


# ---- many small cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(0.5, 0.0), (1.0, -0.5)])
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_small_cases_with_an_lm_against_the_reference(lib, lms, shape, scale, weights):
    """Seeds 0-99 per shape and scale, an order-3 model, at (lm_weight, word_score) = (0.5, 0) and (1, -0.5), eos on: the twin's
    n-best ids equal the reference's, run on the twin's own den; score, ctc_score and lm_score within 1e-9 * max(1, |.|).  A case
    whose reference margin is below 1e-9 would compare its sorted scores only, and NONE may: LM_SEED was chosen so that the
    reference alone has no such case (the smallest margin is printed).  On the (12, 6, 4, 3) cases at scale 2 with weight 1 the
    best text differs from the plain search's best in at least 5 of 100 seeds -- the reference's count for this LM_SEED is
    printed -- so the fusion is not a no-op."""
    T, V, beam, cand = shape
    lm, ref_lm = lms[V]
    w, ws = weights
    low = differs = 0
    margin = np.inf
    for seed in range(100):
        x = small_case(shape, scale, seed)
        rec = one(lib, x, V, beam, cand, lm, w, ws)
        ref = RL.search(x, V, PAD, UNK, beam, cand, beam, ref_lm, w, ws, True, den=rec["den"])
        assert rec["cand_id"].tolist() == ref["cand_id"], seed
        low += RL.compare(rec, ref, (shape, scale, seed))
        margin = min(margin, ref["margin"])
        if (shape, scale, w) == (SHAPES[0], 2, 1.0):
            plain = R.search(x, V, PAD, UNK, beam, cand, beam, den=rec["den"])
            differs += ref["hyps"][0][0] != plain["hyps"][0][0]
            assert rec["hyps"][0][0] == ref["hyps"][0][0]
        assert all(0 not in h[0] and PAD not in h[0] and UNK not in h[0] for h in rec["hyps"])
    print(f"ctc_beam_lm small {shape} scale {scale} weights {weights}: {low} low-margin cases, smallest margin {margin:.3e}, "
          f"LM best != plain best in {differs}")
    assert low == 0
    if (shape, scale, w) == (SHAPES[0], 2, 1.0):
        assert differs >= 5


# ---- edge cases and refusals ----------------------------------------------------------------------------------------------------------
def check_edges(lib, lm, ref_lm, gpu=False):
    """T = 1, beam = cand = 1, fewer prefixes alive than nbest, no labelling with probability > 0; eos off."""
    V = 64
    x = R.scaled_logits(1, 1, V, 6)
    rec = one(lib, x, V, 4, 3, lm, 0.5, 0.1, gpu=gpu)
    assert not RL.compare(rec, RL.search(x, V, PAD, UNK, 4, 3, 4, ref_lm, 0.5, 0.1, True, den=rec["den"]))
    x = R.scaled_logits(2, 20, V, 6)
    for eos in (True, False):
        rec = one(lib, x, V, 1, 1, lm, 0.5, 0.1, eos=eos, gpu=gpu)
        assert not RL.compare(rec, RL.search(x, V, PAD, UNK, 1, 1, 1, ref_lm, 0.5, 0.1, eos, den=rec["den"])) and len(rec["hyps"]) == 1
    x = np.full((1, V), -np.inf, np.float32)
    x[0, [0, 9]] = [1.0, 2.0]
    rec = one(lib, x, V, 8, 4, lm, 0.5, 0.0, gpu=gpu)
    assert rec["status"] == [0, 0] + [1] * 6 and sorted(h[0] for h in rec["hyps"]) == [(), (9,)]
    x = np.full((3, V), -np.inf, np.float32)
    x[:, PAD] = 0.0
    assert one(lib, x, V, 4, 4, lm, 0.5, 0.0, gpu=gpu)["status"] == [1] * 4


def test_host_edge_cases(lib, lms):
    check_edges(lib, *lms[64])


def check_refusals(lib, lm, gpu=False):
    """The plain refusals, and the model's: a NULL lm or opts, a model of another V, a non-finite weight or score; nothing written."""
    from streamspeech_amd import lib as L
    from streamspeech_amd.ngram import NgramLM
    from tests.test_ctc_beam_cpu import refusals
    for xs, beam, cand, nbest, stride in refusals():
        assert RL.run(lib, xs, 64, PAD, UNK, beam, cand, nbest, lm.h, 0.5, 0.0, gpu=gpu, out_stride=stride)[0] == L.SS_ERR_ARG
    x = [R.scaled_logits(6, 6, 64, 6)]
    assert RL.run(lib, x, 64, PAD, UNK, 4, 4, 4, None, 0.5, 0.0, gpu=gpu)[0] == L.SS_ERR_ARG
    assert RL.run(lib, x, 64, PAD, UNK, 4, 4, 4, lm.h, 0.5, 0.0, gpu=gpu, opts=False)[0] == L.SS_ERR_ARG
    assert RL.run(lib, [x[0][:, :63].copy()], 63, PAD, UNK, 4, 4, 4, lm.h, 0.5, 0.0, gpu=gpu)[0] == L.SS_ERR_ARG
    for w, ws in ((np.nan, 0.0), (np.inf, 0.0), (0.5, np.nan), (0.5, -np.inf)):
        assert RL.run(lib, x, 64, PAD, UNK, 4, 4, 4, lm.h, w, ws, gpu=gpu)[0] == L.SS_ERR_ARG
    a, _ = small_lm(64)
    with NgramLM(dict(a, eos=-1)) as no_eos:                    # the eos term needs an eos id; without the term the model serves
        assert RL.run(lib, x, 64, PAD, UNK, 4, 4, 4, no_eos.h, 0.5, 0.0, True, gpu=gpu)[0] == L.SS_ERR_ARG
        assert RL.run(lib, x, 64, PAD, UNK, 4, 4, 4, no_eos.h, 0.5, 0.0, False, gpu=gpu)[0] == 0
    assert RL.run(lib, x, 64, PAD, UNK, 4, 4, 4, lm.h, 0.5, 0.0, gpu=gpu)[0] == 0


def test_host_refusals(lib, lms):
    check_refusals(lib, lms[64][0])


# ---- the Python layers --------------------------------------------------------------------------------------------------------------
def test_ctc_decoder_beam_search_with_an_lm(lib, lms):
    """CTCDecoder.beam_search(lm=...) on a stand-in engine whose ctc_beam is the host twin: the plain keys plus ctc_score and
    lm_score; without lm the engine sees the plain call and the hypotheses have neither key."""
    from streamspeech_amd.engine import CtcHypothesis
    from streamspeech_amd.generators import CTCDecoder
    x = R.scaled_logits(60, 40, 64, 6)
    lm, _ = lms[64]
    seen = {}

    class Dict:
        def pad(self): return 1
        def eos(self): return 2
        def unk(self): return 3

    class Eng:
        def ctc_beam(self, head, enc, beam, cand=None, nbest=None, **kw):
            seen["kw"] = kw
            if not kw:
                return [CtcHypothesis(list(y), s) for y, s in R.run(lib, [x], 64, 1, 3, beam, cand or 4, nbest)[1][0]["hyps"]]
            rec = one(lib, x, 64, beam, cand or 4, kw["lm"], kw["lm_weight"], kw["word_score"], nbest=nbest)
            return [CtcHypothesis(list(h[0]), *h[1:]) for h in rec["hyps"]]

    dec = CTCDecoder(Dict(), Eng(), 1)
    enc = {"encoder_out": [torch.zeros(40, 1, 4)]}
    hyps = dec.beam_search(enc, 4, nbest=3, lm=lm, lm_weight=0.5, word_score=0.25)[0]
    assert seen["kw"] == {"lm": lm, "lm_weight": 0.5, "word_score": 0.25} and len(hyps) == 3
    for h in hyps:
        assert set(h) == {"tokens", "score", "attn", "alignment", "positional_scores", "ctc_score", "lm_score"}
        assert abs(h["score"] - (h["ctc_score"] + 0.5 * h["lm_score"] + 0.25 * len(h["tokens"]))) <= 1e-9
    assert hyps[0]["score"] >= hyps[1]["score"] >= hyps[2]["score"]
    plain = dec.beam_search(enc, 4, nbest=3)[0]
    assert seen["kw"] == {} and all("ctc_score" not in h and "lm_score" not in h for h in plain)
    assert CtcHypothesis([1], -1.0) == ([1], -1.0, None, None)


def test_offline_lm_flags(capsys):
    from streamspeech_amd import offline
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", "x", "--synthetic", "2"]
    a = offline.build_parser().parse_args(base + ["--ctc-beam", "4", "--ctc-lm-asr", "a.arpa", "--ctc-lm-st", "b.arpa.gz",
                                                  "--ctc-lm-weight", "0.8", "--ctc-word-score", "-0.25"])
    assert (a.ctc_lm_asr, a.ctc_lm_st, a.ctc_lm_weight, a.ctc_word_score) == ("a.arpa", "b.arpa.gz", 0.8, -0.25)
    a = offline.build_parser().parse_args(base)
    assert (a.ctc_lm_asr, a.ctc_lm_st, a.ctc_lm_weight, a.ctc_word_score) == (None, None, 0.5, 0.0)
    for flags in (["--ctc-lm-asr", "a.arpa"], ["--ctc-lm-st", "a.arpa"], ["--ctc-lm-weight", "0.3"], ["--ctc-word-score", "1"]):
        with pytest.raises(SystemExit):
            offline.main(base + flags)
        assert "need --ctc-beam" in capsys.readouterr().err
