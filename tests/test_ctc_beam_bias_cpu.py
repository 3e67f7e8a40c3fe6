"""The CTC prefix beam search with a hotword set, without a device: the library's host twin (ss_ctc_beam_bias_host: the kernels'
step code with the bias term in the order, with an n-gram model or without) against tests/ctc_bias_ref.py -- against every
labelling of a tiny case by brute force and the closed form of the bias, with scale 0 against the plain and the LM twin bit for
bit, on the 600 small cases of tests/test_ctc_beam_cpu.py with the reference run on the twin's own den -- the finish term, a
negative boost, a phrase whose completion is extended, the refusals, and the Python layers over it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import arpa_writer as W
from tests import ctc_align_ref as A
from tests import ctc_beam_lm_ref as RL
from tests import ctc_beam_ref as R
from tests import ctc_bias_ref as RB
from tests.ngram_ref import Ref
from tests.test_ctc_beam_cpu import PAD, SCALES, SHAPES, UNK, small_case
from tests.test_ctc_beam_lm_cpu import small_lm

BIAS_SEED = 3                 # the phrase sets of the small cases (chosen on the reference alone: see the test's docstring)
BIAS_SCALES = (1.0, 0.4)
LM_W = (0.5, 0.0)             # (lm_weight, word_score) of the LM + bias cases


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


def small_set(V, seed=BIAS_SEED):
    """-> (phrases, boosts) over the labels of a small case (not blank, pad or unk): 4 phrases of up to 3 labels for V = 6, 24 of
    up to 4 for V = 64 (every third extends an earlier one by one or two labels), boosts in [-1, 3)."""
    labels = [c for c in range(1, V) if c not in (PAD, UNK)]
    rng = np.random.default_rng(7919 * seed + V)
    return RB.random_set(rng, labels, 4 if V <= 8 else 24, 3 if V <= 8 else 4)


@pytest.fixture(scope="module")
def sets():
    from streamspeech_amd.hotwords import CtcBias
    out = {}
    for V in sorted({s[1] for s in SHAPES}):
        phrases, boosts = small_set(V)
        out[V] = (CtcBias(phrases, boosts, V, PAD, UNK), RB.Naive(phrases, boosts))
    yield out
    for b, _ in out.values():
        b.close()


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


def one(lib, x, V, beam, cand, bias, scale, finish=True, lm=None, w=0.0, ws=0.0, eos=True, nbest=None, pad=PAD, unk=UNK, gpu=False):
    rc, recs = RB.run(lib, [x], V, pad, unk, beam, cand, beam if nbest is None else nbest, bias.h, scale, finish,
                      lm.h if lm is not None else None, w, ws, eos, gpu=gpu)
    assert rc == 0
    return recs[0]


# ---- every labelling of a tiny case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lm", [False, True])
def test_every_labelling_with_hotwords_against_brute_force(lib, with_lm):
    """The tiny case of tests/test_ctc_beam_cpu.py (V = 4, T = 5, cand = 3, the twin's cap raised so that nothing is pruned) with
    the phrases (1, 3) and (2, 2, 1) over its labels, scale 0.8 -- and the same with the order-2 model of the LM test at weight
    0.7, word_score 0.3, eos on: all 148 labellings come back, ctc_score within 1e-9 of the brute-force CTC sum, bias_score within
    1e-9 of the closed form, score within 1e-9 of ctc + 0.8 bias (+ 0.7 lm + 0.3 |y|), in the brute-force order wherever
    neighbouring scores differ by more than 1e-9."""
    from streamspeech_amd.hotwords import CtcBias
    from streamspeech_amd.lib import CTC_BEAM_MAX_BEAM
    from streamspeech_amd.ngram import NgramLM
    V, T = 4, 5
    x = R.scaled_logits(9, T, V, 2)
    phrases, boosts = [[1, 3], [2, 2, 1]], [1.25, 0.75]
    index = {W.BOS: 0, "1": 1, W.EOS: 2, "3": 3}               # the label 2 is the model's </s> as well
    a = W.arrays(W.generate(["1", "3"], 2, [0, 7], 4), index, V, unk=-1)
    ref_lm = Ref(a)
    with CtcBias(phrases, boosts, V) as bias, NgramLM(a) as lm:
        assert lib.ss_debug_ctc_beam_host_max(256) == CTC_BEAM_MAX_BEAM
        try:
            rec = one(lib, x, V, 256, 3, bias, 0.8, True, lm if with_lm else None, 0.7, 0.3, pad=-1, unk=-1)
        finally:
            assert lib.ss_debug_ctc_beam_host_max(CTC_BEAM_MAX_BEAM) == 256
    lp = R.frame_values(x, V, -1, -1, rec["den"])
    every = R.labelling_scores(lp)
    assert len(rec["hyps"]) == len(every) == 148 and {h[0] for h in rec["hyps"]} == set(every)
    want = {}
    worst = worst_b = worst_f = 0.0
    biased = 0
    for y, fin, ctc, lms_, bs in rec["hyps"]:
        tot, _ = A.brute_force(lp, list(y))
        b = RB.closed_form(phrases, boosts, y)
        biased += b != 0
        lm_sum = sum(ref_lm.score(y, True)[0]) if with_lm else 0.0
        want[y] = tot + 0.8 * b + (0.7 * lm_sum + 0.3 * len(y) if with_lm else 0.0)
        worst, worst_b, worst_f = max(worst, abs(ctc - tot)), max(worst_b, abs(bs - b)), max(worst_f, abs(fin - want[y]))
        assert abs(lms_ - lm_sum) <= 1e-9
    print(f"ctc_beam_bias exhaustive (lm {with_lm}): max |ctc_score - brute force| = {worst:.3e}, max |bias_score - closed form| = "
          f"{worst_b:.3e}, max |score - fused brute force| = {worst_f:.3e}; {biased} labellings hold a phrase")
    assert worst <= 1e-9 and worst_b <= 1e-9 and worst_f <= 1e-9 and biased >= 10
    order = sorted(want, key=lambda y: -want[y])
    for k, (y, fin, _, _, _) in enumerate(rec["hyps"]):
        near = [want[order[j]] for j in (k - 1, k + 1) if 0 <= j < len(order)]
        if all(abs(want[order[k]] - v) > 1e-9 for v in near):
            assert y == order[k], k


# ---- scale 0: the plain search, the LM search -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_scale_zero_is_the_plain_and_the_lm_twin_bit_for_bit(lib, sets, lms, shape, scale):
    """Bias scale 0 on the 600 small cases.  Without a model: tokens, n_tokens, status and score == ctc_score are the bits of
    ss_ctc_beam_host's records.  With the order-3 model at (0.5, 0), eos on: score, ctc_score, lm_score, n_tokens, status and the
    tokens are the bits of ss_ctc_beam_lm_host's records."""
    T, V, beam, cand = shape
    bias, _ = sets[V]
    lm, _ = lms[V]
    for seed in range(100):
        x = small_case(shape, scale, seed)
        rec = one(lib, x, V, beam, cand, bias, 0.0, True)
        rc, plain = R.run(lib, [x], V, PAD, UNK, beam, cand, beam)
        assert rc == 0
        raw = np.frombuffer(rec["raw"][:40 * beam], RB.BHYP)
        praw = np.frombuffer(plain[0]["raw"][:16 * beam], R.HYP)
        for k in ("score", "n_tokens", "status"):
            assert raw[k].tobytes() == praw[k].tobytes(), (seed, k)
        assert raw["ctc_score"].tobytes() == praw["score"].tobytes() and not raw["lm_score"].any(), seed
        assert rec["raw"][40 * beam:] == plain[0]["raw"][16 * beam:], seed
        assert rec["den"].tobytes() == plain[0]["den"].tobytes() and rec["cand_id"].tobytes() == plain[0]["cand_id"].tobytes()
        rec = one(lib, x, V, beam, cand, bias, 0.0, True, lm, *LM_W)
        rc, with_lm = RL.run(lib, [x], V, PAD, UNK, beam, cand, beam, lm.h, *LM_W)
        assert rc == 0
        raw = np.frombuffer(rec["raw"][:40 * beam], RB.BHYP)
        lraw = np.frombuffer(with_lm[0]["raw"][:32 * beam], RL.LMHYP)
        for k in ("score", "ctc_score", "lm_score", "n_tokens", "status"):
            assert raw[k].tobytes() == lraw[k].tobytes(), (seed, k)
        assert rec["raw"][40 * beam:] == with_lm[0]["raw"][32 * beam:], seed


# ---- many small cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_lm", [False, True])
@pytest.mark.parametrize("bscale", BIAS_SCALES)
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_small_cases_with_hotwords_against_the_reference(lib, sets, lms, shape, scale, bscale, with_lm):
    """Seeds 0-99 per shape and logit scale, at the bias scales 1 and 0.4, bias alone and with the order-3 model at (0.5, 0) and
    eos on, finish on: the twin's n-best ids equal the reference's, run on the twin's own den; score, ctc_score, lm_score and
    bias_score within 1e-9 * max(1, |.|).  A case whose reference margin is below 1e-9 would compare its sorted scores only, and
    NONE may: BIAS_SEED was chosen so that the reference alone has no such case (the smallest margin is printed).  On the
    (12, 6, 4, 3) cases at logit scale 2, bias alone at scale 1, the reference's best text differs from the plain reference's best
    in at least 5 of 100 seeds, and the twin's count equals the reference's -- so the bias is not a no-op."""
    T, V, beam, cand = shape
    bias, naive = sets[V]
    lm, ref_lm = lms[V] if with_lm else (None, None)
    w, ws = LM_W if with_lm else (0.0, 0.0)
    counted = (shape, scale, bscale, with_lm) == (SHAPES[0], 2, 1.0, False)
    low = differs = differs_twin = 0
    margin = np.inf
    for seed in range(100):
        x = small_case(shape, scale, seed)
        rec = one(lib, x, V, beam, cand, bias, bscale, True, lm, w, ws)
        ref = RB.search(x, V, PAD, UNK, beam, cand, beam, naive, bscale, True, ref_lm, w, ws, True, den=rec["den"])
        assert rec["cand_id"].tolist() == ref["cand_id"], seed
        low += RB.compare(rec, ref, (shape, scale, bscale, with_lm, seed))
        margin = min(margin, ref["margin"])
        if counted:
            plain = R.search(x, V, PAD, UNK, beam, cand, beam, den=rec["den"])
            differs += ref["hyps"][0][0] != plain["hyps"][0][0]
            differs_twin += rec["hyps"][0][0] != plain["hyps"][0][0]
        assert all(0 not in h[0] and PAD not in h[0] and UNK not in h[0] for h in rec["hyps"])
    print(f"ctc_beam_bias small {shape} scale {scale} bias scale {bscale} lm {with_lm}: {low} low-margin cases, smallest margin "
          f"{margin:.3e}, biased best != plain best in {differs} (twin {differs_twin})")
    assert low == 0 and margin >= 1e-9
    if counted:
        assert differs >= 5 and differs_twin == differs


# ---- the finish term, a negative boost, a completion that is extended ------------------------------------------------------------------
def forced(V, path, hi=12.0):
    """Logits whose frame t all but forces path[t] (0 = blank)."""
    x = np.zeros((len(path), V), np.float32)
    for t, c in enumerate(path):
        x[t, c] = hi
    return x


def test_finish_on_and_off(lib, sets):
    """Finish off: score = ctc + scale * bias_sum with the open credit still in it; finish on: the same strings lose
    scale * open(state).  On forced logits that end inside a phrase the two differ by exactly that; on the small cases both agree
    with the reference run with the same flag, and a string that ends at the root scores the same either way."""
    from streamspeech_amd.hotwords import CtcBias
    V = 8
    x = forced(V, [4, 0, 5, 5, 0])                             # "4 5", the first two tokens of the phrase 4 5 6
    with CtcBias([[4, 5, 6], [7]], [2.0, 1.0], V, PAD, UNK) as bias:
        on = one(lib, x, V, 4, 3, bias, 0.5, True)
        off = one(lib, x, V, 4, 3, bias, 0.5, False)
    assert on["hyps"][0][0] == off["hyps"][0][0] == (4, 5)
    assert off["hyps"][0][4] == 4.0 and on["hyps"][0][4] == 0.0                  # bias_score: lent 2 + 2, nothing kept
    assert off["hyps"][0][1] == off["hyps"][0][2] + 0.5 * 4.0 and on["hyps"][0][1] == off["hyps"][0][1] - 0.5 * 4.0
    assert abs(on["hyps"][0][1] - on["hyps"][0][2]) <= 1e-12
    assert on["hyps"][0][2] == off["hyps"][0][2]
    bias, naive = sets[6]
    for seed in range(20):
        xs = small_case(SHAPES[0], 2, seed)
        for fin in (True, False):
            rec = one(lib, xs, 6, 4, 3, bias, 1.0, fin)
            assert not RB.compare(rec, RB.search(xs, 6, PAD, UNK, 4, 3, 4, naive, 1.0, fin, den=rec["den"]), (seed, fin))
            for y, score, ctc, _, bs in rec["hyps"]:
                assert bs == naive.walk(y, fin)[2]


def test_a_negative_boost_pushes_a_phrase_down(lib):
    """Frames that slightly prefer 4 5 to 4 6: with the phrase 4 5 at boost -3 the search returns 4 6 first, 4 5 behind it with
    bias_score -6; the plain order has them the other way round."""
    from streamspeech_amd.hotwords import CtcBias
    V = 8
    x = forced(V, [4, 0, 5])
    x[2, 6] = 11.0
    rc, plain = R.run(lib, [x], V, PAD, UNK, 4, 3, 4)
    assert rc == 0 and [h[0] for h in plain[0]["hyps"][:2]] == [(4, 5), (4, 6)]
    with CtcBias([[4, 5]], [-3.0], V, PAD, UNK) as bias:
        rec = one(lib, x, V, 4, 3, bias, 1.0, True)
    assert rec["hyps"][0][0] == (4, 6) and rec["hyps"][0][4] == 0.0
    down = [h for h in rec["hyps"] if h[0] == (4, 5)][0]
    assert down[4] == -6.0 and down[1] == down[2] - 6.0


def test_a_completed_phrase_that_is_extended(lib):
    """"new" / "new york": phrases (4) at 1.5 and (4, 5) at 1.0.  The string 4 keeps 1.5; 4 5 holds held(4 5) = 1.5 + 1.0 = 2.5
    (the node 4 carries the larger boost of the two phrases through it); 4 6 keeps the 1.5 of the completed "new" although the
    longer match broke; 4 4 earns it twice."""
    from streamspeech_amd.hotwords import CtcBias
    V = 8
    with CtcBias([[4], [4, 5]], [1.5, 1.0], V, PAD, UNK) as bias:
        for path, y, want in (([4, 0, 0], (4,), 1.5), ([4, 5, 0], (4, 5), 2.5), ([4, 6, 0], (4, 6), 1.5), ([4, 0, 4], (4, 4), 3.0),
                              ([4, 5, 4], (4, 5, 4), 4.0), ([6, 5, 0], (6, 5), 0.0)):
            rec = one(lib, forced(V, path), V, 4, 3, bias, 2.0, True)
            assert rec["hyps"][0][0] == y and rec["hyps"][0][4] == want, (path, rec["hyps"][0])
            assert rec["hyps"][0][1] == rec["hyps"][0][2] + 2.0 * want
            assert want == RB.closed_form([[4], [4, 5]], [1.5, 1.0], y)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, bias, lm, gpu=False):
    """The plain refusals and the model's, and the set's: a NULL bias or bias opts, a set of another V, pad or unk, a non-finite
    scale, a model without options or options without a model; nothing written."""
    from streamspeech_amd import lib as L
    from streamspeech_amd.hotwords import CtcBias
    from tests.test_ctc_beam_cpu import refusals
    for xs, beam, cand, nbest, stride in refusals():
        assert RB.run(lib, xs, 64, PAD, UNK, beam, cand, nbest, bias.h, 1.0, gpu=gpu, out_stride=stride)[0] == L.SS_ERR_ARG
    x = [R.scaled_logits(6, 6, 64, 6)]
    assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, None, 1.0, gpu=gpu)[0] == L.SS_ERR_ARG
    assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, bias.h, 1.0, gpu=gpu, bias_opts=False)[0] == L.SS_ERR_ARG
    assert RB.run(lib, [x[0][:, :63].copy()], 63, PAD, UNK, 4, 4, 4, bias.h, 1.0, gpu=gpu)[0] == L.SS_ERR_ARG
    assert RB.run(lib, x, 64, 5, UNK, 4, 4, 4, bias.h, 1.0, gpu=gpu)[0] == L.SS_ERR_ARG
    assert RB.run(lib, x, 64, PAD, -1, 4, 4, 4, bias.h, 1.0, gpu=gpu)[0] == L.SS_ERR_ARG
    for s in (np.nan, np.inf, -np.inf):
        assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, bias.h, s, gpu=gpu)[0] == L.SS_ERR_ARG
    assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, bias.h, 1.0, lm=lm.h, lm_weight=0.5, gpu=gpu, lm_opts=False)[0] == L.SS_ERR_ARG
    assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, bias.h, 1.0, lm=None, gpu=gpu, lm_opts=True)[0] == L.SS_ERR_ARG
    assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, bias.h, 1.0, lm=lm.h, lm_weight=np.nan, gpu=gpu)[0] == L.SS_ERR_ARG
    with CtcBias([[4, 5]], [1.0], 64) as other:                  # made without pad / unk: not this head's
        assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, other.h, 1.0, gpu=gpu)[0] == L.SS_ERR_ARG
        assert RB.run(lib, x, 64, -1, -1, 4, 4, 4, other.h, 1.0, gpu=gpu)[0] == 0
    assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, bias.h, 1.0, gpu=gpu)[0] == 0
    assert RB.run(lib, x, 64, PAD, UNK, 4, 4, 4, bias.h, 1.0, lm=lm.h, lm_weight=0.5, gpu=gpu)[0] == 0


def test_host_refusals_write_nothing(lib, sets, lms):
    check_refusals(lib, sets[64][0], lms[64][0])


def check_edges(lib, bias, naive, gpu=False):
    """T = 1, beam = cand = 1, fewer prefixes alive than nbest, no labelling with probability > 0, the optional outputs left out."""
    V = 64
    x = R.scaled_logits(1, 1, V, 6)
    rec = one(lib, x, V, 4, 3, bias, 1.0, gpu=gpu)
    assert not RB.compare(rec, RB.search(x, V, PAD, UNK, 4, 3, 4, naive, 1.0, den=rec["den"]))
    x = R.scaled_logits(2, 20, V, 6)
    for fin in (True, False):
        rec = one(lib, x, V, 1, 1, bias, 1.0, fin, gpu=gpu)
        assert not RB.compare(rec, RB.search(x, V, PAD, UNK, 1, 1, 1, naive, 1.0, fin, den=rec["den"])) and len(rec["hyps"]) == 1
    rc, recs = RB.run(lib, [x], V, PAD, UNK, 4, 4, 4, bias.h, 1.0, gpu=gpu, want_den=False)
    assert rc == 0 and recs[0]["raw"] == one(lib, x, V, 4, 4, bias, 1.0, gpu=gpu)["raw"]
    x = np.full((1, V), -np.inf, np.float32)
    x[0, [0, 9]] = [1.0, 2.0]
    rec = one(lib, x, V, 8, 4, bias, 1.0, gpu=gpu)
    assert rec["status"] == [0, 0] + [1] * 6 and sorted(h[0] for h in rec["hyps"]) == [(), (9,)]
    x = np.full((3, V), -np.inf, np.float32)
    x[:, PAD] = 0.0
    assert one(lib, x, V, 4, 4, bias, 1.0, gpu=gpu)["status"] == [1] * 4


def test_host_edge_cases(lib, sets):
    check_edges(lib, *sets[64])


# ---- the Python layers --------------------------------------------------------------------------------------------------------------
def test_ctc_decoder_beam_search_with_hotwords(lib, sets, lms):
    """CTCDecoder.beam_search(bias=...) on a stand-in engine whose ctc_beam is the host twin: the plain keys plus ctc_score and
    bias_score (and lm_score with lm); without bias the engine sees what it saw before."""
    from streamspeech_amd.engine import CtcBiasHypothesis, CtcHypothesis
    from streamspeech_amd.generators import CTCDecoder
    x = R.scaled_logits(60, 40, 64, 6)
    bias, lm = sets[64][0], lms[64][0]
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
            rec = one(lib, x, 64, beam, cand or 4, kw["bias"], kw["bias_scale"], True, kw.get("lm"), kw.get("lm_weight", 0.0),
                      kw.get("word_score", 0.0), nbest=nbest)
            return [CtcBiasHypothesis(list(h[0]), h[1], h[2], h[3] if "lm" in kw else None, h[4]) for h in rec["hyps"]]

    dec = CTCDecoder(Dict(), Eng(), 1)
    enc = {"encoder_out": [torch.zeros(40, 1, 4)]}
    hyps = dec.beam_search(enc, 4, nbest=3, bias=bias, bias_scale=0.75)[0]
    assert seen["kw"] == {"bias": bias, "bias_scale": 0.75} and len(hyps) == 3
    for h in hyps:
        assert set(h) == {"tokens", "score", "attn", "alignment", "positional_scores", "ctc_score", "bias_score"}
        assert abs(h["score"] - (h["ctc_score"] + 0.75 * h["bias_score"])) <= 1e-9
    hyps = dec.beam_search(enc, 4, nbest=3, lm=lm, lm_weight=0.5, word_score=0.25, bias=bias, bias_scale=0.75)[0]
    assert seen["kw"] == {"lm": lm, "lm_weight": 0.5, "word_score": 0.25, "bias": bias, "bias_scale": 0.75}
    for h in hyps:
        assert set(h) == {"tokens", "score", "attn", "alignment", "positional_scores", "ctc_score", "lm_score", "bias_score"}
        assert abs(h["score"] - (h["ctc_score"] + 0.5 * h["lm_score"] + 0.25 * len(h["tokens"]) + 0.75 * h["bias_score"])) <= 1e-9
    assert hyps[0]["score"] >= hyps[1]["score"] >= hyps[2]["score"]
    plain = dec.beam_search(enc, 4, nbest=3)[0]
    assert seen["kw"] == {} and all("ctc_score" not in h and "bias_score" not in h for h in plain)
    assert CtcHypothesis([1], -1.0).bias_score is None and CtcBiasHypothesis([1], -1.0, -2.0, None, 1.0).bias_score == 1.0


def test_offline_hotword_flags(capsys):
    from streamspeech_amd import offline
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", "x", "--synthetic", "2"]
    a = offline.build_parser().parse_args(base + ["--ctc-beam", "4", "--ctc-hotwords-asr", "a.txt", "--ctc-hotwords-st", "b.txt",
                                                  "--ctc-hotword-boost", "2.5"])
    assert (a.ctc_hotwords_asr, a.ctc_hotwords_st, a.ctc_hotword_boost) == ("a.txt", "b.txt", 2.5)
    a = offline.build_parser().parse_args(base)
    assert (a.ctc_hotwords_asr, a.ctc_hotwords_st, a.ctc_hotword_boost) == (None, None, 1.5)
    for flags in (["--ctc-hotwords-asr", "a.txt"], ["--ctc-hotwords-st", "a.txt"], ["--ctc-hotword-boost", "0.3"]):
        with pytest.raises(SystemExit):
            offline.main(base + flags)
        assert "need --ctc-beam" in capsys.readouterr().err


def test_agent_hotword_flags_and_options():
    """--ctc-hotwords / --ctc-hotword-boost parse on every streaming agent (default off); they need --ctc-beam, which is the ASR
    agent's alone: ValueError at construction, before anything is loaded.  CtcBeamOptions hands the set to engine.CtcStream only
    when there is one."""
    import argparse
    from streamspeech_amd import text_policy as P
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    req = ["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0"]

    def parse(cls, *extra):
        p = argparse.ArgumentParser()
        cls.add_args(p)
        return p.parse_args(req + list(extra))

    a = parse(StreamSpeechASRAgent)
    assert (a.ctc_hotwords, a.ctc_hotword_boost) == (None, 1.5) and P.ctc_beam_flags(a) is None
    a = parse(StreamSpeechASRAgent, "--ctc-beam", "4", "--ctc-hotwords", "h.txt", "--ctc-hotword-boost", "2")
    o = P.ctc_beam_flags(a)
    assert (o.beam, o.bias, o.bias_scale) == (4, None, 1.0) and (a.ctc_hotwords, a.ctc_hotword_boost) == ("h.txt", 2.0)
    for cls in (StreamSpeechS2STAgent, StreamSpeechS2TTAgent, StreamSpeechASRAgent):
        for extra in (("--ctc-hotwords", "h.txt"), ("--ctc-hotword-boost", "2")):
            with pytest.raises(ValueError, match="ctc-beam"):
                cls(parse(cls, *extra))
    for cls in (StreamSpeechS2STAgent, StreamSpeechS2TTAgent):
        with pytest.raises(ValueError, match="ctc-beam"):
            cls(parse(cls, "--ctc-beam", "4", "--ctc-hotwords", "h.txt"))
    for extra in (("--ctc-beam", "4", "--ctc-hotword-boost", "2"), ("--ctc-beam", "4", "--ctc-hotwords", "h.txt", "--ctc-hotword-boost", "nan")):
        with pytest.raises(ValueError, match="hotword"):
            StreamSpeechASRAgent(parse(StreamSpeechASRAgent, *extra))
    bias = object()
    assert P.CtcBeamOptions(8).stream_kwargs() == dict(beam=8, cand=None, nbest=None)
    assert P.CtcBeamOptions(4, bias=bias, bias_scale=0.5).stream_kwargs() == dict(beam=4, cand=None, nbest=None, bias=bias, bias_scale=0.5)
    with pytest.raises(ValueError):
        P.CtcBeamOptions(4, bias=bias, bias_scale=float("inf"))
