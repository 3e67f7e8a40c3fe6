"""CTC prefix beam search without a device: the library's host twin (ss_ctc_beam_host: the kernels' step code, record layout and
refusals) against tests/ctc_beam_ref.py -- against every labelling of a tiny case by brute force, on 600 seeded small cases with the
reference run on the twin's own den, against a mutant of the reference without the persistent child lookup, and on the edge cases
tests/test_ctc_beam_gpu.py repeats on the kernels -- and the Python layers over it."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as A
from tests import ctc_beam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, UNK = 1, 3
SHAPES = [(12, 6, 4, 3), (12, 6, 2, 5), (40, 64, 8, 8)]      # (T, V, beam, cand)
SCALES = (2, 6)
MUTANT_CASE = ((12, 6, 4, 3), 2, 78)                         # the small case the mutant fails on: (shape, logit scale, seed)


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


def one(lib, x, V, beam, cand, nbest=None, pad=PAD, unk=UNK, gpu=False):
    rc, recs = R.run(lib, [x], V, pad, unk, beam, cand, beam if nbest is None else nbest, gpu=gpu)
    assert rc == 0
    return recs[0]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_beam_entry_points_are_declared_and_bound(lib):
    from streamspeech_amd import lib as L
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in (("ss_batch_ctc_beam", 12), ("ss_ctc_beam_host", 15), ("ss_op_ctc_beam", 16), ("ss_debug_ctc_beam_host_max", 1)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"
    assert lib.ss_abi_version() == 2
    assert C.sizeof(L.SSCtcBeamHyp) == R.HYP.itemsize == 16
    assert [f[0] for f in L.SSCtcBeamHyp._fields_] == list(R.HYP.names)
    for name in ("BEAM", "CAND", "FRAMES"):
        assert "#define SS_CTC_BEAM_MAX_%s %d" % (name, getattr(L, "CTC_BEAM_MAX_" + name)) in header


# ---- every labelling of a tiny case -------------------------------------------------------------------------------------------------
def test_every_labelling_against_brute_force(lib):
    """V = 4, T = 5, cand = 3 = V - 1, no pad / unk: 148 labellings.  The twin's beam cap is raised for this call alone (the hook
    ss_debug_ctc_beam_host_max), so nothing is pruned and every labelling's score is the exact CTC probability: each equals the
    enumeration of all 4^5 paths (tests/ctc_align_ref.py:brute_force) within 1e-9, on the twin's own per-frame values."""
    from streamspeech_amd.lib import CTC_BEAM_MAX_BEAM
    V, T = 4, 5
    x = R.scaled_logits(9, T, V, 2)
    assert lib.ss_debug_ctc_beam_host_max(256) == CTC_BEAM_MAX_BEAM
    try:
        rec = one(lib, x, V, 256, 3, pad=-1, unk=-1)
    finally:
        assert lib.ss_debug_ctc_beam_host_max(CTC_BEAM_MAX_BEAM) == 256
    assert R.run(lib, [x], V, -1, -1, 33, 3, 33)[0] != 0        # the cap is back
    lp = R.frame_values(x, V, -1, -1, rec["den"])
    every = R.labelling_scores(lp)
    got = dict(rec["hyps"])
    assert len(rec["hyps"]) == len(got) == len(every) and set(got) == set(every)
    scores = [s for _, s in rec["hyps"]]
    assert scores == sorted(scores, reverse=True)
    worst = 0.0
    for y, s in got.items():
        tot, _ = A.brute_force(lp, list(y))
        worst = max(worst, abs(s - tot))
    print(f"ctc_beam exhaustive: {len(got)} labellings, max |score - brute force| = {worst:.3e}")
    assert worst <= 1e-9
    assert abs(np.logaddexp.reduce(scores)) <= T * A.TOL        # and they sum to 1, as far as T float32 log-softmax rows do


def test_top_32_of_every_labelling_at_the_cap(lib):
    """The same with the cap in place, T = 4: 61 labellings, at most 25 before the last frame, so nothing is pruned before it and
    the 32 that come back are the 32 most likely, each exact."""
    V, T = 4, 4
    x = R.scaled_logits(10, T, V, 2)
    rec = one(lib, x, V, 32, 3, pad=-1, unk=-1)
    every = sorted(R.labelling_scores(R.frame_values(x, V, -1, -1, rec["den"])).items(), key=lambda v: -v[1])
    assert len(every) == 61 and len(rec["hyps"]) == 32 and every[31][1] - every[32][1] > 1e-9
    assert {y for y, _ in rec["hyps"]} == {y for y, _ in every[:32]}
    for y, s in rec["hyps"]:
        assert abs(s - dict(every)[y]) <= 1e-9


# ---- many small cases ---------------------------------------------------------------------------------------------------------------
def small_case(shape, scale, seed):
    T, V, beam, cand = shape
    return R.scaled_logits(seed, T, V, scale)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_small_cases_against_the_reference_on_its_own_den(lib, shape, scale):
    """Seeds 0-99 per shape and scale: the twin's n-best ids equal the reference's, run on the twin's own den; scores within
    1e-9 * max(1, |score|).  A case whose reference margin is below 1e-9 would compare its sorted scores only, and at most 2 % may:
    on the twin's values NONE of the 600 does -- the smallest margin is 1.9e-6.  In the (12, 6, 4, 3) cases at scale 2 the best
    labelling differs from the collapsed arg-max in 43 of 100 (>= 5 required): the search is not the arg-max in disguise."""
    T, V, beam, cand = shape
    low = differs = 0
    margin = np.inf
    for seed in range(100):
        x = small_case(shape, scale, seed)
        rec = one(lib, x, V, beam, cand)
        ref = R.search(x, V, PAD, UNK, beam, cand, beam, den=rec["den"])
        assert rec["cand_id"].tolist() == ref["cand_id"], seed
        low += R.compare(rec, ref, (shape, scale, seed))
        margin = min(margin, ref["margin"])
        differs += rec["hyps"][0][0] != R.collapsed_argmax(R.frame_values(x, V, PAD, UNK))
        assert all(0 not in y and PAD not in y and UNK not in y for y, _ in rec["hyps"])
    print(f"ctc_beam small {shape} scale {scale}: {low} low-margin cases, smallest margin {margin:.3e}, best != arg-max in {differs}")
    assert low <= 2
    if (shape, scale) == (SHAPES[0], 2):
        assert differs >= 5


def test_mutant_without_the_persistent_child_lookup_fails():
    """The reference with node identity "slot at frame t" (a string that left the beam and comes back is a new node): on the
    (12, 6, 4, 3) cases at scale 2 its n-best must differ from the true reference's on at least one seed -- it does on seed 78
    (a string splits into two nodes that each hold a part of its probability)."""
    shape, scale, _ = MUTANT_CASE
    T, V, beam, cand = shape
    failed = []
    for seed in range(100):
        x = small_case(shape, scale, seed)
        ref = R.search(x, V, PAD, UNK, beam, cand, beam)
        mut = R.search(x, V, PAD, UNK, beam, cand, beam, slot_identity=True)
        try:
            R.compare(mut, ref)
        except AssertionError:
            failed.append(seed)
    assert MUTANT_CASE[2] in failed, failed


def test_host_passes_where_the_mutant_fails(lib):
    shape, scale, seed = MUTANT_CASE
    T, V, beam, cand = shape
    x = small_case(shape, scale, seed)
    rec = one(lib, x, V, beam, cand)
    mut = R.search(x, V, PAD, UNK, beam, cand, beam, den=rec["den"], slot_identity=True)
    with pytest.raises(AssertionError):
        R.compare(rec, mut)
    labels = [y for y, _ in rec["hyps"]]
    assert len(set(labels)) == len(labels)
    assert not R.compare(rec, R.search(x, V, PAD, UNK, beam, cand, beam, den=rec["den"]))


# ---- the per-frame values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ld", [(64, 64), (257, 260), (6000, 6000)])
def test_host_den_and_candidates(lib, V, ld):
    """den within the suite's TOL of the float64 log-sum-exp; cand_id the reference's choice exactly, with a row of tied logits and a
    row with fewer than `cand` finite columns; columns past V (1e9) are never read."""
    x = A.logits(V, 9, V, ld)
    x[2, 1:V] = np.float32(0.5)                                   # every column ties: ids ascend from the first unmasked one
    x[3, 5:9] = x[3].max() if ld == V else x[3, :V].max()         # a tie at the top
    x[4, :V] = -np.inf
    x[4, [0, 7, PAD, UNK, 20]] = [1.0, 0.5, 9.0, 9.0, 0.5]        # two finite candidates, pad and unk above them
    cand = 8
    rec = one(lib, x, V, 4, cand)
    x64 = x[:, :V].astype(np.float64)
    m = x64.max(axis=1)
    lse = m + np.log(np.exp(x64 - m[:, None]).sum(axis=1))
    err = np.abs((rec["den"][:, 0].astype(np.float64) + rec["den"][:, 1]) - lse).max()
    print(f"ctc_beam den V={V}: max |max + logsum - f64 logsumexp| = {err:.3e}")
    assert err <= A.TOL
    want = [R.candidates(x[t], V, PAD, UNK, cand) for t in range(x.shape[0])]
    assert rec["cand_id"].tolist() == want
    assert want[2] == [2, 4, 5, 6, 7, 8, 9, 10] and want[4] == [7, 20] + [-1] * 6 and want[3][:4] == [5, 6, 7, 8]


@pytest.mark.parametrize("shape", SHAPES)
def test_host_scores_against_float64_and_the_aligner(lib, shape):
    """Against the reference on the float64 log-softmax: |score - ref| <= T * 2e-5 + 1e-9 * max(1, |ref|) (T per-frame values, each
    within the suite's TOL), label for label where the reference's margin is above twice that, by sorted scores otherwise.  And no
    hypothesis scores above the aligner's log p(labels | audio) + T * 2e-5: the search sums a subset of the alignments."""
    T, V, beam, cand = shape
    for seed in range(10):
        x = small_case(shape, 6, seed)
        rec = one(lib, x, V, beam, cand)
        ref = R.search(x, V, PAD, UNK, beam, cand, beam)
        bound = lambda s: T * A.TOL + 1e-9 * max(1.0, abs(s))  # noqa: E731
        if ref["margin"] > 2 * T * A.TOL:
            assert [y for y, _ in rec["hyps"]] == [y for y, _ in ref["hyps"]]
            assert all(abs(a - b) <= bound(b) for (_, a), (_, b) in zip(rec["hyps"], ref["hyps"]))
        else:
            assert all(abs(a - b) <= bound(b) for a, b in zip(sorted(s for _, s in rec["hyps"]), sorted(s for _, s in ref["hyps"])))
        rc, al = A.run(lib, [(x, list(y)) for y, _ in rec["hyps"]], V, pad=PAD)
        assert rc == 0
        for (y, s), a in zip(rec["hyps"], al):
            assert a["status"] == 0 and s <= a["score"] + T * A.TOL, (seed, y, s, a["score"])


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------
def test_host_edge_cases(lib):
    V = 64
    # T = 1: the empty string and the candidates, by their lp
    x = R.scaled_logits(1, 1, V, 6)
    rec = one(lib, x, V, 4, 3)
    ref = R.search(x, V, PAD, UNK, 4, 3, 4, den=rec["den"])
    assert not R.compare(rec, ref) and sorted(len(y) for y, _ in rec["hyps"]) == [0, 1, 1, 1]
    # beam = cand = 1
    x = R.scaled_logits(2, 20, V, 6)
    rec = one(lib, x, V, 1, 1)
    assert not R.compare(rec, R.search(x, V, PAD, UNK, 1, 1, 1, den=rec["den"])) and len(rec["hyps"]) == 1
    # nbest larger than the prefixes alive: at T = 1 with one finite candidate two prefixes live
    x = np.full((1, V), -np.inf, np.float32)
    x[0, [0, 9]] = [1.0, 2.0]
    rec = one(lib, x, V, 8, 4)
    assert rec["status"] == [0, 0] + [1] * 6 and [y for y, _ in rec["hyps"]] == [(9,), ()]
    # no labelling has probability > 0: only pad is finite
    x = np.full((3, V), -np.inf, np.float32)
    x[:, PAD] = 0.0
    assert one(lib, x, V, 4, 4)["status"] == [1] * 4
    # pad / unk hold the largest logit in every row: never in a hypothesis, nor a candidate; columns past V hold 1e9
    x = R.scaled_logits(3, 30, V, 6, ld=70)
    x[:, [PAD, UNK]] = 50.0
    rec = one(lib, x, V, 8, 8)
    assert not (np.isin(rec["cand_id"], [0, PAD, UNK])).any() and rec["cand_id"].max() < V
    assert all(PAD not in y and UNK not in y for y, _ in rec["hyps"]) and rec["status"] == [0] * 8
    assert not R.compare(rec, R.search(x, V, PAD, UNK, 8, 8, 8, den=rec["den"]))
    assert all(s < -30 for _, s in rec["hyps"])                   # the masked mass is in the denominator: log_softmax first


def ragged_pack(V=64):
    """Eight utterances, a NaN one and a T = 1 one in the middle."""
    xs = [R.scaled_logits(70 + k, T, V, 6) for k, T in enumerate((23, 40, 7, 31, 1, 40, 12, 55))]
    xs[3][17, 40] = np.nan
    return xs


def check_pack(lib, gpu=False):
    V, beam, cand, nbest = 64, 8, 8, 5
    xs = ragged_pack(V)
    rc, recs = R.run(lib, xs, V, PAD, UNK, beam, cand, nbest, gpu=gpu)
    assert rc == 0
    rc, rev = R.run(lib, xs[::-1], V, PAD, UNK, beam, cand, nbest, gpu=gpu)
    assert rc == 0
    for k, x in enumerate(xs):
        alone = R.run(lib, [x], V, PAD, UNK, beam, cand, nbest, gpu=gpu)[1][0]
        assert alone["raw"] == recs[k]["raw"] == rev[len(xs) - 1 - k]["raw"], k
        assert alone["den"].tobytes() == recs[k]["den"].tobytes() and alone["cand_id"].tobytes() == recs[k]["cand_id"].tobytes()
        ref = R.search(x, V, PAD, UNK, beam, cand, nbest, den=recs[k]["den"])
        if k == 3:
            assert recs[k]["status"] == [2] * nbest and ref["status"] == 2 and np.isnan(recs[k]["den"][17]).all()
        else:
            R.compare(recs[k], ref, k)
            assert recs[k]["status"][0] == 0


def test_host_ragged_pack_nan_utterance_and_invariance(lib):
    check_pack(lib)


def test_host_without_the_optional_outputs(lib):
    x = R.scaled_logits(5, 12, 64, 6)
    full = one(lib, x, 64, 4, 4)
    rc, recs = R.run(lib, [x], 64, PAD, UNK, 4, 4, 4, want_den=False)
    assert rc == 0 and recs[0]["raw"] == full["raw"]


def refusals(V=64):
    """[(logits list, beam, cand, nbest, out_stride)] every one of which is SS_ERR_ARG with nothing written."""
    from streamspeech_amd.lib import CTC_BEAM_MAX_BEAM, CTC_BEAM_MAX_CAND, CTC_BEAM_MAX_FRAMES
    x = R.scaled_logits(6, 6, V, 6)
    long_x = np.zeros((CTC_BEAM_MAX_FRAMES + 1, V), np.float32)
    return [([x], 0, 4, 1, None), ([x], CTC_BEAM_MAX_BEAM + 1, 4, 1, None), ([x], 4, 0, 1, None), ([x], 4, CTC_BEAM_MAX_CAND + 1, 1, None),
            ([x], 4, 4, 0, None), ([x], 4, 4, 5, None), ([x, x[:3]], 4, 4, 2, 5), ([long_x], 4, 4, 2, None), ([], 4, 4, 2, None)]


def check_refusals(lib, gpu=False):
    from streamspeech_amd import lib as L
    for xs, beam, cand, nbest, stride in refusals():
        assert R.run(lib, xs, 64, PAD, UNK, beam, cand, nbest, gpu=gpu, out_stride=stride)[0] == L.SS_ERR_ARG, (beam, cand, nbest, stride)


def test_host_refusals(lib):
    from streamspeech_amd import lib as L
    check_refusals(lib)
    x = R.scaled_logits(7, 4, 64, 6)
    hyp, tok = np.zeros(4, R.HYP), np.zeros(16, np.int32)
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    T = (C.c_int32 * 1)(4)
    assert lib.ss_ctc_beam_host(None, 64, 64, PAD, UNK, 1, T, 2, 2, 2, P(hyp), P(tok), 4, None, None) == L.SS_ERR_ARG
    assert lib.ss_ctc_beam_host(P(x), 63, 64, PAD, UNK, 1, T, 2, 2, 2, P(hyp), P(tok), 4, None, None) == L.SS_ERR_ARG
    assert lib.ss_ctc_beam_host(P(x), 64, 64, PAD, UNK, 1, None, 2, 2, 2, P(hyp), P(tok), 4, None, None) == L.SS_ERR_ARG
    assert lib.ss_ctc_beam_host(P(x), 64, 64, PAD, UNK, 1, T, 2, 2, 2, None, P(tok), 4, None, None) == L.SS_ERR_ARG
    assert lib.ss_ctc_beam_host(P(x), 64, 64, PAD, UNK, 1, T, 2, 2, 2, P(hyp), None, 4, None, None) == L.SS_ERR_ARG
    assert not hyp["status"].any() and not tok.any()
    assert lib.ss_ctc_beam_host(P(x), 64, 64, PAD, UNK, 1, T, 2, 2, 2, P(hyp), P(tok), 4, None, None) == 0
    assert hyp["status"].tolist() == [0, 0, 0, 0] and hyp["n_tokens"][0] >= 0 and hyp["score"][0] >= hyp["score"][1]


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def test_default_cand():
    from streamspeech_amd.engine import ctc_beam_default_cand
    assert [ctc_beam_default_cand(b) for b in (1, 4, 8, 31, 32)] == [2, 5, 9, 32, 32]


def test_ctc_decoder_beam_search_feeds_align(lib):
    """CTCDecoder.beam_search on a stand-in engine whose ctc_beam is the host twin: fairseq-shaped hypotheses, each ready for
    CTCDecoder.align."""
    from streamspeech_amd.engine import CtcHypothesis
    from streamspeech_amd.generators import CTCDecoder
    x = R.scaled_logits(60, 40, 8, 6)
    seen = {}

    class Dict:
        def pad(self): return 1
        def eos(self): return 2
        def unk(self): return 3

    class Eng:
        def ctc_beam(self, head, enc, beam, cand=None, nbest=None):
            seen["call"] = (head, tuple(enc.shape), beam, cand, nbest)
            return [CtcHypothesis(list(y), s) for y, s in one(lib, x, 8, beam, cand or 4, nbest)["hyps"]]

    dec = CTCDecoder(Dict(), Eng(), 1)
    hyps = dec.beam_search({"encoder_out": [torch.zeros(40, 1, 4)]}, 4, nbest=3)[0]
    assert seen["call"] == (1, (40, 4), 4, None, 3) and len(hyps) == 3
    assert all(h["tokens"].dtype == torch.long and isinstance(h["score"], float) for h in hyps)
    assert hyps[0]["score"] >= hyps[1]["score"] >= hyps[2]["score"] > -math.inf
    rc, al = A.run(lib, [(x, h["tokens"].tolist()) for h in hyps], 8, pad=PAD)
    assert rc == 0 and all(a["status"] == 0 and h["score"] <= a["score"] + 40 * A.TOL for a, h in zip(al, hyps))


def test_offline_nbest_flags_parse():
    from streamspeech_amd import offline
    args = offline.build_parser().parse_args(["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", "x", "--synthetic",
                                             "2", "--ctc-beam", "4", "--ctc-nbest", "2"])
    assert (args.ctc_beam, args.ctc_beam_cand, args.ctc_nbest) == (4, None, 2)
    assert offline.build_parser().parse_args(["--path", "a", "--vocoder", "b", "--results-path", "x"]).ctc_beam == 0
