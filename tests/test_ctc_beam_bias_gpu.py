"""The CTC prefix beam search with a hotword set on the GPU (csrc/ctc_beam.hip: the bias forms of the search kernel) through
ss_op_ctc_beam_bias against the host twin that tests/test_ctc_beam_bias_cpu.py pins to the Python reference and to brute force.
Both run the same frame code on the same float64 state; what differs is the row's log-sum (another expf), so the twin is run on
the device's own logits and compared on what the den leaves alone: the n-best label strings, status and n_tokens are equal, the
scores within 1e-9 * max(1, |.|) of the reference run on the kernel's own den, and bias_score -- a function of the labels alone --
bit for bit.  Then the caps, a ragged pack, a NaN row, the refusals, ss_batch_ctc_beam_bias on the seeded synthetic checkpoint
and the offline driver's n-best files."""
import numpy as np
import pytest
import torch

from tests import ctc_beam_ref as R
from tests import ctc_bias_ref as RB
from tests.test_ctc_beam_bias_cpu import BIAS_SCALES, LM_W, check_edges, check_refusals, one, small_set
from tests.test_ctc_beam_cpu import PAD, SCALES, SHAPES, UNK, small_case
from tests.test_ctc_beam_lm_cpu import small_lm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


@pytest.fixture(scope="module")
def objs(lib):
    """Per V of the small shapes: (hotword set, its naive automaton, model, its reference scorer)."""
    from streamspeech_amd.hotwords import CtcBias
    from streamspeech_amd.ngram import NgramLM
    out = {}
    for V in sorted({s[1] for s in SHAPES}):
        phrases, boosts = small_set(V)
        a, ref = small_lm(V)
        out[V] = (CtcBias(phrases, boosts, V, PAD, UNK), RB.Naive(phrases, boosts), NgramLM(a), ref)
    yield out
    for b, _, lm, _ in out.values():
        b.close()
        lm.close()


def against_twin_and_reference(lib, objs, x, V, beam, cand, bscale, with_lm, name, finish=True):
    bias, naive, lm, ref_lm = objs[V]
    lm, ref_lm = (lm, ref_lm) if with_lm else (None, None)
    w, ws = LM_W if with_lm else (0.0, 0.0)
    rec = one(lib, x, V, beam, cand, bias, bscale, finish, lm, w, ws, gpu=True)
    host = one(lib, x, V, beam, cand, bias, bscale, finish, lm, w, ws)
    ref = RB.search(x, V, PAD, UNK, beam, cand, beam, naive, bscale, finish, ref_lm, w, ws, True, den=rec["den"])
    assert rec["cand_id"].tolist() == ref["cand_id"] == host["cand_id"].tolist(), name
    low = RB.compare(rec, ref, name)
    same_den = rec["den"].tobytes() == host["den"].tobytes()
    if same_den:                                               # the same per-frame values: the same frame code, the same bytes
        assert rec["raw"] == host["raw"], name
    if not low:
        assert [h[0] for h in rec["hyps"]] == [h[0] for h in host["hyps"]] and rec["status"] == host["status"], name
        assert [h[4] for h in rec["hyps"]] == [h[4] for h in host["hyps"]], name       # bias_score: the labels' alone
    return rec, low, same_den


def test_op_small_shapes_against_the_host_twin(lib, objs):
    """Twenty seeds of each (T, V, beam, cand) of the CPU test at logit scale 2 and 6 alternating, both bias scales, bias alone and
    with the model; none may fall back to sorted scores."""
    n = same = 0
    for shape in SHAPES:
        for seed in range(20):
            for bscale in BIAS_SCALES:
                for with_lm in (False, True):
                    _, low, same_den = against_twin_and_reference(lib, objs, small_case(shape, SCALES[seed & 1], seed), shape[1], shape[2],
                                                                  shape[3], bscale, with_lm, (shape, seed, bscale, with_lm))
                    assert not low
                    n += 1
                    same += same_den
    print(f"ctc_beam_bias op: {n} cases, labels equal to the host twin's, scores within 1e-9 of the reference on the kernel's den; "
          f"{same} with the twin's den bit for bit, and then memcmp-equal records")


@pytest.mark.parametrize("with_lm", [False, True])
def test_op_at_the_caps(lib, objs, with_lm):
    """beam = cand = 32 at T = 6, V = 64: 1056 entries per frame from the third frame on, more than one entry per thread."""
    rec, low, _ = against_twin_and_reference(lib, objs, R.scaled_logits(32, 6, 64, 2), 64, 32, 32, 1.0, with_lm, "caps")
    assert not low and len(rec["hyps"]) == 32


def test_op_scale_zero_is_the_plain_kernel(lib, objs):
    """Bias scale 0 without a model: the shared fields of the records are ss_op_ctc_beam's bits."""
    for shape in SHAPES:
        T, V, beam, cand = shape
        for seed in range(5):
            x = small_case(shape, 6, seed)
            rc, plain = R.run(lib, [x], V, PAD, UNK, beam, cand, beam, gpu=True)
            assert rc == 0
            praw = np.frombuffer(plain[0]["raw"][:16 * beam], R.HYP)
            rec = one(lib, x, V, beam, cand, objs[V][0], 0.0, True, gpu=True)
            raw = np.frombuffer(rec["raw"][:40 * beam], RB.BHYP)
            for k in ("score", "n_tokens", "status"):
                assert raw[k].tobytes() == praw[k].tobytes(), (shape, seed, k)
            assert raw["ctc_score"].tobytes() == praw["score"].tobytes()
            assert rec["raw"][40 * beam:] == plain[0]["raw"][16 * beam:]


@pytest.mark.parametrize("with_lm", [False, True])
def test_op_ragged_pack_nan_utterance_and_invariance(lib, objs, with_lm):
    """A pack of T = 1, 12 and 40 and a fourth utterance with a NaN row (status 2): each alone, in the pack and in the reversed
    pack gives memcmp-equal records; sentinels behind every buffer (the runner checks)."""
    V, beam, cand, nbest = 64, 8, 8, 5
    bias, naive, lm, ref_lm = objs[V]
    kw = dict(lm=lm.h, lm_weight=LM_W[0], word_score=LM_W[1]) if with_lm else {}
    xs = [R.scaled_logits(70 + k, T, V, 6) for k, T in enumerate((1, 12, 40, 23))]
    xs[3][4, 40] = np.nan
    rc, recs = RB.run(lib, xs, V, PAD, UNK, beam, cand, nbest, bias.h, 1.0, gpu=True, **kw)
    assert rc == 0
    rc, rev = RB.run(lib, xs[::-1], V, PAD, UNK, beam, cand, nbest, bias.h, 1.0, gpu=True, **kw)
    assert rc == 0
    for k, x in enumerate(xs):
        alone = RB.run(lib, [x], V, PAD, UNK, beam, cand, nbest, bias.h, 1.0, gpu=True, **kw)[1][0]
        assert alone["raw"] == recs[k]["raw"] == rev[len(xs) - 1 - k]["raw"], k
        if k == 3:
            assert recs[k]["status"] == [2] * nbest
        else:
            ref = RB.search(x, V, PAD, UNK, beam, cand, nbest, naive, 1.0, True, ref_lm if with_lm else None, *(LM_W if with_lm else (0.0, 0.0)),
                            True, den=recs[k]["den"])
            assert not RB.compare(recs[k], ref, k) and recs[k]["status"][0] == 0


def test_op_edges_and_refusals(lib, objs):
    bias, naive, lm, _ = objs[64]
    check_edges(lib, bias, naive, gpu=True)
    check_refusals(lib, bias, lm, gpu=True)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


@pytest.fixture(scope="module")
def encs(model):
    from streamspeech_amd import synth
    return [model.encoder_forward(torch.from_numpy(synth.synth_fbank(60 + k, T)).to(model.device), 16, 16)
            for k, T in enumerate((40, 133, 90))]


def phrases_from(hyps, n=6):
    """A hotword set that bears on these hypotheses: up to n distinct bigrams, first those of the runner-up strings that the best
    one lacks, then the best one's own (bigrams cannot occur inside one another, so any set of them is admissible)."""
    best = list(hyps[0].tokens)
    own = list(zip(best, best[1:]))
    pairs = [p for h in hyps[1:] for p in zip(h.tokens, h.tokens[1:]) if p not in own] + own
    out = []
    for p in pairs:
        if len(out) < n and list(p) not in out:
            out.append(list(p))
    return out


def test_model_pack_against_the_op(model, encs, lib):
    """Both heads, bias alone and with a model: ss_batch_ctc_beam_bias's records are bit-equal to ss_op_ctc_beam_bias's on the
    head's own logits (ss_debug_last_logits); score = ctc + scale * bias (+ the model's terms); the set, made of bigrams of the
    plain search's own n-best, earns some hypothesis credit; without bias the call returns what it returned."""
    from streamspeech_amd.engine import CtcBiasHypothesis, CtcHypothesis
    from streamspeech_amd.hotwords import CtcBias
    from streamspeech_amd.modules import Dictionary
    from streamspeech_amd.ngram import NgramLM
    from tests.test_ctc_beam_lm_gpu import dictionary_lm
    cfg = model.cfg
    Tp = [int(e.shape[0]) for e in encs]
    packed = torch.cat(encs, 0).contiguous()
    beam, cand, nbest = 4, 6, 3
    off = np.concatenate([[0], np.cumsum(Tp)])
    for hd, V in ((0, cfg.src_vocab), (1, cfg.tgt_vocab)):
        plain = model.batch_ctc_beam(hd, packed, Tp, beam, cand, nbest)
        assert all(type(h) is CtcHypothesis and h.bias_score is None and len(h) == 4 for hs in plain for h in hs)
        phrases = phrases_from(plain[1])
        assert phrases
        with CtcBias(phrases, 4.0, V, cfg.pad, cfg.unk) as bias, NgramLM(dictionary_lm(Dictionary.placeholder(V), 30 + hd)) as lm:
            for fuse in ({}, dict(lm=lm, lm_weight=0.5, word_score=0.1)):
                got = model.batch_ctc_beam(hd, packed, Tp, beam, cand, nbest, bias=bias, bias_scale=0.8, **fuse)
                logits = model.last_logits().cpu().numpy()
                assert logits.shape[1] == V
                rc, recs = RB.run(lib, [logits[off[b]:off[b + 1]] for b in range(len(Tp))], V, cfg.pad, cfg.unk, beam, cand, nbest, bias.h,
                                  0.8, True, lm.h if fuse else None, fuse.get("lm_weight", 0.0), fuse.get("word_score", 0.0), gpu=True)
                assert rc == 0
                for b in range(len(Tp)):
                    assert len(got[b]) == nbest and all(type(h) is CtcBiasHypothesis for h in got[b])
                    assert [(tuple(h.tokens), h.score, h.ctc_score, h.lm_score or 0.0, h.bias_score) for h in got[b]] == recs[b]["hyps"], (hd, b)
                    for h in got[b]:
                        lm_part = 0.5 * h.lm_score + 0.1 * len(h.tokens) if fuse else 0.0
                        assert (h.lm_score is None) == (not fuse)
                        assert abs(h.score - (h.ctc_score + lm_part + 0.8 * h.bias_score)) <= 1e-9 * max(1.0, abs(h.score))
                assert model.ctc_beam(hd, encs[1], beam, cand, nbest, bias=bias, bias_scale=0.8, **fuse) == got[1]
                assert any(h.bias_score > 0 for h in got[1]), hd
                print(f"ctc_beam_bias model head {hd} lm {bool(fuse)}: n-best of utterance 1 "
                      f"{'changed' if [h.tokens for h in got[1]] != [h.tokens for h in plain[1]] else 'kept'}, best bias_score "
                      f"{got[1][0].bias_score:.2f}")
        assert model.batch_ctc_beam(hd, packed, Tp, beam, cand, nbest) == plain


def test_model_refusals(model, encs):
    from streamspeech_amd import lib as L
    from streamspeech_amd.hotwords import CtcBias
    enc, Tp = encs[1].contiguous(), [int(encs[1].shape[0])]
    cfg = model.cfg
    with CtcBias([[5, 6]], 1.0, cfg.src_vocab, cfg.pad, cfg.unk) as bias, CtcBias([[5, 6]], 1.0, 64, 1, 3) as other, \
            CtcBias([[5, 6]], 1.0, cfg.src_vocab) as no_pad:
        want = model.batch_ctc_beam(0, enc, Tp, 4, bias=bias)
        for kw in (dict(beam=33, bias=bias), dict(beam=4, cand=33, bias=bias), dict(beam=4, nbest=5, bias=bias), dict(beam=4, bias=other),
                   dict(beam=4, bias=no_pad), dict(beam=4, bias=bias, bias_scale=float("nan"))):
            with pytest.raises(L.StreamSpeechHipError) as e:
                model.batch_ctc_beam(0, enc, Tp, **kw)
            assert e.value.code == L.SS_ERR_ARG, kw
        assert model.batch_ctc_beam(0, enc, Tp, 4, bias=bias) == want


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_offline_nbest_columns_only_with_the_flags(tmp_path, model, monkeypatch):
    """--ctc-hotwords-asr alone: the ASR head's .nbest lines are id, rank, score, ctc_score, lm_score (0), bias_score, n_tokens,
    text; the ST head's file and every other file are byte for byte what --ctc-beam alone writes; the ASR lines are what
    HipModel.batch_ctc_beam(bias=...) returned (the driver's own calls, recorded)."""
    from streamspeech_amd import offline
    from streamspeech_amd.engine import HipModel
    from streamspeech_amd.modules import Dictionary
    calls = []
    real = HipModel.batch_ctc_beam

    def recorded(self, head, *a, **kw):
        out = real(self, head, *a, **kw)
        calls.append((head, kw, out))
        return out
    monkeypatch.setattr(HipModel, "batch_ctc_beam", recorded)
    common = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--synthetic", "3", "--no-wav", "--max-len-b-mt", "6", "--ctc-beam", "4",
              "--ctc-nbest", "3"]
    offline.main(common + ["--results-path", str(tmp_path / "beam")])
    d = Dictionary.placeholder(model.cfg.src_vocab)
    seen = [h for c in calls if c[0] == 0 for hs in c[2] for h in hs[:1]]
    phrases = [p for h in seen for p in phrases_from([h], 2)][:1]
    assert phrases
    phrases.append([7 if 7 not in phrases[0] else 8])            # (a one-token phrase that is not inside the first)
    hot = tmp_path / "hot.txt"
    hot.write_text("# hotwords\n" + "".join(" ".join(d[c] for c in p) + ("\t3.0\n" if k else "\n") for k, p in enumerate(phrases)),
                   encoding="utf-8")
    calls.clear()
    offline.main(common + ["--results-path", str(tmp_path / "hot"), "--ctc-hotwords-asr", str(hot), "--ctc-hotword-boost", "2.5"])
    names = sorted(p.name for p in (tmp_path / "beam").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "hot").iterdir())
    for name in names:
        if (tmp_path / "beam" / name).is_file() and name != "generate-test.asr.nbest":
            assert (tmp_path / "beam" / name).read_bytes() == (tmp_path / "hot" / name).read_bytes(), name
    plain = [ln.split("\t") for ln in (tmp_path / "beam" / "generate-test.asr.nbest").read_text(encoding="utf-8").splitlines()]
    rows = [ln.split("\t") for ln in (tmp_path / "hot" / "generate-test.asr.nbest").read_text(encoding="utf-8").splitlines()]
    assert all(len(r) == 5 for r in plain) and all(len(r) == 8 for r in rows) and len(rows) == len(plain) == 9
    for k in range(3):
        grp = rows[3 * k:3 * k + 3]
        assert len({r[0] for r in grp}) == 1 and [int(r[1]) for r in grp] == [0, 1, 2]
        scores = [float(r[2]) for r in grp]
        assert scores == sorted(scores, reverse=True)
        for r in grp:
            assert float(r[4]) == 0.0 and abs(float(r[2]) - (float(r[3]) + float(r[5]))) <= 1e-5 * max(1.0, abs(float(r[2])))
    asr = [c for c in calls if c[0] == 0]
    assert asr and all(c[1].get("bias") is not None and c[1]["bias_scale"] == 1.0 and "lm" not in c[1] for c in asr)
    assert asr[0][1]["bias"].n_phrases == len(phrases) and all("bias" not in c[1] for c in calls if c[0] == 1)
    best = sorted((f"{h[0].score:.6f}", f"{h[0].ctc_score:.6f}", f"{h[0].bias_score:.6f}", str(len(h[0].tokens))) for c in asr for h in c[2])
    assert sorted((r[2], r[3], r[5], r[6]) for r in rows if r[1] == "0") == best
    assert any(float(r[5]) != 0.0 for r in rows)
