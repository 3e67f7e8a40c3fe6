"""The CTC prefix beam search with an n-gram model on the GPU (csrc/ctc_beam.hip: the LM form of the search kernel) through
ss_op_ctc_beam_lm against tests/ctc_beam_lm_ref.py under the rule of tests/test_ctc_beam_lm_cpu.py -- the reference runs on the
kernel's own den, so the n-best ids are equal (to the reference's and the host twin's) and score / ctc_score / lm_score within
1e-9 * max(1, |.|) unless the reference's margin is below 1e-9 -- then ss_batch_ctc_beam_lm on the seeded synthetic checkpoint and
the offline driver's n-best files.  With zero weights the records are ss_op_ctc_beam's; an utterance alone, in a pack and in the
reversed pack gives memcmp-equal records."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import arpa_writer as W
from tests import ctc_align_ref as A
from tests import ctc_beam_lm_ref as RL
from tests import ctc_beam_ref as R
from tests.test_ctc_beam_cpu import PAD, SCALES, SHAPES, UNK, small_case
from tests.test_ctc_beam_lm_cpu import check_edges, check_refusals, one, small_lm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


@pytest.fixture(scope="module")
def lms(lib):
    """{(V, order): (handle, reference scorer)} for the shapes below."""
    from streamspeech_amd.ngram import NgramLM
    out = {}
    for V, order in ((6, 3), (64, 3), (64, 1), (64, 5), (257, 3), (6000, 3)):
        a, ref = small_lm(V, order=order)
        out[(V, order)] = (NgramLM(a), ref)
    yield out
    for lm, _ in out.values():
        lm.close()


def against_reference(lib, lms, x, V, beam, cand, w, ws, name, order=3, eos=True, twin=True):
    lm, ref_lm = lms[(V, order)]
    rec = one(lib, x, V, beam, cand, lm, w, ws, eos=eos, gpu=True)
    ref = RL.search(x, V, PAD, UNK, beam, cand, beam, ref_lm, w, ws, eos, den=rec["den"])
    assert rec["cand_id"].tolist() == ref["cand_id"], name
    low = RL.compare(rec, ref, name)
    if twin:
        host = one(lib, x, V, beam, cand, lm, w, ws, eos=eos)
        assert [h[0] for h in rec["hyps"]] == [h[0] for h in host["hyps"]], name
    print(f"ctc_beam_lm op {name}: margin {ref['margin']:.3e}  best {rec['hyps'][0][1]:.4f} = ctc {rec['hyps'][0][2]:.4f} + lm "
          f"{rec['hyps'][0][3]:.4f} ({len(rec['hyps'][0][0])} tokens)")
    return rec, low


def test_op_small_shapes_of_the_cpu_test(lib, lms):
    """Ten seeds of each (T, V, beam, cand) of the CPU test at both scales and both weight pairs; none may fall back to sorted
    scores."""
    for shape in SHAPES:
        for scale in SCALES:
            for seed in range(10):
                for w, ws in ((0.5, 0.0), (1.0, -0.5)):
                    _, low = against_reference(lib, lms, small_case(shape, scale, seed), shape[1], shape[2], shape[3], w, ws,
                                               (shape, scale, seed, w))
                    assert not low


@pytest.mark.parametrize("V,ld", [(64, 64), (257, 260), (6000, 6000)])
def test_op_vocabularies(lib, lms, V, ld):
    """T = 40, beam / cand = 8 / 8; ld > V with 1e9 behind the row."""
    _, low = against_reference(lib, lms, R.scaled_logits(V, 40, V, 6, ld), V, 8, 8, 0.5, 0.1, f"V{V}")
    assert not low


def test_op_at_the_caps(lib, lms):
    """beam = cand = 32 at T = 150, V = 6000: 1056 entries per frame, every one of them an LM lookup or a node's bonus."""
    rec, _ = against_reference(lib, lms, R.scaled_logits(32, 150, 6000, 6), 6000, 32, 32, 0.5, 0.1, "caps")
    assert len(rec["hyps"]) == 32


@pytest.mark.parametrize("order", [1, 3, 5])
def test_op_orders_and_eos(lib, lms, order):
    """LM orders 1, 3, 5 at V = 64 (with order 5 every hypothesis of the T = 3 case is shorter than the order), eos on and off."""
    for eos in (True, False):
        _, low = against_reference(lib, lms, R.scaled_logits(40 + order, 40, 64, 6), 64, 8, 8, 0.7, -0.2, f"order{order}_eos{eos}", order, eos)
        assert not low
        rec, low = against_reference(lib, lms, R.scaled_logits(50 + order, 3, 64, 6), 64, 8, 8, 0.7, -0.2, f"order{order}_T3_eos{eos}", order, eos)
        assert not low and max(len(h[0]) for h in rec["hyps"]) <= 3


def test_op_one_frame_and_edges(lib, lms):
    check_edges(lib, *lms[(64, 3)], gpu=True)


def test_op_zero_weights_are_the_plain_kernel(lib, lms):
    """lm_weight = word_score = 0: the shared fields of the records are ss_op_ctc_beam's bits, eos term on or off."""
    for shape in SHAPES:
        T, V, beam, cand = shape
        for seed in range(5):
            x = small_case(shape, 6, seed)
            rc, plain = R.run(lib, [x], V, PAD, UNK, beam, cand, beam, gpu=True)
            assert rc == 0
            praw = np.frombuffer(plain[0]["raw"][:16 * beam], R.HYP)
            for eos in (False, True):
                rec = one(lib, x, V, beam, cand, lms[(V, 3)][0], 0.0, 0.0, eos=eos, gpu=True)
                raw = np.frombuffer(rec["raw"][:32 * beam], RL.LMHYP)
                for k in ("score", "n_tokens", "status"):
                    assert raw[k].tobytes() == praw[k].tobytes(), (shape, seed, eos, k)
                assert raw["ctc_score"].tobytes() == praw["score"].tobytes()
                assert rec["raw"][32 * beam:] == plain[0]["raw"][16 * beam:]


def test_op_ragged_pack_nan_utterance_and_invariance(lib, lms):
    """A ragged pack of five, one with a NaN row (status 2) and a T = 1 one: each alone, in the pack and in the reversed pack gives
    memcmp-equal records."""
    V, beam, cand, nbest = 64, 8, 8, 5
    lm, ref_lm = lms[(64, 3)]
    xs = [R.scaled_logits(70 + k, T, V, 6) for k, T in enumerate((23, 40, 7, 1, 55))]
    xs[2][4, 40] = np.nan
    rc, recs = RL.run(lib, xs, V, PAD, UNK, beam, cand, nbest, lm.h, 0.5, 0.1, gpu=True)
    assert rc == 0
    rc, rev = RL.run(lib, xs[::-1], V, PAD, UNK, beam, cand, nbest, lm.h, 0.5, 0.1, gpu=True)
    assert rc == 0
    for k, x in enumerate(xs):
        alone = RL.run(lib, [x], V, PAD, UNK, beam, cand, nbest, lm.h, 0.5, 0.1, gpu=True)[1][0]
        assert alone["raw"] == recs[k]["raw"] == rev[len(xs) - 1 - k]["raw"], k
        ref = RL.search(x, V, PAD, UNK, beam, cand, nbest, ref_lm, 0.5, 0.1, True, den=recs[k]["den"])
        if k == 2:
            assert recs[k]["status"] == [2] * nbest and ref["status"] == 2
        else:
            RL.compare(recs[k], ref, k)
            assert recs[k]["status"][0] == 0


def test_op_refusals(lib, lms):
    check_refusals(lib, lms[(64, 3)][0], gpu=True)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


@pytest.fixture(scope="module")
def encs(model):
    from streamspeech_amd import synth
    return [model.encoder_forward(torch.from_numpy(synth.synth_fbank(60 + k, T)).to(model.device), 16, 16)
            for k, T in enumerate((40, 133, 90))]


def dictionary_lm(d, seed, tmp=None):
    """An order-3 model over every symbol of a Dictionary, as arrays (and as an .arpa file under tmp)."""
    syms = [d[i] for i in range(4, len(d))]
    grams = W.generate(syms, 3, [0, 4000, 4000], seed, logp_range=(-0.8, -0.05))
    if tmp is not None:
        tmp.write_text(W.text(grams), encoding="utf-8")
    return W.arrays(grams, d.index, len(d))


def test_model_pack_against_the_op_and_the_aligner(model, encs, lib):
    """Both heads: ss_batch_ctc_beam_lm's records are bit-equal to ss_op_ctc_beam_lm's on the head's own logits
    (ss_debug_last_logits), align(tokens).score >= ctc_score - T * 2e-5, and without lm the call returns the plain tuples."""
    from streamspeech_amd.modules import Dictionary
    from streamspeech_amd.ngram import NgramLM
    cfg = model.cfg
    Tp = [int(e.shape[0]) for e in encs]
    packed = torch.cat(encs, 0).contiguous()
    beam, cand, nbest = 4, 6, 3
    off = np.concatenate([[0], np.cumsum(Tp)])
    for hd, V in ((0, cfg.src_vocab), (1, cfg.tgt_vocab)):
        with NgramLM(dictionary_lm(Dictionary.placeholder(V), 30 + hd)) as lm:
            got = model.batch_ctc_beam(hd, packed, Tp, beam, cand, nbest, lm=lm, lm_weight=0.5, word_score=0.1)
            logits = model.last_logits().cpu().numpy()
            assert logits.shape[1] == V
            rc, recs = RL.run(lib, [logits[off[b]:off[b + 1]] for b in range(len(Tp))], V, cfg.pad, cfg.unk, beam, cand, nbest, lm.h,
                              0.5, 0.1, gpu=True)
            assert rc == 0
            for b in range(len(Tp)):
                assert len(got[b]) == nbest
                assert [(tuple(h.tokens), h.score, h.ctc_score, h.lm_score) for h in got[b]] == recs[b]["hyps"], (hd, b)
                for h in got[b]:
                    a = model.ctc_align(hd, encs[b], h.tokens, want_path=False)
                    assert a.status == 0 and a.score >= h.ctc_score - Tp[b] * A.TOL, (hd, b, h.ctc_score, a.score)
                    assert abs(h.score - (h.ctc_score + 0.5 * h.lm_score + 0.1 * len(h.tokens))) <= 1e-9 * max(1.0, abs(h.score))
            assert model.ctc_beam(hd, encs[1], beam, cand, nbest, lm=lm, lm_weight=0.5, word_score=0.1) == got[1]
            no_eos = model.batch_ctc_beam(hd, packed, Tp, beam, cand, nbest, lm=lm, lm_weight=0.5, word_score=0.1, lm_eos=False)
            assert all(abs(h.score - (h.ctc_score + 0.5 * h.lm_score + 0.1 * len(h.tokens))) <= 1e-9 * max(1.0, abs(h.score))
                       for hs in no_eos for h in hs)
        plain = model.batch_ctc_beam(hd, packed, Tp, beam, cand, nbest)
        assert all(h.ctc_score is None and h.lm_score is None and len(h) == 4 for hs in plain for h in hs)


def test_model_scratch_cap_and_refusals(model, encs):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    from streamspeech_amd.modules import Dictionary
    from streamspeech_amd.ngram import NgramLM
    enc, Tp = encs[1].contiguous(), [int(encs[1].shape[0])]
    with NgramLM(dictionary_lm(Dictionary.placeholder(model.cfg.src_vocab), 30)) as lm, \
            NgramLM(small_lm(64)[0]) as other:
        sc = Scratch(model.device)
        ctx = model.new_context(sc)
        ctx.batch_ctc_greedy(0, enc, Tp)                         # the logits workspace and the segment buffer are booked
        want = model.batch_ctc_beam(0, enc, Tp, 4, lm=lm, lm_weight=0.5)
        sc.set_cap(sc.bytes() + 64)
        before = sc.bytes()
        with pytest.raises(L.StreamSpeechHipError) as e:
            ctx.batch_ctc_beam(0, enc, Tp, 4, lm=lm, lm_weight=0.5)
        assert e.value.code == L.SS_ERR_SCRATCH_CAP and sc.bytes() == before and sc.audit()[0] == sc.audit()[1]
        # the refusals through the C ABI itself, on sentinel-filled outputs: nothing is written
        hyp = torch.full((8 * 4,), -7, dtype=torch.int32, device=model.device)
        tok = torch.full((4 * Tp[0],), -7, dtype=torch.int32, device=model.device)

        def raw(handle, beam, lm_h, w=0.5):
            opts = L.SSCtcLmOpts(w, 0.0, 1)
            return model.lib.ss_batch_ctc_beam_lm(handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), 0, 1, C.c_void_p(enc.data_ptr()),
                                                  (C.c_int32 * 1)(*Tp), beam, 5, min(beam, 4), C.c_void_p(hyp.data_ptr()),
                                                  C.c_void_p(tok.data_ptr()), Tp[0], lm_h, C.byref(opts))
        assert raw(ctx.h, 4, lm.h) == L.SS_ERR_SCRATCH_CAP
        assert raw(model.h, 33, lm.h) == raw(model.h, 4, None) == raw(model.h, 4, other.h) == raw(model.h, 4, lm.h, float("nan")) == L.SS_ERR_ARG
        torch.cuda.synchronize()
        assert bool((hyp == -7).all()) and bool((tok == -7).all())
        sc.set_cap(0)
        assert ctx.batch_ctc_beam(0, enc, Tp, 4, lm=lm, lm_weight=0.5) == want
        assert raw(model.h, 4, lm.h) == 0
        torch.cuda.synchronize()
        assert not bool((hyp == -7).any())
        for kw in (dict(beam=33), dict(beam=4, cand=33), dict(beam=4, nbest=5), dict(beam=0), dict(beam=4, lm_weight=float("nan")),
                   dict(beam=4, word_score=float("inf"))):
            with pytest.raises(L.StreamSpeechHipError) as e:
                model.batch_ctc_beam(0, enc, Tp, lm=lm, **kw)
            assert e.value.code == L.SS_ERR_ARG, kw
        for head, m in ((2, lm), (0, other)):                    # no such head; a model of another vocabulary
            with pytest.raises(L.StreamSpeechHipError) as e:
                model.batch_ctc_beam(head, enc, Tp, 4, lm=m)
            assert e.value.code == L.SS_ERR_ARG
        assert model.batch_ctc_beam(0, enc, Tp, 4, lm=lm, lm_weight=0.5) == want


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_offline_nbest_columns_only_with_the_flags(tmp_path, model, monkeypatch):
    """--ctc-lm-asr alone: the ASR head's .nbest lines get ctc_score and lm_score after score, the ST head's file and every other
    file are what --ctc-beam alone writes; the lines are what HipModel.batch_ctc_beam(lm=...) returned for the ASR head (the
    driver's own calls, recorded), rank 0 its best."""
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
    arpa = tmp_path / "src.arpa"
    dictionary_lm(Dictionary.placeholder(model.cfg.src_vocab), 30, arpa)
    common = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--synthetic", "3", "--no-wav", "--max-len-b-mt", "6", "--ctc-beam", "4",
              "--ctc-nbest", "3"]
    offline.main(common + ["--results-path", str(tmp_path / "beam")])
    calls.clear()
    offline.main(common + ["--results-path", str(tmp_path / "lm"), "--ctc-lm-asr", str(arpa), "--ctc-lm-weight", "0.8", "--ctc-word-score",
                           "0.2"])
    names = sorted(p.name for p in (tmp_path / "beam").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "lm").iterdir())
    for name in names:
        if (tmp_path / "beam" / name).is_file() and name != "generate-test.asr.nbest":
            assert (tmp_path / "beam" / name).read_bytes() == (tmp_path / "lm" / name).read_bytes(), name
    plain = [ln.split("\t") for ln in (tmp_path / "beam" / "generate-test.asr.nbest").read_text(encoding="utf-8").splitlines()]
    rows = [ln.split("\t") for ln in (tmp_path / "lm" / "generate-test.asr.nbest").read_text(encoding="utf-8").splitlines()]
    assert all(len(r) == 5 for r in plain) and all(len(r) == 7 for r in rows) and len(rows) == len(plain) == 9
    for k in range(3):
        grp = rows[3 * k:3 * k + 3]
        assert len({r[0] for r in grp}) == 1 and [int(r[1]) for r in grp] == [0, 1, 2]
        scores = [float(r[2]) for r in grp]
        assert scores == sorted(scores, reverse=True)
        for r in grp:
            assert abs(float(r[2]) - (float(r[3]) + 0.8 * float(r[4]) + 0.2 * int(r[5]))) <= 1e-5 * max(1.0, abs(float(r[2])))
            assert float(r[3]) <= 0.0 and float(r[4]) < 0.0
    asr = [c for c in calls if c[0] == 0]
    assert asr and all(c[1].get("lm") is not None and (c[1]["lm_weight"], c[1]["word_score"]) == (0.8, 0.2) for c in asr)
    assert all("lm" not in c[1] for c in calls if c[0] == 1)
    best = sorted((f"{h[0].score:.6f}", f"{h[0].ctc_score:.6f}", f"{h[0].lm_score:.6f}", str(len(h[0].tokens))) for c in asr for h in c[2])
    assert sorted(tuple(r[2:6]) for r in rows if r[1] == "0") == best
