"""CTC prefix beam search on the GPU (csrc/ctc_beam.hip): the two kernels through ss_op_ctc_beam against tests/ctc_beam_ref.py under
the rule of tests/test_ctc_beam_cpu.py -- the reference runs on the kernel's own den, so the n-best ids are equal and the scores
within 1e-9 * max(1, |score|) unless the reference's margin is below 1e-9 (then sorted scores) -- then ss_batch_ctc_beam on the seeded
synthetic checkpoint and the offline driver's n-best files.

Bounds: den within TOL = 2e-5 of the float64 log-sum-exp (the bound and the arithmetic of tests/test_ctc_scores_gpu.py); a
hypothesis sums a subset of its labels' alignments over T per-frame values, so its score is at most the aligner's + T * 2e-5; an
utterance alone, in a pack and in the reversed pack: memcmp-equal records."""
import numpy as np
import pytest
import torch

from tests import ctc_align_ref as A
from tests import ctc_beam_ref as R
from tests.test_ctc_beam_cpu import PAD, UNK, check_pack, check_refusals, one, small_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------
def _against_reference(lib, x, V, beam, cand, name):
    rec = one(lib, x, V, beam, cand, gpu=True)
    ref = R.search(x, V, PAD, UNK, beam, cand, beam, den=rec["den"])
    assert rec["cand_id"].tolist() == ref["cand_id"], name
    low = R.compare(rec, ref, name)
    x64 = x[:, :V].astype(np.float64)
    m = x64.max(axis=1)
    err = np.abs((rec["den"][:, 0].astype(np.float64) + rec["den"][:, 1]) - (m + np.log(np.exp(x64 - m[:, None]).sum(axis=1)))).max()
    print(f"ctc_beam op {name}: margin {ref['margin']:.3e}  max |den - f64| = {err:.3e}  best {rec['hyps'][0][1]:.4f}")
    assert err <= A.TOL
    return rec, low


def test_op_small_shapes_of_the_cpu_test(lib):
    """Ten seeds of each (T, V, beam, cand) of the CPU test at both scales; none may fall back to sorted scores."""
    from tests.test_ctc_beam_cpu import SCALES, SHAPES
    for shape in SHAPES:
        for scale in SCALES:
            for seed in range(10):
                _, low = _against_reference(lib, small_case(shape, scale, seed), shape[1], shape[2], shape[3], (shape, scale, seed))
                assert not low


@pytest.mark.parametrize("V,ld", [(64, 64), (257, 260), (6000, 6000)])
def test_op_vocabularies(lib, V, ld):
    """T = 40, beam / cand = 8 / 8: one, two and 24 columns per thread of the candidate kernel; ld > V with 1e9 behind the row."""
    x = R.scaled_logits(V, 40, V, 6, ld)
    rec, _ = _against_reference(lib, x, V, 8, 8, f"V{V}")
    host = one(lib, x, V, 8, 8)
    assert rec["cand_id"].tolist() == host["cand_id"].tolist() and [y for y, _ in rec["hyps"]] == [y for y, _ in host["hyps"]]


def test_op_at_the_caps(lib):
    """beam = cand = 32, T = 320, V = 6000: 1056 entries per frame, the largest trie and child table of the test."""
    x = R.scaled_logits(32, 320, 6000, 6)
    rec, _ = _against_reference(lib, x, 6000, 32, 32, "caps")
    assert len(rec["hyps"]) == 32


def test_op_one_frame_and_edges(lib):
    V = 64
    rec, _ = _against_reference(lib, R.scaled_logits(1, 1, V, 6), V, 4, 3, "T1")
    assert sorted(len(y) for y, _ in rec["hyps"]) == [0, 1, 1, 1]
    _against_reference(lib, R.scaled_logits(2, 20, V, 6), V, 1, 1, "beam1_cand1")
    x = np.full((1, V), -np.inf, np.float32)
    x[0, [0, 9]] = [1.0, 2.0]
    rec = one(lib, x, V, 8, 4, gpu=True)
    assert rec["status"] == [0, 0] + [1] * 6 and [y for y, _ in rec["hyps"]] == [(9,), ()]
    x = R.scaled_logits(3, 30, V, 6, ld=70)
    x[:, [PAD, UNK]] = 50.0
    rec, _ = _against_reference(lib, x, V, 8, 8, "pad_unk_on_top")
    assert all(PAD not in y and UNK not in y for y, _ in rec["hyps"]) and not np.isin(rec["cand_id"], [0, PAD, UNK]).any()
    tie = A.logits(5, 6, V)
    tie[2, 1:V] = np.float32(0.5)
    rec, _ = _against_reference(lib, tie, V, 4, 8, "tied_row")
    assert rec["cand_id"][2].tolist() == [2, 4, 5, 6, 7, 8, 9, 10]


def test_op_ragged_pack_nan_utterance_and_invariance(lib):
    """A ragged pack of eight with a NaN utterance and a T = 1 utterance in the middle; each alone and the reversed pack: the same
    bytes."""
    check_pack(lib, gpu=True)


def test_op_refusals(lib):
    check_refusals(lib, gpu=True)                                # (run checks that nothing was written)
    x = R.scaled_logits(5, 12, 64, 6)
    full = one(lib, x, 64, 4, 4, gpu=True)
    rc, recs = R.run(lib, [x], 64, PAD, UNK, 4, 4, 4, gpu=True, want_den=False)
    assert rc == 0 and recs[0]["raw"] == full["raw"]


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


@pytest.fixture(scope="module")
def encs(model):
    from streamspeech_amd import synth
    return [model.encoder_forward(torch.from_numpy(synth.synth_fbank(60 + k, T)).to(model.device), 16, 16)
            for k, T in enumerate((40, 133, 330, 90))]


def test_model_pack_of_four_against_the_op_and_the_aligner(model, encs, lib):
    """Both heads: ss_batch_ctc_beam's records are bit-equal to ss_op_ctc_beam's on the head's own logits (ss_debug_last_logits), no
    score exceeds batch_ctc_align's for the same labels by more than T * 2e-5, and CTCDecoder.beam_search returns the same."""
    from streamspeech_amd.generators import CTCDecoder
    cfg = model.cfg
    Tp = [int(e.shape[0]) for e in encs]
    packed = torch.cat(encs, 0).contiguous()
    beam, cand, nbest = 4, 6, 3
    for hd in (0, 1):
        got = model.batch_ctc_beam(hd, packed, Tp, beam, cand, nbest)
        logits = model.last_logits().cpu().numpy()
        V = logits.shape[1]
        off = np.concatenate([[0], np.cumsum(Tp)])
        rc, recs = R.run(lib, [logits[off[b]:off[b + 1]] for b in range(4)], V, cfg.pad, cfg.unk, beam, cand, nbest, gpu=True)
        assert rc == 0
        for b in range(4):
            assert len(got[b]) == nbest and [(tuple(h.tokens), h.score) for h in got[b]] == recs[b]["hyps"], (hd, b)
            assert all(0 not in h.tokens and cfg.pad not in h.tokens and cfg.unk not in h.tokens for h in got[b])
            al = [model.ctc_align(hd, encs[b], h.tokens, want_path=False) for h in got[b]]
            for h, a in zip(got[b], al):
                assert a.status == 0 and h.score <= a.score + Tp[b] * A.TOL, (hd, b, h.score, a.score)
            print(f"ss_batch_ctc_beam head {hd} Tp {Tp[b]}: best {got[b][0].score:.4f} ({len(got[b][0].tokens)} tokens), aligner "
                  f"{al[0].score:.4f}")
        alone = model.ctc_beam(hd, encs[1], beam, cand, nbest)
        assert alone == got[1]

        class Dict:
            def pad(self): return cfg.pad
            def eos(self): return cfg.eos
            def unk(self): return cfg.unk

        hyps = CTCDecoder(Dict(), model, hd).beam_search({"encoder_out": [encs[1].unsqueeze(1)]}, beam, cand=cand, nbest=nbest)[0]
        assert [(h["tokens"].tolist(), h["score"]) for h in hyps] == [(h.tokens, h.score) for h in got[1]]


def test_model_scratch_cap_and_refusals(model, encs):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    enc, Tp = encs[1].contiguous(), [int(encs[1].shape[0])]
    sc = Scratch(model.device)
    ctx = model.new_context(sc)
    ctx.batch_ctc_greedy(0, enc, Tp)                             # the logits workspace and the segment buffer are booked
    want = model.batch_ctc_beam(0, enc, Tp, 4)
    sc.set_cap(sc.bytes() + 64)
    before = sc.bytes()
    with pytest.raises(L.StreamSpeechHipError) as e:
        ctx.batch_ctc_beam(0, enc, Tp, 4)
    assert e.value.code == L.SS_ERR_SCRATCH_CAP and sc.bytes() == before and sc.audit()[0] == sc.audit()[1]
    sc.set_cap(0)
    assert ctx.batch_ctc_beam(0, enc, Tp, 4) == want
    assert sc.bytes() > before and sc.audit()[0] == sc.audit()[1]
    for kw in (dict(beam=33), dict(beam=4, cand=33), dict(beam=4, nbest=5), dict(beam=0)):
        with pytest.raises(L.StreamSpeechHipError) as e:
            model.batch_ctc_beam(0, enc, Tp, **kw)
        assert e.value.code == L.SS_ERR_ARG
    with pytest.raises(L.StreamSpeechHipError) as e:
        model.batch_ctc_beam(2, enc, Tp, 4)
    assert e.value.code == L.SS_ERR_ARG
    assert model.batch_ctc_beam(0, enc, Tp, 4) == want           # the context is as usable as before


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_offline_writes_the_nbest_files_only_with_the_flag(tmp_path):
    from streamspeech_amd import offline
    common = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--synthetic", "3", "--no-wav", "--max-len-b-mt", "6"]
    offline.main(common + ["--results-path", str(tmp_path / "plain")])
    offline.main(common + ["--results-path", str(tmp_path / "beam"), "--ctc-beam", "4", "--ctc-nbest", "3"])
    plain = sorted(p.name for p in (tmp_path / "plain").iterdir())
    beam = sorted(p.name for p in (tmp_path / "beam").iterdir())
    assert not any(n.endswith(".nbest") for n in plain)
    assert sorted(set(beam) - set(plain)) == ["generate-test.asr.nbest", "generate-test.st.nbest"]
    for name in plain:
        if (tmp_path / "plain" / name).is_file():
            assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "beam" / name).read_bytes(), name
    for key in ("asr", "st"):
        rows = [ln.split("\t") for ln in (tmp_path / "beam" / f"generate-test.{key}.nbest").read_text(encoding="utf-8").splitlines()]
        assert all(len(r) == 5 for r in rows) and len(rows) == 3 * 3
        for k in range(3):
            grp = rows[3 * k:3 * k + 3]
            assert len({r[0] for r in grp}) == 1 and [int(r[1]) for r in grp] == [0, 1, 2]
            scores = [float(r[2]) for r in grp]
            assert scores == sorted(scores, reverse=True) and scores[0] > -np.inf and scores[0] <= 0.0
            assert all(int(r[3]) >= 0 for r in grp)
