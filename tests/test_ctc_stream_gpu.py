"""The resumable CTC prefix beam search on the GPU (the resumable kernels of csrc/ctc_beam.hip, csrc/ctc_stream.hip).  The oracle is
the one-shot search on the same device (ss_op_ctc_beam / ss_op_ctc_beam_lm, which tests/test_ctc_beam_gpu.py and
tests/test_ctc_beam_lm_gpu.py pin to the Python reference), and every comparison is memcmp of records and owned tokens: the checks
of tests/test_ctc_stream_cpu.py again through ss_op_ctc_stream_advance, then a large vocabulary and the caps, then
engine.CtcStream on the seeded synthetic checkpoint behind the incremental encoder (a StreamPool and encoder_stream_forward)
against ss_batch_ctc_beam(_lm) on the finished utterance.

Device against host twin: the two compute a row's log-sum with different expf, so their den differ in the last bits and, as in
tests/test_ctc_beam_gpu.py (test_op_vocabularies), the comparison between them is of the label strings, not of the score bytes."""
import numpy as np
import pytest
import torch

from tests import ctc_beam_ref as R
from tests import ctc_stream_ref as S
from tests.test_ctc_beam_cpu import PAD, SCALES, SHAPES, UNK
from tests.test_ctc_beam_lm_cpu import small_lm
from tests.test_ctc_stream_cpu import (WEIGHTS, check_advance_refusals, check_create_refusals, check_pack, check_slot_reuse,
                                       check_split_invariance, check_stream)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


@pytest.fixture(scope="module")
def lms(lib):
    from streamspeech_amd.ngram import NgramLM
    out = {V: NgramLM(small_lm(V)[0]) for V in sorted({s[1] for s in SHAPES})}
    yield out
    for lm in out.values():
        lm.close()


# ---- the kernels on the CPU test's cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_op_split_invariance_and_partials(lib, lms, shape, scale):
    n = check_split_invariance(lib, lms, shape, scale, gpu=True)
    print(f"ctc_stream op {shape} scale {scale}: {n} streams, every call memcmp-equal to ss_op_ctc_beam(_lm)")


def test_op_pack_nan_session_and_invariance(lib, lms):
    check_pack(lib, gpu=True)
    check_pack(lib, lms[64], WEIGHTS[0], gpu=True)


def test_op_slot_reuse(lib, lms):
    check_slot_reuse(lib, gpu=True)
    check_slot_reuse(lib, lms[64], WEIGHTS[1], gpu=True)


def test_op_refusals(lib, lms):
    check_create_refusals(lib, lms[64], gpu=True)
    check_advance_refusals(lib, gpu=True)
    check_advance_refusals(lib, lms[64], gpu=True)


# ---- vocabularies and caps ----------------------------------------------------------------------------------------------------------
def test_op_large_vocabulary_and_the_host_twin(lib):
    """V = ld = 6000 (24 columns per thread of the candidate kernel), T = 40, beam / cand 8 / 8, in calls of 1, 23 and 16 frames;
    the host twin on the same calls finds the same label strings."""
    V, T = 6000, 40
    x = R.scaled_logits(V, T, V, 6, V)
    check_stream(lib, x, V, 8, 8, [1, 24], gpu=True)
    got = {}
    for gpu in (True, False):
        with S.Stream(lib, V, PAD, UNK, 1, T, 8, 8, 8, gpu=gpu) as st:
            f = 0
            for t in (1, 24, 40):
                rc, recs = st.advance([0], [x[f:t]], [t], [t == T])
                assert rc == 0
                got[(gpu, t)] = ([h[0] for h in recs[0]["hyps"]], recs[0]["part"])
                f = t
    for t in (1, 24, 40):
        assert got[(True, t)] == got[(False, t)], t


def test_op_at_the_caps_with_a_model(lib, lms):
    """beam = cand = 32, T = 64 in an object made for 1500 frames (the largest trie and child table), in calls of 1, 31 and 32
    frames, with the model."""
    x = R.scaled_logits(33, 64, 64, 2)
    check_stream(lib, x, 64, 32, 32, [1, 32], lms[64], WEIGHTS[0], gpu=True, max_frames=1500)
    check_stream(lib, x, 64, 32, 32, [1, 32], gpu=True, max_frames=1500)


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


LENS, STEP, CHUNK, MAX_ROWS = (160, 533, 1320), 32, 16, 340


@pytest.fixture(scope="module")
def fbanks(model):
    from streamspeech_amd import synth
    return [torch.from_numpy(synth.synth_fbank(80 + k, T)).to(model.device) for k, T in enumerate(LENS)]


@pytest.fixture(scope="module")
def head_lms(model):
    from streamspeech_amd.modules import Dictionary
    from streamspeech_amd.ngram import NgramLM
    from tests.test_ctc_beam_lm_gpu import dictionary_lm
    out = [NgramLM(dictionary_lm(Dictionary.placeholder(V), 30 + hd)) for hd, V in enumerate((model.cfg.src_vocab, model.cfg.tgt_vocab))]
    yield out
    for lm in out:
        lm.close()


BEAM, CAND, NBEST = 4, 6, 3
FUSE = dict(lm_weight=0.5, word_score=0.1)


def _streams(model, head_lms, n):
    from streamspeech_amd.engine import CtcStream
    return {(hd, fused): CtcStream(model, hd, n, MAX_ROWS, BEAM, CAND, NBEST, **(dict(lm=head_lms[hd], **FUSE) if fused else {}))
            for hd in (0, 1) for fused in (False, True)}


def test_model_streams_against_the_batch_call(model, fbanks, head_lms):
    """Three sessions of 160, 533 and 1320 fbank frames fed 32 frames a step at chunk 16, in a StreamPool and then each alone
    through encoder_stream_forward: CtcStream.advance takes each step's n_final (everything, with final, at a session's last step).
    Both heads, plain and with a model: a session's last call returns exactly batch_ctc_beam's hypotheses on its finished encoder
    output, in the pool and alone, after the same frame counts per step; the stable prefix only grows and never changes."""
    assert model.pack_invariant()
    n = len(LENS)
    want, trace = {}, {}
    # ---- in a pool ----
    pool = model.stream_pool(n, MAX_ROWS)
    cs = _streams(model, head_lms, n)
    try:
        for step in range(-(-max(LENS) // STEP)):
            fed = [min(T, STEP * (step + 1)) for T in LENS]
            act = [i for i, T in enumerate(LENS) if STEP * step < T]
            out, views, nf, _ = pool.forward(act, [fbanks[i][:fed[i]].contiguous() for i in act], [CHUNK] * len(act), [CHUNK] * len(act))
            T2 = [int(v.shape[0]) for v in views]
            final = [fed[i] == LENS[i] for i in act]
            upto = [t2 if fin else k for t2, k, fin in zip(T2, nf, final)]
            for key, st in cs.items():
                parts = st.advance(act, out, T2, upto, final)
                for i, p, u in zip(act, parts, upto):
                    assert p.frames == u and p.final == (fed[i] == LENS[i])
                    trace.setdefault((key, i), []).append(p)
            for i, v, fin in zip(act, views, final):
                if fin:
                    for hd, fused in cs:
                        kw = dict(lm=head_lms[hd], **FUSE) if fused else {}
                        want[((hd, fused), i)] = model.batch_ctc_beam(hd, v.contiguous(), [int(v.shape[0])], BEAM, CAND, NBEST, **kw)[0]
                    pool.reset(i)
    finally:
        for st in cs.values():
            st.close()
    for (key, i), parts in trace.items():
        assert parts[-1].final and parts[-1].hyps == want[(key, i)], (key, i)
        assert len(parts[-1].hyps) == NBEST
        stable, toks = 0, []
        for p in parts:
            assert p.n_stable >= stable and all(h.tokens[:stable] == toks for h in p.hyps), (key, i)
            stable, toks = p.n_stable, p.hyps[0].tokens[:p.n_stable]
        assert want[(key, i)][0].tokens[:stable] == toks
    for i, T in enumerate(LENS):
        parts = trace[((0, False), i)]
        lag = np.mean([len(p.hyps[0].tokens) - p.n_stable for p in parts])
        print(f"ctc_stream model: fbank {T}: {parts[-1].frames} frames, {len(parts[-1].hyps[0].tokens)} tokens in {len(parts)} calls, "
              f"mean lag of n_stable behind the best hypothesis {lag:.2f} tokens")
    # ---- each alone, through the single-stream encoder ----
    cs = _streams(model, head_lms, 1)
    try:
        for i, T in enumerate(LENS):
            model.encoder_stream_reset()
            for step in range(-(-T // STEP)):
                fed = min(T, STEP * (step + 1))
                out = model.encoder_stream_forward(fbanks[i][:fed].contiguous(), CHUNK, CHUNK)
                T2, fin = int(out.shape[0]), fed == T
                upto = T2 if fin else int(model.stream_stats[0])
                for key, st in cs.items():
                    p = st.advance([0], out, [T2], [upto], [fin])[0]
                    assert (p.frames, p.final) == (trace[(key, i)][step].frames, fin), (key, i, step)
                    if fin:                                    # (this encoder's own rows: its own oracle)
                        kw = dict(lm=head_lms[key[0]], **FUSE) if key[1] else {}
                        assert p.hyps == model.batch_ctc_beam(key[0], out, [T2], BEAM, CAND, NBEST, **kw)[0], (key, i)
        model.encoder_stream_reset()
    finally:
        for st in cs.values():
            st.close()


def test_model_stream_scratch_bookings_and_refusals(model, fbanks, head_lms):
    """The state is booked on the model's scratch set in one piece of the header's size, refused on the cap with the set as it
    was, and released by close(); the model call's own refusals (upto above the session's rows, another model's object)."""
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import CtcStream, Scratch
    sc = Scratch(model.device)
    ctx = model.new_context(sc)
    enc = ctx.encoder_forward(fbanks[0], CHUNK, CHUNK).contiguous()
    T2 = int(enc.shape[0])
    want = ctx.batch_ctc_beam(0, enc, [T2], BEAM, CAND, NBEST)[0]
    start = sc.bytes()
    slots, nodes = 1024, 1 + BEAM * 100                          # the power of two >= 2 * 4 * 100
    per_slot = 12 * slots + 8 * nodes + 40 * BEAM + 8
    sc.set_cap(start + 3 * per_slot - 1)
    with pytest.raises(L.StreamSpeechHipError) as e:
        CtcStream(ctx, 0, 3, 100, BEAM, CAND, NBEST)
    assert e.value.code == L.SS_ERR_SCRATCH_CAP and sc.bytes() == start and sc.audit()[0] == sc.audit()[1]
    sc.set_cap(start + 3 * per_slot)
    with CtcStream(ctx, 0, 3, 100, BEAM, CAND, NBEST) as st:
        assert sc.bytes() == start + 3 * per_slot and sc.audit()[0] == sc.audit()[1]
        sc.set_cap(0)
        for bad in (dict(upto=[T2 + 1]), dict(T=[T2 - 1]), dict(slots=[3])):
            kw = dict(slots=[2], T=[T2], upto=[T2], final=[True])
            kw.update(bad)
            with pytest.raises(L.StreamSpeechHipError) as e:
                st.advance(kw["slots"], enc, kw["T"], kw["upto"], kw["final"])
            assert e.value.code == L.SS_ERR_ARG
        st.model = model                                        # a model on another scratch set than the object's
        with pytest.raises(L.StreamSpeechHipError) as e:
            st.advance([2], enc, [T2], [T2], [True])
        assert e.value.code == L.SS_ERR_ARG
        st.model = ctx
        with pytest.raises(L.StreamSpeechHipError) as e:
            st.reset(3)
        assert e.value.code == L.SS_ERR_ARG
        a = st.advance([2], enc, [T2], [T2 // 2], [False])[0]
        assert a.frames == T2 // 2 and not a.final
        assert st.advance([2], enc, [T2], [T2], [True])[0].hyps == want
        with CtcStream(ctx, 0, 1, 100, BEAM, lm=head_lms[0], **FUSE) as fused:
            assert sc.bytes() >= start + 3 * per_slot + per_slot + 20 * nodes
            got = fused.advance([0], enc, [T2], [T2], [True])[0].hyps
        assert got == ctx.batch_ctc_beam(0, enc, [T2], BEAM, lm=head_lms[0], **FUSE)[0]
        held = sc.bytes()                                       # (the calls' own workspaces have grown: they stay)
    assert sc.bytes() == held - 3 * per_slot and sc.audit()[0] == sc.audit()[1]
    for kw in (dict(beam=33), dict(beam=4, cand=33), dict(beam=4, nbest=5), dict(beam=0), dict(beam=4, max_frames=1501),
               dict(beam=4, max_frames=0), dict(beam=4, max_sessions=0), dict(beam=4, head=2)):
        args = dict(head=0, max_sessions=1, max_frames=100)
        args.update(kw)
        with pytest.raises(L.StreamSpeechHipError) as e:
            CtcStream(ctx, **args)
        assert e.value.code == L.SS_ERR_ARG, kw


# ---- the session pool and the agent ------------------------------------------------------------------------------------------------
def _pool_plan():
    """Four ASR sessions (2.1 - 5.3 s, 320 / 640 ms segments, one joining late) and one S2TT session."""
    from streamspeech_amd import synth
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    from tests import ref_fixtures as RF
    plan = {}
    for i, (kind, secs, ms, start) in enumerate((("asr", 2.1, 320, 0), ("asr", 5.3, 320, 0), ("s2tt", 4.0, 320, 1), ("asr", 3.2, 640, 2),
                                                 ("asr", 4.4, 320, 0))):
        args = RF.agent_args(StreamSpeechS2TTAgent if kind == "s2tt" else StreamSpeechASRAgent, ms, 16000)
        plan[f"{kind}{i}"] = (kind, args, synth.synth_pcm(2000 + i, int(16000 * secs)), 16000, ms, start)
    return plan


def test_pool_asr_sessions_on_the_prefix_search(model, synth_weights):
    """A TextSessionPool(ctc_beam=...) with four ASR sessions and one S2TT session: every ASR session's writes add up to the
    " ".join of its final best hypothesis and each write only appends; nbest(sid) is batch_ctc_beam on the rows its last advance
    saw; the S2TT session answers what it answers in a pool without the option; the step counters appear only with the option,
    and an ASR-only step of such a pool runs no row through the arg-max heads."""
    from streamspeech_amd.engine import ctc_beam_default_cand
    from streamspeech_amd.text_policy import CtcBeamOptions
    from streamspeech_amd.text_pool import TextSessionPool
    from tests import ref_fixtures as RF
    from tests.test_text_pool_gpu import _drive
    cfg = synth_weights[0]
    plan = _pool_plan()
    plain = TextSessionPool(model, 8, 256)
    want = _drive(plain, plan, cfg)
    assert plain.ctc_stream is None and "ctc_stream_calls" not in plain.last_step
    pool = TextSessionPool(model, 8, 256, ctc_beam=CtcBeamOptions(4))
    finals, advance = {}, pool.ctc_stream.advance

    def spy(slots, enc_packed, T, upto, final):
        got = advance(slots, enc_packed, T, upto, final)
        sid_of = {s.slot: sid for sid, s in pool.sessions.items() if s.slot is not None}
        off = 0
        for sl, t, fin, p in zip(slots, T, final, got):
            if fin:
                ref = model.batch_ctc_beam(0, enc_packed[off:off + t].contiguous(), [t], 4, ctc_beam_default_cand(4), 4)[0]
                assert p.hyps == ref, sid_of[sl]
                finals[sid_of[sl]] = ref
            off += t
        return got

    pool.ctc_stream.advance = spy
    got = _drive(pool, plan, cfg)
    assert {"ctc_stream_calls", "ctc_stream_rows"} <= set(pool.last_step)
    d = RF.dictionaries(cfg)
    sids = {name: sid for sid, name in enumerate(plan)}          # open() numbers the sessions in plan order
    for name, recs in got.items():
        if name.startswith("s2tt"):
            assert recs == want[name], name
            continue
        best = finals[sids[name]][0]
        text = "".join(c or "" for _, c, _ in recs)
        assert text == " ".join(d["source_unigram"][c] for c in best.tokens), name
        assert pool.nbest(sids[name]) == finals[sids[name]] and pool.partial(sids[name]) is None
        print(f"ctc_stream pool {name}: {len(recs)} steps, {len(best.tokens)} tokens, {sum(1 for _, c, _ in recs[:-1] if c)} early writes")
    # an ASR-only step: the searches' rows, no arg-max rows
    solo = TextSessionPool(model, 2, 256, ctc_beam=CtcBeamOptions(4, nbest=2))
    one = {k: v for k, v in plan.items() if k == "asr0"}
    _drive(solo, one, cfg)
    assert solo.pool.stats()[1] == 0 and solo.last_step["ctc_stream_calls"] == 1 and solo.last_step["ctc_stream_rows"] > 0
    assert len(solo.nbest(0)) == 2
    with pytest.raises(ValueError):
        TextSessionPool(model, 2, 256, details=True, ctc_beam=CtcBeamOptions(4))


def test_asr_agent_with_ctc_beam_writes_what_the_pool_session_writes(model, synth_weights):
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_policy import CtcBeamOptions
    from streamspeech_amd.text_pool import TextSessionPool
    from tests import ref_fixtures as RF
    from tests.test_text_pool_gpu import _drive
    cfg = synth_weights[0]
    plan = {k: v for k, v in _pool_plan().items() if k == "asr1"}
    kind, _, pcm, sr, ms, _ = plan["asr1"]
    pool = TextSessionPool(model, 2, 256, ctc_beam=CtcBeamOptions(4))
    recs = _drive(pool, plan, cfg)["asr1"]
    args = RF.agent_args(StreamSpeechASRAgent, ms, sr, extra=("--ctc-beam", "4"))
    agent = RF.set_dicts(StreamSpeechASRAgent(args, model=StreamSpeechModel.from_engine(model)), cfg)
    step, pos, text = sr * ms // 1000, 0, ""
    try:
        while True:
            chunk = pcm[pos:pos + step]
            pos += step
            fin = pos >= len(pcm)
            o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=fin))
            text += "" if o.is_empty else o.content
            if fin:
                break
        assert text == "".join(c or "" for _, c, _ in recs) and text
        assert [h.tokens for h in agent.nbest] == [h.tokens for h in pool.nbest(0)]
    finally:
        agent.ctc_stream.close()
        model.encoder_stream_set_tail(0)
