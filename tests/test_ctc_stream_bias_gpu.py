"""The resumable CTC prefix beam search with a hotword set on the GPU (the resumable bias kernels of csrc/ctc_beam.hip, the object of
csrc/ctc_stream.hip).  The checks of tests/test_ctc_stream_bias_cpu.py again through ss_op_ctc_stream_advance, where the oracle
is the one-shot search on the same device (ss_op_ctc_beam_bias, which tests/test_ctc_beam_bias_gpu.py pins to the host twin and
the reference) and every comparison is memcmp of records and owned tokens; the host twin on the same calls (its row log-sums
come from another expf, so the comparison with it is of label strings and stable prefixes); then a TextSessionPool and the ASR
agent with hotwords on the seeded synthetic checkpoint against batch_ctc_beam(bias=) on the rows their last advance saw."""
import numpy as np
import pytest
import torch

from tests.test_ctc_beam_bias_cpu import LM_W
from tests.test_ctc_beam_cpu import PAD, SHAPES, UNK, small_case
from tests.test_ctc_stream_bias_cpu import BiasStream, check_every_split, check_sessions_in_one_call, check_slot_reuse

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


@pytest.fixture(scope="module")
def objs(lib):
    from streamspeech_amd.hotwords import CtcBias
    from streamspeech_amd.ngram import NgramLM
    from tests.test_ctc_beam_bias_cpu import small_set
    from tests.test_ctc_beam_lm_cpu import small_lm
    out = {V: (CtcBias(*small_set(V), V, PAD, UNK), NgramLM(small_lm(V)[0])) for V in sorted({s[1] for s in SHAPES})}
    yield out
    for b, lm in out.values():
        b.close()
        lm.close()


def test_op_every_split_is_the_one_shot_kernel(lib, objs):
    n = check_every_split(lib, objs, gpu=True, seeds=range(2))
    print(f"ctc_stream bias op: {n} streams, every call memcmp-equal to ss_op_ctc_beam_bias")


@pytest.mark.parametrize("with_lm", [False, True])
def test_op_three_sessions_in_one_call_and_the_host_twin(lib, objs, with_lm):
    """Three sessions with different splits in every call: memcmp-equal to the one-shot kernel on each session's frames so far,
    and the host twin on the same calls finds the same label strings, stable prefixes and beam sizes."""
    check_sessions_in_one_call(lib, objs, with_lm, gpu=True)
    shape = SHAPES[2]
    T, V, beam, cand = shape
    bias, lm = objs[V]
    lh, lo = (lm.h, (LM_W[0], LM_W[1], 1)) if with_lm else (None, None)
    xs = [small_case(shape, 6, 50), small_case(shape, 2, 51)[:23], small_case(shape, 6, 52)[:1]]
    upto = [[9, 9, 40], [1, 20, 23], [1, 1, 1]]
    got = {}
    for gpu in (True, False):
        with BiasStream(lib, V, PAD, UNK, 4, T, beam, cand, 5, bias.h, (1.0, 1), lh, lo, gpu=gpu) as st:
            f = [0, 0, 0]
            for j in range(3):
                rc, recs = st.advance([3, 0, 2], [xs[k][f[k]:upto[k][j]] for k in range(3)], [upto[k][j] for k in range(3)], [j == 2] * 3)
                assert rc == 0
                got[(gpu, j)] = [(r["labels"], r["part"], r["status"]) for r in recs]
                f = [upto[k][j] for k in range(3)]
    for j in range(3):
        assert got[(True, j)] == got[(False, j)], j


def test_op_slot_reuse(lib, objs):
    check_slot_reuse(lib, objs, False, gpu=True)
    check_slot_reuse(lib, objs, True, gpu=True)


# ---- the session pool and the agent ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _hotwords(model, plan, cfg):
    """A set over source_unigram that bears on these sessions: bigrams of the plain search's final best hypotheses."""
    from streamspeech_amd.text_policy import CtcBeamOptions
    from streamspeech_amd.text_pool import TextSessionPool
    from tests.test_ctc_beam_bias_gpu import phrases_from
    from tests.test_text_pool_gpu import _drive
    pool = TextSessionPool(model, 8, 256, ctc_beam=CtcBeamOptions(4))
    _drive(pool, plan, cfg)
    phrases = []
    for sid in range(len(plan)):
        for p in phrases_from(pool.nbest(sid), 2):
            if p not in phrases:
                phrases.append(p)
    assert phrases
    return phrases


def test_pool_and_agent_with_hotwords(model, synth_weights, tmp_path):
    """A TextSessionPool(ctc_beam=CtcBeamOptions(4, bias=...)) with two ASR sessions: every session's writes add up to the
    " ".join of the final best hypothesis of batch_ctc_beam(bias=) on the rows its last advance saw, nbest(sid) is that call's
    list, and some best hypothesis earned credit.  The ASR agent with --ctc-beam 4 --ctc-hotwords FILE on the same audio writes
    what the pool's session writes."""
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    from streamspeech_amd.engine import CtcBiasHypothesis, ctc_beam_default_cand
    from streamspeech_amd.hotwords import CtcBias
    from streamspeech_amd.modules import Dictionary, StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_policy import CtcBeamOptions
    from streamspeech_amd.text_pool import TextSessionPool
    from tests import ref_fixtures as RF
    from tests.test_ctc_stream_gpu import _pool_plan
    from tests.test_text_pool_gpu import _drive
    cfg = synth_weights[0]
    plan = {k: v for k, v in _pool_plan().items() if k in ("asr0", "asr1")}
    phrases = _hotwords(model, plan, cfg)
    with CtcBias(phrases, 2.0, model.cfg.src_vocab, model.cfg.pad, model.cfg.unk) as bias:
        pool = TextSessionPool(model, 8, 256, ctc_beam=CtcBeamOptions(4, bias=bias, bias_scale=1.0))
        finals, advance = {}, pool.ctc_stream.advance

        def spy(slots, enc_packed, T, upto, final):
            got = advance(slots, enc_packed, T, upto, final)
            sid_of = {s.slot: sid for sid, s in pool.sessions.items() if s.slot is not None}
            off = 0
            for sl, t, fin, p in zip(slots, T, final, got):
                if fin:
                    ref = model.batch_ctc_beam(0, enc_packed[off:off + t].contiguous(), [t], 4, ctc_beam_default_cand(4), 4, bias=bias,
                                               bias_scale=1.0)[0]
                    assert p.hyps == ref and all(type(h) is CtcBiasHypothesis for h in p.hyps), sid_of[sl]
                    finals[sid_of[sl]] = ref
                off += t
            return got

        pool.ctc_stream.advance = spy
        got = _drive(pool, plan, cfg)
        d = RF.dictionaries(cfg)
        texts = {}
        for sid, name in enumerate(plan):
            best = finals[sid][0]
            texts[name] = "".join(c or "" for _, c, _ in got[name])
            assert texts[name] == " ".join(d["source_unigram"][c] for c in best.tokens), name
            assert pool.nbest(sid) == finals[sid]
        assert any(finals[sid][0].bias_score > 0 for sid in finals)
    # ---- the agent: the same set, read from a file over the agent's own dictionary ----
    ph = Dictionary.placeholder(model.cfg.src_vocab)
    hot = tmp_path / "hot.txt"
    hot.write_text("".join(" ".join(ph[c] for c in p) + "\n" for p in phrases), encoding="utf-8")
    kind, _, pcm, sr, ms, _ = plan["asr1"]
    args = RF.agent_args(StreamSpeechASRAgent, ms, sr, extra=("--ctc-beam", "4", "--ctc-hotwords", str(hot), "--ctc-hotword-boost", "2.0"))
    agent = RF.set_dicts(StreamSpeechASRAgent(args, model=StreamSpeechModel.from_engine(model)), cfg)
    step, pos, text = sr * ms // 1000, 0, ""
    try:
        assert agent.ctc_stream.bias.n_phrases == len(phrases)
        while True:
            chunk = pcm[pos:pos + step]
            pos += step
            fin = pos >= len(pcm)
            o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=fin))
            text += "" if o.is_empty else o.content
            if fin:
                break
        assert text == texts["asr1"] and text
        assert [(h.tokens, h.bias_score) for h in agent.nbest] == [(h.tokens, h.bias_score) for h in finals[1]]
    finally:
        agent.ctc_stream.close()
        agent.ctc_stream.bias.close()
        model.encoder_stream_set_tail(0)
