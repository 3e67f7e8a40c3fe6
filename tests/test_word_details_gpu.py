"""Word time spans and confidences end to end on the GPU: TextSessionPool(details=True) answers the segments of a pool without
details and words that are consistent with them; the ASR agent's --word-details gives the words of a one-session pool; the offline
driver's --word-times writes the two word files and changes no other file."""
import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _args(kind, segment_ms, sr, over=None, extra=()):
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    cls = StreamSpeechS2TTAgent if kind == "s2tt" else StreamSpeechASRAgent
    return cls, RF.agent_args(cls, segment_ms, sr, over, extra)


def _detok_words(symbols):
    return "".join(symbols).replace("▁", " ").split()


def _check_words(words, received_ms, what):
    prev_end = 0
    for w in words:
        assert 0 <= w.start_ms < w.end_ms <= received_ms, (what, w, received_ms)
        assert w.start_ms >= prev_end, (what, w)
        assert 0.0 < w.confidence <= 1.0, (what, w)
        prev_end = w.end_ms


def test_pool_details(model, synth_weights):
    from streamspeech_amd import synth
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    d = RF.dictionaries(cfg)
    spec = [("asr", 320, 16000, 2.1), ("s2tt", 640, 16000, 2.9), ("asr", 960, 48000, 3.0), ("s2tt", 320, 16000, 1.4)]
    pools = [TextSessionPool(model, 4, 128, details=True), TextSessionPool(model, 4, 128)]
    src_tokens = {}
    orig = pools[0]._asr
    pools[0]._asr = lambda s, tokens: (src_tokens.__setitem__(s.sid, list(tokens)), orig(s, tokens))[1]
    sess = []
    for k, (kind, ms, sr, secs) in enumerate(spec):
        pcm = synth.synth_pcm(500 + k, int(16000 * secs))
        if sr != 16000:
            pcm = np.repeat(pcm, sr // 16000)
        _, args = _args(kind, ms, sr)
        sess.append({"kind": kind, "sr": sr, "step": sr * ms // 1000, "pcm": pcm, "pos": 0, "stable": {},
                     "sid": [p.open(kind, args, dicts=d) for p in pools]})
    assert pools[0].details(sess[0]["sid"][0]) is None
    live = list(range(len(sess)))
    while live:
        segs = [{}, {}]
        for k in live:
            s = sess[k]
            chunk = s["pcm"][s["pos"]:s["pos"] + s["step"]]
            s["pos"] += s["step"]
            s["fin"] = s["pos"] >= len(s["pcm"])
            for j in (0, 1):
                segs[j][s["sid"][j]] = SpeechSegment(content=chunk.tolist(), sample_rate=s["sr"], finished=s["fin"])
        outs = [p.step(g) for p, g in zip(pools, segs)]
        assert pools[0].last_step["ctc_scored"] == (1 if pools[0].last_step["encoded"] else 0)
        assert pools[1].last_step["ctc_scored"] == 0
        for k in list(live):
            s = sess[k]
            a, b = outs[0][s["sid"][0]], outs[1][s["sid"][1]]
            assert (a.is_empty, None if a.is_empty else a.content, bool(a.finished)) == \
                   (b.is_empty, None if b.is_empty else b.content, bool(b.finished)), k
            assert pools[1].details(s["sid"][1]) is None
            det = pools[0].details(s["sid"][0])
            received_ms = min(s["pos"], len(s["pcm"])) * 1000 // s["sr"]
            if det is not None:
                for name, words in (("src", det.source_words), ("tgt", det.target_words)):
                    _check_words(words, received_ms, (k, name))
                    held = s["stable"].setdefault(name, {})
                    for i, w in held.items():              # a word once stable: text, span and confidence bitwise, for good
                        assert i < len(words) and words[i] == w, (k, name, i, words[i] if i < len(words) else None, w)
                    for i, w in enumerate(words):
                        assert w.stable in (True, False)
                        if w.stable:
                            held[i] = w
                    if s["fin"]:
                        assert all(w.stable for w in words), (k, name)
                if s["kind"] == "asr" and s["sid"][0] in src_tokens:
                    want = _detok_words([d["source_unigram"][c] for c in src_tokens[s["sid"][0]]])
                    assert [w.text for w in det.source_words] == want, k
            if s["fin"]:
                assert det is not None and (det.source_words or det.target_words), k
                live.remove(k)
    model.encoder_stream_set_tail(0)


def test_asr_agent_word_details_match_a_one_session_pool(model, synth_weights):
    from streamspeech_amd import synth
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    cls, args = _args("asr", 320, 16000, extra=("--word-details",))
    assert args.word_details
    _, plain_args = _args("asr", 320, 16000)
    assert plain_args.word_details is False
    agent = RF.set_dicts(cls(args, model=StreamSpeechModel.from_engine(model)), cfg)
    plain = RF.set_dicts(cls(plain_args, model=StreamSpeechModel.from_engine(model.new_context())), cfg)
    pool = TextSessionPool(model.new_context(), 1, 128, details=True)
    sid = pool.open("asr", args, dicts=RF.dictionaries(cfg))
    pcm = synth.synth_pcm(611, int(16000 * 2.3))
    step, pos, worst, seen = 16000 * 320 // 1000, 0, 0.0, 0
    assert agent.details is None
    while pos < len(pcm):
        chunk = pcm[pos:pos + step]
        pos += step
        seg = dict(content=chunk.tolist(), sample_rate=16000, finished=pos >= len(pcm))
        o = agent.pushpop(SpeechSegment(**seg))
        q = plain.pushpop(SpeechSegment(**seg))
        p = pool.step({sid: SpeechSegment(**seg)})[sid]
        assert plain.details is None
        for other in (q, p):                               # the flag changes nothing the agent answers
            assert (o.is_empty, None if o.is_empty else o.content, bool(o.finished)) == \
                   (other.is_empty, None if other.is_empty else other.content, bool(other.finished))
        da, dp = agent.details, pool.details(sid)
        assert (da is None) == (dp is None)
        if da is None:
            continue
        for wa, wp in ((da.source_words, dp.source_words), (da.target_words, dp.target_words)):
            assert [w[:3] + (w.stable,) for w in wa] == [w[:3] + (w.stable,) for w in wp]
            for x, y in zip(wa, wp):
                worst = max(worst, abs(x.confidence - y.confidence))
                seen += 1
    print(f"agent vs pool: {seen} words, max |confidence difference| = {worst:.3e}")
    # the agent's heads run the single-utterance GEMM, the pool's the pack-invariant one: the same logits to rounding (the suite
    # holds the two encoder paths to 2e-5), and d confidence <= max |d lprob|
    assert seen > 0 and worst < 1e-4
    model.encoder_stream_set_tail(0)


class _VocSurface:
    """CodeHiFiGANVocoderWithDur call surface over the shared fixture handle (as tests/test_speech_pool_gpu.py)."""

    def __init__(self, hv):
        self.hip = hv

    def __call__(self, x, dur_prediction=False):
        from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
        return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)


@pytest.mark.parametrize("kind", ["s2tt", "s2st"])
def test_translation_agents_answer_the_same_with_word_details(model, hip_vocoder, synth_weights, kind):
    """--word-details on the S2TT and S2ST agents: every answer as without the flag, agent.details after each policy() that ran the
    encoder, `stable` None under --full-recompute-encoder."""
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    cfg = synth_weights[0]
    cls = StreamSpeechS2TTAgent if kind == "s2tt" else StreamSpeechS2STAgent
    kw = {"vocoder": _VocSurface(hip_vocoder)} if kind == "s2st" else {}

    def make(extra, ctx, over=None):
        args = RF.agent_args(cls, 320, 16000, over, extra)
        return RF.set_dicts(cls(args, model=StreamSpeechModel.from_engine(ctx), **kw), cfg)

    on, off = make(("--word-details",), model), make((), model.new_context())
    full = make(("--word-details", "--full-recompute-encoder"), model.new_context())
    pcm = synth.synth_pcm(733, int(16000 * 1.9))
    step, pos, n_det = 16000 * 320 // 1000, 0, 0
    while pos < len(pcm):
        chunk = pcm[pos:pos + step]
        pos += step
        fin = pos >= len(pcm)
        outs = [a.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=16000, finished=fin)) for a in (on, off, full)]
        rec = [(o.is_empty, None if o.is_empty else o.content, bool(o.finished)) for o in outs]
        assert rec[0] == rec[1], pos
        assert off.details is None
        if on.details is not None:
            n_det += 1
            words = on.details.source_words + on.details.target_words
            assert all(w.stable in (True, False) and 0.0 < w.confidence <= 1.0 for w in words)
            assert full.details is not None
            fw = full.details.source_words + full.details.target_words
            assert all(w.stable is (True if fin else None) for w in fw)
            if fin:
                assert all(w.stable for w in words)
    assert n_det > 0
    model.encoder_stream_set_tail(0)


def test_offline_word_times(model, hip_vocoder, synth_weights, tmp_path):
    from streamspeech_amd import offline, synth
    cfg = synth_weights[0]
    dicts = RF.dictionaries(cfg)
    secs = [1.3, 2.2, 0.01, 0.9]                           # one utterance too short to decode: no words, its lines as ever
    items = [(20 + i, torch.from_numpy(synth.synth_pcm(80 + i, int(16000 * s))).to(model.device)) for i, s in enumerate(secs)]
    kw = dict(batch_size=2, max_len_a_mt=0.0, max_len_b_mt=6, dur_prediction=True, dump_wav=False)
    offline.generate(model, hip_vocoder, items, dicts, str(tmp_path / "a"), "test", **kw)
    offline.generate(model, hip_vocoder, items, dicts, str(tmp_path / "b"), "test", word_times=True, **kw)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == sorted(names + ["generate-test.asr.words", "generate-test.st.words"])
    for n in names:
        if (tmp_path / "a" / n).is_file():
            assert (tmp_path / "a" / n).read_bytes() == (tmp_path / "b" / n).read_bytes(), n
    log = dict(ln.split("\t", 1) for ln in (tmp_path / "b" / "generate-test.log").read_text().splitlines())
    for ext, tag in ((".asr.words", "A"), (".st.words", "S")):
        per = {}
        for ln in (tmp_path / "b" / f"generate-test{ext}").read_text().splitlines():
            sid, word, a, b, conf = ln.split("\t")
            assert 0 <= int(a) < int(b) and 0.0 < float(conf) <= 1.0
            per.setdefault(int(sid), []).append((word, int(a), int(b)))
        assert 22 not in per
        for sid, ws in per.items():
            assert [w for w, _, _ in ws] == log[f"{tag}-{sid}"].split(), sid     # one line per word of the A- / S- text
            assert all(x[2] <= y[1] for x, y in zip(ws, ws[1:]))
            assert ws[-1][2] <= int(secs[sid - 20] * 1000)
        assert set(per) == {sid for sid in (20, 21, 23) if log[f"{tag}-{sid}"].split()}
