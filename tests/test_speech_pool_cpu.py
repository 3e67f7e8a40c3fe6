"""Host side of the concurrent S2ST sessions (streamspeech_amd/speech_pool.py): the S2ST gate against the agent's own arithmetic, the
whole-word cut, the vocoder context rule, and the pool's refusals and host decisions with a stub engine.  No GPU."""
import argparse

import pytest

from streamspeech_amd.speech_pool import KINDS, SpeechSessionPool, vocoder_context, whole_word_cut
from streamspeech_amd.text_policy import s2tt_gate


def _agent_gate(ns, nt, src, tgt, committed, k1, n, finished, whole_word):
    """StreamSpeechS2STAgent.policy's gate as agent.py writes it."""
    if finished:
        return True, src, tgt, -1
    if ns < src + n or nt < tgt + n:
        return False, src, tgt, None
    src, tgt = max(ns, src), max(nt, tgt)
    sub = ((nt - k1) // n) * n
    if whole_word:
        sub += 1
    new = sub - committed
    return new >= 1, src, tgt, new


@pytest.mark.parametrize("whole_word", [False, True])
@pytest.mark.parametrize("case", [
    (0, 0, 0, 0, 0, 0, 1, False), (3, 2, 0, 0, 0, 0, 1, False), (3, 2, 3, 2, 2, 0, 1, False), (5, 4, 3, 2, 2, 0, 1, False),
    (5, 4, 3, 2, 3, 3, 1, False), (6, 6, 3, 3, 2, 1, 2, False), (7, 7, 3, 3, 4, 1, 2, False), (9, 9, 6, 6, 4, 0, 3, False),
    (4, 1, 4, 1, 1, 0, 1, True), (1, 9, 0, 0, 0, 2, 1, False), (9, 1, 0, 0, 0, 0, 1, False), (10, 10, 0, 0, 11, 0, 1, False),
])
def test_s2st_gate_matches_agent_arithmetic(case, whole_word):
    """The pool's S2ST gate: the S2TT gate with one committed subword fewer in whole-word mode."""
    ns, nt, src, tgt, committed, k1, n, fin = case
    g = s2tt_gate(ns, nt, src, tgt, committed - (1 if whole_word else 0), k1, n, fin)
    w, s2, t2, new = _agent_gate(*case, whole_word)
    assert (g.write, g.src_prefix_len, g.tgt_prefix_len) == (w, s2, t2)
    if new is not None:
        assert g.new_tokens == new


def test_whole_word_cut():
    sym = {1: "▁a", 2: "b", 3: "▁c", 4: "d"}.get
    assert whole_word_cut([1, 2, 3, 4], sym) == 2
    assert whole_word_cut([1, 2, 4], sym) == 0
    assert whole_word_cut([2, 4], sym) == 0
    assert whole_word_cut([], sym) == 999999
    assert whole_word_cut([3], sym) == 0


def test_vocoder_context_rule():
    class Cfg:
        def receptive_field_frames(self):
            return 20
    assert vocoder_context(Cfg(), -1) == (28, 20)
    assert vocoder_context(Cfg(), 0) == (0, 20)
    assert vocoder_context(Cfg(), 5) == (5, 20)
    assert vocoder_context(None, -1) == (0, None)


class _Cfg:
    max_target_positions, eos, pad, dec_dim, ctc_upsample = 1024, 2, 1, 8, 25


class _StubPool:
    def __init__(self):
        self.resets = []

    def reset(self, slot):
        self.resets.append(slot)

    def set_tail(self, slot, n):
        pass


class _StubEngine:
    """Enough of HipModel for the pool's host side: nothing here may be launched."""
    cfg = _Cfg()
    device = "cpu"

    def stream_pool(self, max_sessions, max_rows):
        return _StubPool()

    def __getattr__(self, k):                          # no launch entry points: any device work fails the test
        raise AttributeError(f"device work in a host-only test: {k}")


def _args(segment_ms=320, **over):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    p = argparse.ArgumentParser()
    StreamSpeechS2STAgent.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0", "--dur-prediction",
                      "--sample-rate", "16000"])
    a.source_segment_size, a.device = segment_ms, "cpu"
    for k, v in over.items():
        setattr(a, k, v)
    return a


class _Voc:
    class cfg:
        @staticmethod
        def receptive_field_frames():
            return 20


def _dicts():
    from streamspeech_amd.modules import Dictionary
    syms = [("" if i % 3 == 0 else "▁") + f"t{i}" for i in range(40)]
    return {"tgt": Dictionary.units(1000), "target_unigram": Dictionary(syms), "source_unigram": Dictionary(syms),
            "ctc_target_unigram": Dictionary(syms)}


def test_open_refusals():
    assert "s2st" in KINDS and "s2tt" in KINDS and "asr" in KINDS
    with pytest.raises(ValueError):
        SpeechSessionPool(_StubEngine(), 2, 64).open("s2st", _args(), dicts=_dicts())
    pool = SpeechSessionPool(_StubEngine(), 2, 64, vocoder=_Voc())
    with pytest.raises(ValueError):
        pool.open("s2st", _args(full_recompute_encoder=True), dicts=_dicts())
    with pytest.raises(ValueError):
        pool.open("tts", _args(), dicts=_dicts())
    assert pool.sessions == {}
    sid = pool.open("s2st", _args(960), dicts=_dicts())
    s = pool.sessions[sid]
    assert s.whole_word and s.vocoder_ctx == 28 and s.vocoder_rf == 20


def test_capacity_refusal_changes_nothing():
    from streamspeech_amd.simuleval_shim import SpeechSegment
    pool = SpeechSessionPool(_StubEngine(), 2, 16, vocoder=_Voc())
    a, b = pool.open("s2st", _args(), dicts=_dicts()), pool.open("s2st", _args(), dicts=_dicts())
    ok = SpeechSegment(content=[0.0] * 5120, sample_rate=16000, finished=False)
    big = SpeechSegment(content=[0.0] * 16000, sample_rate=16000, finished=False)       # 25 encoder rows > 16
    with pytest.raises(ValueError):
        pool.step({a: ok, b: big})
    assert all(len(s.states.source) == 0 and not s.pending for s in pool.sessions.values())
    assert len(pool.free) == 2


def test_host_decisions_of_a_write():
    """_mt_decide: the whole-word cut of a non-final hypothesis, the trailing <pad> of a final whole-word write, and both
    'nothing new' reads."""
    pool = SpeechSessionPool(_StubEngine(), 2, 64, vocoder=_Voc())
    d = _dicts()
    ww = pool.sessions[pool.open("s2st", _args(960), dicts=d)]
    # ids 0-3 are the special symbols: id k is "t{k-4}", word-initial unless k - 4 is a multiple of 3 (5, 6, 8, 9 start words)
    a, n, pad = pool._mt_decide(ww, [5, 7, 6, 7])        # cut before the last word start (index 2)
    assert a is None and n == 2 and pad == 0 and ww.tgt_subwords == [5, 7] and ww.prev_output_tokens_mt == [2, 5, 7]
    a, _, _ = pool._mt_decide(ww, [5, 7, 6, 7])          # same committed subwords: READ
    assert a == ("read",)
    a, _, _ = pool._mt_decide(ww, [5, 7])                # only the first subword starts a word: j == 0, READ
    assert a == ("read",)
    ww.states.source_finished = True
    a, n, pad = pool._mt_decide(ww, [5, 7, 6, 7, 2])     # final: eos kept, one trailing <pad>
    assert a is None and n == 4 and pad == 1 and ww.prev_output_tokens_mt == [2, 5, 7, 6, 7, 1]
    a, _, _ = pool._mt_decide(ww, [5, 7, 6, 7, 2])       # nothing new at the end: the agent's empty final write
    assert a == ("speech", [], True, False)
    plain = pool.sessions[pool.open("s2st", _args(320), dicts=d)]
    a, n, pad = pool._mt_decide(plain, [5, 7, 9, 2])
    assert a is None and n == 3 and pad == 0 and plain.prev_output_tokens_mt == [2, 5, 7, 9]
    a, _, _ = pool._mt_decide(plain, [5, 9, 2])          # other subwords, but prev_output_tokens_mt no longer: READ
    assert a == ("read",) and plain.tgt_subwords == [5, 9]
