"""Words in the output speech without a device: words.spoken_from_segments (grouping, words over two writes, words without
units, pending states, the tail, the sum), words.segments_from_spans, and the playback mapping of
streaming_eval.run_utterance(spoken=True) on a scripted agent with a hand-made .spoken."""
import numpy as np
import pytest

from streamspeech_amd import streaming_eval as E
from streamspeech_amd.simuleval_shim import EmptySegment, SpeechSegment
from streamspeech_amd.words import Spoken, SpokenWord, segments_from_spans, spoken_from_segments

#            0      1      2       3      4      5      6
SYM = ["<s>", "<pad>", "</s>", "<unk>", "▁he", "llo", "▁big", "▁wor", "ld", "▁x"]
EOS = 2


def test_a_word_split_over_two_writes_and_the_sum():
    toks = [4, 5, 6]                      # "hello big"
    segs = [(0, 0, 60, 3), (1, 60, 100, 2),                 # write 1: ▁he, llo
            (1, 100, 140, 1), (2, 140, 200, 2), (3, 200, 260, 3)]   # write 2: more of llo, ▁big, and the state that predicts </s>
    sp = spoken_from_segments(toks, segs, SYM, eos=EOS)
    assert sp.words == [SpokenWord("hello", 0, 140, 6), SpokenWord("big", 140, 200, 2)]
    assert sp.tail_ms == 60 and sp.total_ms == 260
    assert sp.total_ms == sum(b - a for _, a, b, _ in segs)
    assert sum(w.end_ms - w.start_ms for w in sp.words) + sp.tail_ms == sp.total_ms


def test_a_word_without_units_is_zero_length_at_its_first_tokens_state():
    toks = [4, 5, 6, 7, 8]                # hello | big | world
    segs = [(0, 0, 40, 2), (1, 40, 100, 1), (2, 100, 100, 0), (3, 100, 180, 4), (4, 180, 180, 0), (5, 180, 200, 1)]
    sp = spoken_from_segments(toks, segs, SYM, eos=EOS)
    assert [w.text for w in sp.words] == ["hello", "big", "world"]
    assert sp.words[1] == SpokenWord("big", 100, 100, 0)
    assert sp.words[2] == SpokenWord("world", 100, 180, 4)          # ld's zero-length marker does not stretch the word
    assert sp.tail_ms == 20 and sp.total_ms == 200
    # the marker of the write that first saw the state wins over a later write's
    sp = spoken_from_segments([4, 6], [(0, 0, 40, 1), (1, 40, 40, 0), (2, 40, 40, 0), (1, 300, 300, 0)], SYM, eos=EOS)
    assert sp.words[1] == SpokenWord("big", 40, 40, 0)


def test_a_pending_state_becomes_a_token():
    write1 = [(0, 0, 60, 2), (1, 60, 120, 3)]     # tokens [▁he]; state 1 predicts the next, not yet committed token
    sp = spoken_from_segments([4], write1, SYM, eos=EOS)
    assert sp.words == [SpokenWord("he", 0, 60, 2)] and sp.tail_ms == 60 and sp.total_ms == 120
    write2 = write1 + [(1, 120, 160, 1), (2, 160, 200, 2)]   # now [▁he, ▁big]: state 1's earlier speech counts for ▁big
    sp = spoken_from_segments([4, 6], write2, SYM, eos=EOS)
    assert sp.words == [SpokenWord("he", 0, 60, 2), SpokenWord("big", 60, 160, 4)]
    assert sp.tail_ms == 40 and sp.total_ms == 200


def test_the_tail_eos_token_pad_state_and_carried_audio():
    toks = [4, 5, EOS]                    # a hypothesis that still carries its </s>
    segs = [(-1, 0, 20, 0), (0, 20, 60, 2), (1, 60, 80, 1), (2, 80, 120, 2), (3, 120, 140, 1)]
    sp = spoken_from_segments(toks, segs, SYM, eos=EOS)
    assert sp.words == [SpokenWord("hello", 20, 80, 3)]
    assert sp.tail_ms == 20 + 40 + 20 and sp.total_ms == 140
    assert spoken_from_segments(toks, segs, SYM) == sp              # eos by its symbol
    assert spoken_from_segments([], [], SYM, eos=EOS) == Spoken([], 0, 0)
    with pytest.raises(ValueError):
        spoken_from_segments([4], [(0, 40, 20, 1)], SYM, eos=EOS)


def test_segments_from_spans():
    spans = np.array([[3, 0, 0, 0], [3, 2, 0, 5], [5, 0, 5, 0], [5, 1, 5, 2]], dtype=np.int32)
    assert segments_from_spans(spans, 100) == [(0, 100, 100, 0), (1, 100, 200, 2), (2, 200, 200, 0), (3, 200, 240, 1)]
    assert segments_from_spans(spans, 100, n_seen=3) == [(1, 100, 200, 2), (3, 200, 240, 1)]


# ---- playback -----------------------------------------------------------------------------------------------------------------------
class Scripted:
    """Answers the scripted number of samples per pushpop (0: a read) and carries a hand-made .spoken."""

    def __init__(self, script, spoken):
        self.script, self.spoken, self.k = list(script), spoken, 0

    def pushpop(self, seg):
        n = self.script[self.k]
        self.k += 1
        if n == 0:
            return EmptySegment()
        return SpeechSegment(content=[0.0] * n, sample_rate=16000, finished=seg.finished)


def test_playback_on_a_write_edge_and_across_a_gap():
    # 5 chunks of 320 ms; writes after chunk 2 (400 ms of speech), chunk 3 (200 ms) and chunk 5 (300 ms):
    #   write 0: delay 640, plays 640 .. 1040, emitted 0 .. 400
    #   write 1: delay 960, starts at max(1040, 960) = 1040, plays 1040 .. 1240, emitted 400 .. 600 (no gap)
    #   write 2: delay 1600, plays 1600 .. 1900, emitted 600 .. 900 (a gap of 360 ms before it)
    spoken = Spoken([SpokenWord("a", 0, 400, 5),          # ends exactly on the edge of write 0: belongs to it
                     SpokenWord("b", 400, 600, 3),        # starts exactly on that edge: the later write; ends on the next edge: the earlier
                     SpokenWord("c", 600, 600, 0),        # zero length on the edge before the gap: starts after the gap, ended before it
                     SpokenWord("d", 620, 900, 4)], 0, 900)
    agent = Scripted([0, 6400, 3200, 0, 4800], spoken)
    r = E.run_utterance(agent, np.zeros(5 * 5120, dtype=np.float32), sync=False, spoken=True)
    assert r["writes"] == 3 and r["samples_out"] == 14400
    got = [(w["text"], w["play_start_ms"], w["play_end_ms"]) for w in r["spoken_words"]]
    assert got == [("a", 640.0, 1040.0), ("b", 1040.0, 1240.0), ("c", 1600.0, 1240.0), ("d", 1620.0, 1900.0)]
    bow, eow = [g[1] for g in got], [g[2] for g in got]
    assert r["SpeechAlign"]["BOW"] == E.speech_align_latency(bow, 1600.0)
    assert r["SpeechAlign"]["EOW"] == E.speech_align_latency(eow, 1600.0)
    assert r["SpeechAlign"]["COW"] == E.speech_align_latency([(a + b) / 2 for a, b in zip(bow, eow)], 1600.0)
    assert sorted(r["SpeechAlign"]["BOW"]) == ["AL", "AP", "DAL", "LAAL"]


def test_playback_ms_directly():
    writes = [(0.0, 640.0, 400.0), (400.0, 1040.0, 200.0), (600.0, 1600.0, 300.0)]
    assert E.playback_ms(0, writes, True) == 640.0 and E.playback_ms(0, writes, False) == 640.0
    assert E.playback_ms(900, writes, False) == 1900.0 and E.playback_ms(900, writes, True) == 1900.0
    assert E.playback_ms(600, writes, True) == 1600.0 and E.playback_ms(600, writes, False) == 1240.0
    assert E.playback_ms(610, writes, True) == E.playback_ms(610, writes, False) == 1610.0


def test_without_the_keyword_the_result_is_todays():
    keys = {"source_ms", "compute_ms", "calls", "call_ms", "actions", "writes", "samples_out", "RTF", "RTF_CA", "StartOffset",
            "StartOffset_CA", "EndOffset", "EndOffset_CA"}
    spoken = Spoken([SpokenWord("a", 0, 400, 5)], 0, 400)
    pcm = np.zeros(2 * 5120, dtype=np.float32)
    r = E.run_utterance(Scripted([0, 6400], spoken), pcm, sync=False)
    assert set(r) == keys
    r = E.run_utterance(Scripted([0, 6400], spoken), pcm, sync=False, spoken=True)
    assert set(r) == keys | {"spoken_words", "SpeechAlign"}
    no_attr = Scripted([0, 6400], None)
    del no_attr.spoken
    assert set(E.run_utterance(no_attr, pcm, sync=False, spoken=True)) == keys       # an agent without .spoken: today's dict
    r = E.run_utterance(Scripted([0, 0], Spoken([], 0, 0)), pcm, sync=False, spoken=True)
    assert r["spoken_words"] == [] and r["SpeechAlign"] == {"BOW": None, "COW": None, "EOW": None}
