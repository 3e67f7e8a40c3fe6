"""streaming_eval.speech_align_latency against numbers recorded from the reference's own AL / LAAL / AP / DAL scorer classes
(tests/golden/speech_align_latency.json, made by tests/make_golden_speech_latency.py): the same float64 operations in the same order,
so equality holds to 1e-9 relative."""
import json
import os

import pytest

from streamspeech_amd.streaming_eval import speech_align_latency

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "speech_align_latency.json"), encoding="utf-8") as _f:
    GOLDEN = json.load(_f)


def test_the_golden_holds_the_issues_cases():
    by = {c["name"]: c for c in GOLDEN}
    assert by["first_delay_past_source"]["delays_ms"][0] > by["first_delay_past_source"]["source_ms"]
    c = by["early_cut"]
    assert any(d >= c["source_ms"] for d in c["delays_ms"][:-1])
    assert len(by["more_words_than_ref"]["delays_ms"]) > by["more_words_than_ref"]["ref_len"]
    assert len(by["fewer_words_than_ref"]["delays_ms"]) < by["fewer_words_than_ref"]["ref_len"]
    assert len(by["one_word"]["delays_ms"]) == 1 and by["one_word"]["ref_len"] is None
    assert any(c["ref_len"] is None for c in GOLDEN) and any(c["ref_len"] is not None for c in GOLDEN)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_against_the_reference_scorers(case):
    got = speech_align_latency(case["delays_ms"], case["source_ms"], case["ref_len"])
    assert sorted(got) == ["AL", "AP", "DAL", "LAAL"]
    for k, want in case["want"].items():
        assert abs(got[k] - want) <= 1e-9 * max(abs(want), 1e-300), (k, got[k], want)


def test_refusals():
    with pytest.raises(ValueError):
        speech_align_latency([], 1000.0)
    with pytest.raises(ValueError):
        speech_align_latency([1.0], 0.0)
