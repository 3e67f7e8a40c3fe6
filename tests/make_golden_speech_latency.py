"""Writes tests/golden/speech_align_latency.json: AL / LAAL / AP / DAL of hand-made per-word delay lists as the reference's own
scorer classes compute them (SimulEval scorers/latency_scorer.py, loaded where they lie as oracle/ref_simuleval.py loads them).
Only the recorded numbers are committed.  Run from the repository root: python -m tests.make_golden_speech_latency"""
import json
import os
import types

CASES = [
    # name, delays (ms), source length (ms), reference length or None
    ("first_delay_past_source", [5200.0, 5600.0, 6100.0], 5000.0, None),
    ("first_delay_past_source_with_ref", [5200.0, 5600.0, 6100.0], 5000.0, 5),
    ("early_cut", [800.0, 1500.0, 2600.0, 4000.0, 4300.0, 4700.0], 4000.0, None),
    ("early_cut_with_ref", [800.0, 1500.0, 2600.0, 4000.0, 4300.0, 4700.0], 4000.0, 4),
    ("no_cut", [320.0, 960.0, 1280.0, 2240.0, 2560.0], 3333.0, None),
    ("more_words_than_ref", [320.0, 960.0, 1280.0, 2240.0, 2560.0, 3100.5, 3480.25], 3333.0, 4),
    ("fewer_words_than_ref", [320.0, 960.0, 1280.0, 2240.0], 3333.0, 9),
    ("as_many_words_as_ref", [640.0, 640.0, 1920.0], 2000.0, 3),
    ("one_word", [1234.5], 2000.0, None),
    ("one_word_with_ref", [1234.5], 2000.0, 3),
    ("one_word_past_source", [2100.0], 2000.0, None),
    ("equal_delays", [960.0, 960.0, 960.0, 960.0], 1280.0, None),
    ("centres", [(320.0 + 700.0) / 2, (700.0 + 1330.0) / 2, (1330.0 + 2111.0) / 2], 1777.0, 2),
]


def main():
    from oracle import ref_simuleval
    assert ref_simuleval.available(), "the reference's SimulEval tree is not here"
    _, sc = ref_simuleval.load()
    scorers = {"AL": sc.ALScorer(), "LAAL": sc.LAALScorer(), "AP": sc.APScorer(), "DAL": sc.DALScorer()}
    out = []
    for name, delays, src, ref_len in CASES:
        ins = types.SimpleNamespace(delays=list(delays), elapsed=list(delays), source_length=src,
                                    reference=None if ref_len is None else "x", reference_length=ref_len)
        out.append({"name": name, "delays_ms": delays, "source_ms": src, "ref_len": ref_len,
                    "want": {k: float(s.compute(ins)) for k, s in scorers.items()}})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speech_align_latency.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"wrote {len(out)} cases to {path}")


if __name__ == "__main__":
    main()
