"""The offline driver's --align-reference on a temporary data root: the synthetic checkpoint, placeholder dictionaries, a three-row
manifest and the two multitask manifests (source_unigram, ctc_target_unigram), each lacking one row."""
import math
import os
import wave

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SECONDS = (1.0, 1.7, 1.2)


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def _data_root(tmp_path):
    from streamspeech_amd import synth
    data = tmp_path / "data"
    data.mkdir()
    with open(data / "test.tsv", "w") as f:
        f.write("id\tsrc_audio\tsrc_n_frames\n")
        for k, sec in enumerate(SECONDS):
            x = np.clip(synth.synth_pcm(900 + k, int(16000 * sec)) * 32768.0, -32768, 32767).astype(np.int16)
            with wave.open(str(data / f"utt{k}.wav"), "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                w.writeframes(x.tobytes())
            f.write(f"utt{k}\t{data / f'utt{k}.wav'}\t{len(x)}\n")
    piece = lambda i: f"▁w{i}"  # noqa: E731
    (data / "source_unigram").mkdir()
    (data / "source_unigram" / "test.tsv").write_text(                      # utt1 has no source reference; utt2's cannot fit
        "id\ttgt_text\nutt0\t%s\nutt2\t%s\n" % (" ".join(piece(i) for i in (5, 9, 9, 30)), " ".join(piece(7 + i % 2) for i in range(60))),
        encoding="utf-8")
    (data / "ctc_target_unigram").mkdir()
    (data / "ctc_target_unigram" / "test.tsv").write_text(                  # utt2 has no target reference; one piece is unknown
        "id\ttgt_text\nutt0\t%s\nutt1\t%s not▁in▁the▁dictionary %s\n" % (" ".join(piece(i) for i in (11, 12)), piece(40), piece(41)),
        encoding="utf-8")
    (data / "mt.yaml").write_text(
        "source_unigram:\n  decoder_type: ctc\n  data: /another/machine/data/source_unigram\n"
        "ctc_target_unigram:\n  decoder_type: ctc\n  data: %s\n" % (data / "ctc_target_unigram"))
    return data


def test_align_reference_writes_its_files_and_changes_no_other(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import offline
    data = _data_root(tmp_path)
    common = [str(data), "--path", "synthetic:0", "--vocoder", "synthetic:0", "--device", "cuda:0", "--multitask-config-yaml", "mt.yaml",
              "--dur-prediction", "--batch-size", "2", "--word-times"]
    offline.main(common + ["--results-path", str(tmp_path / "plain")])
    offline.main(common + ["--results-path", str(tmp_path / "ref"), "--align-reference"])
    a, b = _tree(tmp_path / "plain"), _tree(tmp_path / "ref")
    new = {"generate-test.asr.ref.words", "generate-test.st.ref.words", "generate-test.ref.scores"}
    assert set(b) - set(a) == new and set(a) <= set(b) and "generate-test.asr.words" in a
    for k in a:
        assert a[k] == b[k], f"{k} differs with --align-reference"
    rows = [ln.split("\t") for ln in b["generate-test.ref.scores"].decode().splitlines()]
    assert [(r[0], r[1]) for r in rows] == [(str(i), h) for i in range(3) for h in ("asr", "st")] and all(len(r) == 6 for r in rows)
    got = {(int(r[0]), r[1]): (int(r[2]), float(r[3]), float(r[4]), r[5]) for r in rows}
    assert [got[k][3] for k in sorted(got)] == ["aligned", "aligned", "no_reference", "aligned", "infeasible", "no_reference"]
    assert [got[k][0] for k in sorted(got)] == [4, 2, 0, 3, 60, 0]
    for k, (n, score, vit, status) in got.items():
        if status == "aligned":
            assert math.isfinite(score) and score >= vit - 1e-6 and vit < 0
        elif status == "infeasible":
            assert score == -math.inf and vit == -math.inf
        else:
            assert math.isnan(score) and math.isnan(vit)
    want_words = {"asr": {0: ["w5", "w9", "w9", "w30"]}, "st": {0: ["w11", "w12"], 1: ["w40<unk>", "w41"]}}
    for key in ("asr", "st"):
        lines = [ln.split("\t") for ln in b[f"generate-test.{key}.ref.words"].decode().splitlines()]
        assert all(len(ln) == 5 for ln in lines)
        by_id = {}
        for sid, word, start, end, conf in lines:
            by_id.setdefault(int(sid), []).append((word, int(start), int(end), float(conf)))
        assert {i: [w[0] for w in ws] for i, ws in by_id.items()} == want_words[key]
        for i, ws in by_id.items():
            clip_ms = 40 * math.ceil(SECONDS[i] * 1000 / 40)        # the clip in whole 40-ms encoder frames
            prev = 0
            for _, start, end, conf in ws:
                assert prev <= start < end <= clip_ms and start % 40 == 0 and end % 40 == 0
                assert 0.0 < conf <= 1.0
                prev = end
