"""CTC forced alignment without a device: tests/ctc_align_ref.py against torch's ctc_loss and against brute-force enumeration, the
library's host twin (ss_ctc_align_host: the kernels' transition code, record layout and refusals) against that reference on every
op case tests/test_ctc_align_gpu.py runs, and the Python layers over it (Dictionary.index, load_multitask_text, CTCDecoder.align ->
words_from_ctc, the driver's refusals, the ABI of the new symbols)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 1


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_align_entry_points_are_declared_and_bound(lib):
    import ctypes as C
    from streamspeech_amd import lib as L
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in (("ss_batch_ctc_align", 13), ("ss_ctc_align_host", 14), ("ss_op_ctc_align", 15)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"
    assert lib.ss_abi_version() == 2
    assert C.sizeof(L.SSCtcAlignResult) == R.RESULT.itemsize == 24
    assert [f[0] for f in L.SSCtcAlignResult._fields_] == list(R.RESULT.names)
    assert "#define SS_CTC_ALIGN_MAX_FRAMES %d" % L.CTC_ALIGN_MAX_FRAMES in header
    assert "#define SS_CTC_ALIGN_MAX_LABELS %d" % L.CTC_ALIGN_MAX_LABELS in header


# ---- the reference against torch and against enumeration ---------------------------------------------------------------------------
def _torch_ctc(lp, y):
    T = lp.shape[0]
    loss = torch.nn.functional.ctc_loss(torch.from_numpy(lp).unsqueeze(1), torch.tensor([y], dtype=torch.long).reshape(1, len(y)),
                                        torch.tensor([T]), torch.tensor([len(y)]), blank=0, reduction="none", zero_infinity=False)
    return -float(loss[0])


@pytest.mark.parametrize("T,y,V", [(37, [4, 4, 7, 9, 9, 9, 2, 5, 5], 12), (1, [], 8), (1, [3], 8), (3, [2, 2], 8), (2, [2, 2], 8),
                                   (64, None, 6000)])
def test_reference_forward_sum_is_torch_ctc_loss(T, y, V):
    rng = np.random.default_rng(T + V)
    if y is None:
        y = R.labels(rng, 20, V, repeats=3)
    lp = R.log_softmax(R.logits(T, T, V), V)
    ref = R.align(lp, y)
    want = _torch_ctc(lp, y)
    if want == -math.inf:
        assert ref["status"] == 1 and ref["score"] == -math.inf and ref["viterbi"] == -math.inf
        return
    assert ref["status"] == 0 and abs(ref["score"] - want) <= 1e-12 * max(1.0, abs(want))
    assert R.collapse(ref["path"]) == list(y)
    assert abs(R.path_score(lp, ref["path"]) - ref["viterbi"]) <= 1e-12 * max(1.0, abs(ref["viterbi"]))
    assert ref["score"] >= ref["viterbi"]


def test_reference_against_every_labelling():
    """(T, V, y) = (5, 4, [1, 1, 2]): all 4^5 labellings, for the sum and for the best path."""
    lp = R.log_softmax(R.logits(9, 5, 4), 4)
    tot, best = R.brute_force(lp, [1, 1, 2])
    ref = R.align(lp, [1, 1, 2])
    assert abs(ref["score"] - tot) < 1e-12 and abs(ref["viterbi"] - best) < 1e-12
    assert abs(R.path_score(lp, ref["path"]) - best) < 1e-12


def test_reference_tie_rule():
    """Uniform rows: every path ties.  The end is the trailing blank; a state's best predecessor is itself whenever it was reachable
    a frame earlier (stay first), so the walk back stays in the trailing blank as long as it can, then advances, then skips."""
    lp = np.full((6, 5), -math.log(5.0))
    ref = R.align(lp, [2, 3])
    assert ref["path"].tolist() == [2, 3, 0, 0, 0, 0] and ref["first"] == [0, 1] and ref["last"] == [0, 1]


# ---- the host twin on the op cases -------------------------------------------------------------------------------------------------
def _run_checked(lib, cases, V, gpu=False):
    rc, recs = R.run(lib, [(x, y) for _, x, y in cases], V, pad=PAD, gpu=gpu)
    assert rc == 0
    return [R.check(rec, x, V, y, name) for rec, (name, x, y) in zip(recs, cases)], recs


@pytest.mark.parametrize("V,ld", [(64, 64), (257, 260), (6000, 6000)])
def test_host_small_cases(lib, V, ld):
    refs, recs = _run_checked(lib, R.small_cases(V, ld), V)
    assert [r["status"] for r in refs] == [0, 0, 0, 1, 0, 0, 0]
    assert recs[4]["path"].tolist() == [5, 0, 5]                 # T = 3, [a, a]: the one path
    assert (recs[5]["path"] != 0).all()                          # T = L: no blank fits
    one = R.run(lib, [(R.small_cases(V, ld)[0][1], [])], V, pad=PAD)[1][0]
    assert one["path"].tolist() == [0] and one["score"] == one["viterbi"]      # L = 0: the all-blank path


def test_host_block_cases(lib):
    for case in R.block_cases():
        V = 6000 if "6000" in case[0] else 257 if "257" in case[0] else 64
        _run_checked(lib, [case], V)


def _ragged(V=64):
    s, b = R.small_cases(V), R.block_cases()
    return [s[6], s[0], b[0], ("empty", R.logits(40, 9, V), []), s[3], s[5], s[1], b[2]]


def test_host_ragged_pack_and_its_invariance(lib):
    pack = _ragged()
    refs, recs = _run_checked(lib, pack, 64)
    assert [r["status"] for r in refs] == [0, 0, 0, 0, 1, 0, 0, 0]
    _, rev = _run_checked(lib, pack[::-1], 64)
    for k, case in enumerate(pack):
        alone = R.run(lib, [case[1:]], 64, pad=PAD)[1][0]
        assert R.same_bits(alone, recs[k]) and R.same_bits(alone, rev[len(pack) - 1 - k]), case[0]


def test_host_nan_row_and_dead_label(lib):
    V = 64
    x = R.logits(50, 30, V)
    y = [7, 9, 9, 12]
    bad = x.copy()
    bad[11, 40] = np.nan                                           # one NaN, in a column no state reads
    dead = x.copy()
    dead[:, 9] = -np.inf                                           # a label whose column is -inf in every frame
    refs, recs = _run_checked(lib, [("before", x, y), ("nan_row", bad, y), ("dead_label", dead, y), ("after", x, y)], V)
    assert [r["status"] for r in refs] == [0, 2, 1, 0]
    assert R.same_bits(recs[0], recs[3])                           # the neighbours are untouched


def test_host_follows_a_constructed_labelling(lib):
    x, y, frames = R.constructed()
    (ref,), (rec,) = _run_checked(lib, [("constructed", x, y)], 64)
    assert rec["path"].tolist() == frames.tolist() == ref["path"].tolist()
    runs = [(t, v) for t, v in enumerate(frames) if v != 0 and (t == 0 or frames[t - 1] != v)]
    assert rec["first"].tolist() == [t for t, _ in runs]


def test_host_without_the_optional_outputs(lib):
    x, y = R.logits(51, 12, 64), [4, 8]
    full = R.run(lib, [(x, y)], 64, pad=PAD)[1][0]
    rc, recs = R.run(lib, [(x, y)], 64, pad=PAD, want_path=False, want_frame=False)
    assert rc == 0 and recs[0]["first"].tolist() == full["first"].tolist() and recs[0]["tok_lprob"].tobytes() == full["tok_lprob"].tobytes()


def refusals(V=64):
    """[(cases, pad)] every one of which is SS_ERR_ARG with nothing written."""
    from streamspeech_amd.lib import CTC_ALIGN_MAX_FRAMES, CTC_ALIGN_MAX_LABELS
    x = R.logits(52, 6, V)
    long_x = np.zeros((CTC_ALIGN_MAX_FRAMES + 1, V), np.float32)
    return [([(x, [0])], PAD), ([(x, [4, PAD])], PAD), ([(x, [-2])], PAD), ([(x, [V])], PAD), ([(x, [4]), (x, [4, 0, 5])], PAD),
            ([(long_x, [4])], PAD), ([(x, [4] * (CTC_ALIGN_MAX_LABELS + 1))], PAD), ([], PAD)]


def test_host_refusals(lib):
    from streamspeech_amd import lib as L
    for cases, pad in refusals():
        if cases:
            assert R.run(lib, cases, 64, pad=pad)[0] == L.SS_ERR_ARG
    import ctypes as C
    x, res = R.logits(53, 4, 64), np.zeros(2, R.RESULT)
    one = (C.c_int32 * 1)
    args = lambda B=1, T=4, n=1: (B, one(T), one(5), one(n))  # noqa: E731
    P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    i32, f32 = np.zeros(8, np.int32), np.zeros(8, np.float32)
    assert lib.ss_ctc_align_host(P(x), 64, 64, PAD, *args(B=0), P(res), P(i32), P(i32), P(i32), P(f32), None) == L.SS_ERR_ARG
    assert lib.ss_ctc_align_host(P(x), 64, 64, PAD, *args(T=0), P(res), P(i32), P(i32), P(i32), P(f32), None) == L.SS_ERR_ARG
    assert lib.ss_ctc_align_host(None, 64, 64, PAD, *args(), P(res), P(i32), P(i32), P(i32), P(f32), None) == L.SS_ERR_ARG
    assert lib.ss_ctc_align_host(P(x), 64, 64, PAD, *args(), None, P(i32), P(i32), P(i32), P(f32), None) == L.SS_ERR_ARG
    assert lib.ss_ctc_align_host(P(x), 64, 64, PAD, *args(), P(res), P(i32), None, P(i32), P(f32), None) == L.SS_ERR_ARG
    assert lib.ss_ctc_align_host(P(x), 63, 64, PAD, *args(), P(res), P(i32), P(i32), P(i32), P(f32), None) == L.SS_ERR_ARG
    assert lib.ss_ctc_align_host(P(x), 64, 64, PAD, *args(), P(res), None, P(i32), P(i32), P(f32), None) == 0       # the path is optional
    assert res["status"][0] == 0 and res["n_tokens"][0] == 1 and not res["status"][1]


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
def test_dictionary_index():
    from streamspeech_amd.modules import Dictionary
    d = Dictionary(["▁he", "llo", "▁wor", "ld", "llo"])
    assert [d.index(s) for s in ("<s>", "<pad>", "</s>", "<unk>", "▁he", "llo", "ld")] == [0, 1, 2, 3, 4, 5, 7]
    assert d.index("nowhere") == d.unk() == 3
    assert all(d.index(d[i]) == i for i in range(8))
    assert Dictionary.placeholder(20).index("▁w5") == 9


def test_load_multitask_text_and_the_path_fallback(tmp_path):
    from streamspeech_amd import offline
    data = tmp_path / "data"
    (data / "source_unigram").mkdir(parents=True)
    (data / "source_unigram" / "test.tsv").write_text('id\ttgt_text\nutt_a\t▁he llo ▁wor ld\nutt_b\t\nutt_c\t▁"quo ted\n', encoding="utf-8")
    (data / "elsewhere").mkdir()
    (data / "elsewhere" / "test.tsv").write_text("id\ttgt_text\nutt_a\t▁w1 ▁w2\n", encoding="utf-8")
    (data / "test.tsv").write_text("id\tsrc_audio\tsrc_n_frames\nutt_a\ta.wav\t1\nutt_b\tb.wav\t1\nutt_z\tz.wav\t1\n")
    (data / "mt.yaml").write_text(
        "source_unigram:\n  decoder_type: ctc\n  data: /a/path/of/another/machine/source_unigram\n"
        "ctc_target_unigram:\n  decoder_type: ctc\n  data: %s\ntarget_unigram:\n  decoder_type: transformer\n" % (data / "elsewhere"))
    text = offline.load_multitask_text(str(data / "source_unigram"), "test")
    assert text == {"utt_a": ["▁he", "llo", "▁wor", "ld"], "utt_b": [], "utt_c": ['▁"quo', "ted"]}
    assert offline.multitask_text_dir(str(data), "mt.yaml", "source_unigram") == str(data / "source_unigram")      # the fallback
    assert offline.multitask_text_dir(str(data), "mt.yaml", "ctc_target_unigram") == str(data / "elsewhere")       # the path as named
    assert offline.multitask_text_dir(str(data), "mt.yaml", "target_unigram") is None
    assert offline.multitask_text_dir(str(data), None, "source_unigram") is None
    from streamspeech_amd.modules import Dictionary
    dicts = {"source_unigram": Dictionary(["▁he", "llo", "▁wor"]), "ctc_target_unigram": Dictionary.placeholder(10)}
    refs = offline.load_references(str(data), "mt.yaml", "test", dicts)
    assert refs == {"asr": {0: [4, 5, 6, 3], 1: []}, "st": {0: [5, 6]}}          # "ld" -> <unk>; utt_z has no reference
    (data / "none.yaml").write_text("source_unigram:\n  decoder_type: ctc\n")
    assert offline.load_references(str(data), "none.yaml", "test", dicts) is None


def test_align_reference_refusals(tmp_path, capsys):
    from streamspeech_amd import offline
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", str(tmp_path / "out"), "--align-reference"]
    (tmp_path / "none.yaml").write_text("source_unigram:\n  decoder_type: ctc\n")
    for extra in (["--synthetic", "2"], ["--wav-list", str(tmp_path / "list.txt")], [str(tmp_path)],
                  [str(tmp_path), "--multitask-config-yaml", "none.yaml"]):
        with pytest.raises(SystemExit) as e:
            offline.main(base + extra)
        assert e.value.code == 2
        assert "--align-reference" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


SYM = ["<s>", "<pad>", "</s>", "<unk>", "▁he", "llo", "▁wor", "ld"]


def test_ctc_decoder_align_feeds_words_from_ctc(lib):
    """CTCDecoder.align on a stand-in engine whose ctc_align is the host twin: the hypothesis goes through details_from_hyps /
    words_from_ctc unchanged."""
    from streamspeech_amd.engine import CtcAlignment
    from streamspeech_amd.generators import CTCDecoder
    from streamspeech_amd.words import details_from_hyps, words_from_ctc
    x2 = R.logits(60, 40, 8)
    seen = {}

    class Dict:
        def pad(self): return 1
        def eos(self): return 2
        def unk(self): return 3

    class Eng:
        def ctc_align(self, head, enc, tokens, want_path=True):
            seen["call"] = (head, tuple(enc.shape), list(tokens))
            rec = R.run(lib, [(x2, list(tokens))], 8, pad=PAD)[1][0]
            return CtcAlignment(rec["score"], rec["viterbi"], rec["status"], rec["path"].tolist(), rec["first"].tolist(),
                                rec["last"].tolist(), rec["tok_lprob"])

    dec = CTCDecoder(Dict(), Eng(), 1)
    enc = {"encoder_out": [torch.zeros(40, 1, 4)]}
    toks = [4, 5, 6, 7, 4]
    h = dec.align(enc, torch.tensor([toks]))[0][0]
    assert seen["call"] == (1, (40, 4), toks)
    assert h["tokens"].tolist() == toks and h["status"] == 0 and h["score"] >= h["viterbi_score"]
    assert h["token_scores"].dtype == torch.float32 and len(h["index"]) == len(h["last"]) == 5
    words = words_from_ctc(h["tokens"].tolist(), h["index"], h["last"], h["token_scores"].tolist(), SYM, finished=True)
    assert [w.text for w in words] == ["hello", "world", "he"]
    assert words[0].start_ms == h["index"][0] * 40 and words[1].end_ms == (h["last"][3] + 1) * 40
    assert all(0.0 < w.confidence <= 1.0 and w.stable for w in words)
    both = details_from_hyps(h, h, SYM, SYM, finished=True)
    assert [tuple(w) for w in both[0]] == [tuple(w) for w in words] == [tuple(w) for w in both[1]]
    assert R.collapse(h["path"]) == toks
    short = dec.align({"encoder_out": [torch.zeros(40, 1, 4)]}, [4] * 41)[0][0]      # (the stand-in's 40 frames)
    assert short["status"] == 1 and short["index"] == [-1] * 41 and short["score"] == -math.inf
