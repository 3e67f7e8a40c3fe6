"""tests/ctc_ref.py against torch and the reference's own post-processing rule, the host span twin of pipeline.py against it, and
words_from_ctc's cases -- all without a device.  Plus the ABI check of the entry points tests/test_ctc_scores_gpu.py calls."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ctc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, UNK = 1, 3


def test_scored_entry_points_are_declared_and_bound():
    from streamspeech_amd import lib as L
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in (("ss_ctc_greedy_scored", 13), ("ss_batch_ctc_greedy_scored", 13), ("ss_stream_pool_set_scores", 2),
                        ("ss_stream_pool_ctc_scored", 14), ("ss_op_masked_argmax_lprob", 10), ("ss_op_ctc_collapse_spans", 13)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"


def _rows(seed, M, N):
    return (np.random.default_rng(seed).standard_normal((M, N)) * 6).astype(np.float32)


@pytest.mark.parametrize("M,N", [(1, 64), (3, 255), (5, 257), (2, 1005), (4, 6000)])
def test_lprob_is_log_softmax_then_masks_then_max(M, N):
    """agent/ctc_decoder.py:54-61: lprobs = log_softmax; lprobs[pad] = lprobs[unk] = -inf; max."""
    x = _rows(N, M, N)
    x[0, PAD] = 50.0                                       # the row maximum on a masked column
    ids, lp = R.masked_argmax_lprob(x, N, (PAD, UNK))
    ref = torch.log_softmax(torch.from_numpy(x).double(), dim=-1)
    ref[:, PAD] = -math.inf
    ref[:, UNK] = -math.inf
    val, idx = ref.max(dim=-1)
    assert ids.tolist() == idx.tolist()
    assert np.abs(lp - val.numpy()).max() < 1e-12


def test_lprob_special_rows():
    N = 300
    x = _rows(1, 6, N)
    x[0, 7] = x[0, 200] = 30.0                             # two equal maxima: the lower index
    x[1, 10:40] = -np.inf
    x[2, 5] = np.nan                                       # NaN: lprob NaN, the arg-max as if it were -inf
    x[3] = 80.0
    x[4] = -80.0
    x[5, :] = -np.inf
    x[5, 9] = np.nan                                       # NaN stays a candidate among -inf: the FIRST unmasked column wins
    ids, lp = R.masked_argmax_lprob(x, N, (PAD, UNK))
    assert ids[0] == 7 and ids[3] == 0 and ids[4] == 0 and ids[5] == 0
    assert math.isnan(lp[2]) and math.isnan(lp[5])
    y = x[2].copy()
    y[5] = -np.inf
    assert ids[2] == R.masked_argmax_lprob(y[None], N, (PAD, UNK))[0][0]
    assert abs(lp[3] + math.log(N)) < 1e-12 and abs(lp[4] + math.log(N)) < 1e-12
    only = [n for n in range(N) if n != 17]                # all columns but one masked
    assert R.masked_argmax_lprob(x[:1], N, only)[0][0] == 17


def _postprocess(toks, pad):
    """agent/ctc_decoder.py:67-89, as written there."""
    dedup = [(v, i) for i, v in enumerate(toks) if i == 0 or v != toks[i - 1]]
    return [v for v, i in dedup if v != 0 and v != pad], [i for v, i in dedup if v != 0 and v != pad]


def _raws():
    rng = np.random.default_rng(3)
    out = [[5], [0], [4, 4], [0] * 30, [9] * 30, [0, PAD, 7, 7, PAD, 7, 0, 7, 8, 8, 8]]
    for T in (17, 100, 1025):
        out.append(np.repeat(rng.integers(0, 6, T), rng.integers(1, 5, T))[:T].tolist())
    return out


def test_collapse_follows_the_reference_rule_and_the_host_twin_agrees():
    from streamspeech_amd.pipeline import ctc_collapse_host, ctc_collapse_spans_host
    rng = np.random.default_rng(4)
    for raw in _raws():
        lp = (-rng.random(len(raw)) * 3).astype(np.float32)
        toks, index, last, s64, s32 = R.collapse_spans(raw, lp, 0, PAD)
        assert (toks, index) == _postprocess(raw, PAD) == ctc_collapse_host(raw, 0, PAD)
        for j, (a, b) in enumerate(zip(index, last)):
            assert all(raw[k] == toks[j] for k in range(a, b + 1)) and (b + 1 == len(raw) or raw[b + 1] != toks[j])
        assert np.abs(s64 - s32).max(initial=0.0) < 1e-4
        t2, i2, l2, p2 = ctc_collapse_spans_host(raw, lp, 0, PAD)
        assert (t2, i2, l2) == (toks, index, last)
        assert p2.dtype == np.float32 and p2.tobytes() == s32.tobytes()


SYM = ["<s>", "<pad>", "</s>", "<unk>", "▁he", "llo", "▁wor", "ld", "▁a", "tail"]


def _check(args, **kw):
    from streamspeech_amd.words import Word, words_from_ctc
    got = words_from_ctc(*args, SYM, **kw)
    want = R.words(*args, SYM, **kw)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, Word)
        assert tuple(g[:3]) == w[:3] and g.stable == w[4]
        assert (math.isnan(g.confidence) and math.isnan(w[3])) or g.confidence == pytest.approx(w[3], rel=1e-12)
    return got


def test_words_from_ctc():
    lp = np.log(np.array([0.5, 0.25, 0.9, 0.8, 0.7, 0.6], np.float64))
    # "tail" leads without the mark: it starts the first word; "a" is a single-frame word
    toks, index, last = [9, 4, 5, 8, 6, 7], [0, 2, 5, 7, 9, 11], [1, 4, 5, 7, 10, 12]
    tl = np.array([2 * lp[0], 3 * lp[1], lp[2], lp[3], 2 * lp[4], 2 * lp[5]], np.float32)
    w = _check((toks, index, last, tl), n_final=7, t0_ms=1000)
    assert [x.text for x in w] == ["tail", "hello", "a", "world"]
    assert (w[0].start_ms, w[0].end_ms) == (1000, 1080) and (w[2].start_ms, w[2].end_ms) == (1280, 1320)
    assert w[1].confidence == pytest.approx(math.exp((3 * lp[1] + lp[2]) / 4), rel=1e-6)
    assert w[2].confidence == pytest.approx(0.8, rel=1e-6)
    # "a" starts at frame 7: "hello" is stable only once 7 < n_final -- a boundary exactly at n_final is not enough
    assert [x.stable for x in w] == [True, False, False, False]
    assert [x.stable for x in _check((toks, index, last, tl), n_final=8)] == [True, True, False, False]
    assert [x.stable for x in _check((toks, index, last, tl), n_final=13)] == [True, True, True, False]
    assert [x.stable for x in _check((toks, index, last, tl), n_final=0, finished=True)] == [True] * 4
    assert [x.stable for x in _check((toks, index, last, tl))] == [None] * 4
    assert _check(([], [], [], np.zeros(0, np.float32)), n_final=3) == []
    tl[1] = np.nan                                         # a NaN row inside "hello": passed through, the others untouched
    w = _check((toks, index, last, tl), n_final=7)
    assert math.isnan(w[1].confidence) and not math.isnan(w[0].confidence)
    assert all(0.0 < x.confidence <= 1.0 for k, x in enumerate(w) if k != 1)
    from streamspeech_amd.words import words_from_ctc
    with pytest.raises(ValueError):
        words_from_ctc(toks, index, last[:-1], tl, SYM)


def test_ctc_decoder_generate_with_scores_and_prefix():
    """CTCDecoder.generate(want_scores=True) on a stand-in engine: positional_scores / score as agent/ctc_decoder.py:61-62,104-105,
    and with a prefix the spans of the spliced ids from the host twin."""
    from streamspeech_amd.generators import CTCDecoder

    raw = [0, 4, 4, 0, 5, 5, 5, 6]
    lp = (-np.arange(1, 9) / 8).astype(np.float32)

    class Dict:
        def pad(self): return PAD
        def eos(self): return 2
        def unk(self): return UNK

    class Eng:
        def ctc_greedy(self, head, enc, want_logits=False, want_scores=False):
            t, i, l, _, s = R.collapse_spans(raw, lp, 0, PAD)
            base = (t, i, torch.tensor(raw, dtype=torch.int32), None)
            return base + (l, s, lp) if want_scores else base

    dec = CTCDecoder(Dict(), Eng(), 0)
    enc = {"encoder_out": [torch.zeros(8, 1, 4)]}
    plain = dec.generate(enc)[0][0]
    assert "positional_scores" not in plain and "score" not in plain
    h = dec.generate(enc, want_scores=True)[0][0]
    assert h["tokens"].tolist() == plain["tokens"].tolist() == [4, 5, 6] and h["index"] == plain["index"]
    assert h["positional_scores"].dtype == torch.float32 and h["positional_scores"].numpy().tobytes() == lp.tobytes()
    assert h["score"] == float(lp.astype(np.float64).sum())
    assert h["last"] == [2, 6, 7]
    hp = dec.generate(enc, prefix=torch.tensor([[7, 7, 4]]), want_scores=True)[0][0]
    merged = [7, 7, 4, 0, 5, 5, 5, 6]
    t, i, l, _, s = R.collapse_spans(merged, lp, 0, PAD)
    assert hp["tokens"].tolist() == t and hp["index"] == i and hp["last"] == l
    assert hp["token_scores"].numpy().tobytes() == s.tobytes()
    assert hp["positional_scores"].numpy().tobytes() == lp.tobytes()
