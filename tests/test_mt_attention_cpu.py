"""The cross-attention of the first-pass text search, the parts that need no GPU: the float64 reference of the attention
probabilities kernel (tests/mt_attention_ref.py) against torch.softmax(...).mean(heads), the decisive-row rule of the GPU cases on
the reference alone, words_from_attention, the reference fixture tests/golden/mt_attention.npz (and, where the reference tree
exists, its regeneration), the new symbols, and the --mt-alignment flag of the offline driver and the agents."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import mt_attention_ref as R
from streamspeech_amd.words import AlignedWord, words_from_attention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mt_attention.npz")


def _softmax_mean(q, k, H, scale):
    n, kl = q.shape[0], k.shape[0]
    qh = q.double().reshape(n, H, 64).permute(1, 0, 2)
    kh = k.double().reshape(kl, H, 64).permute(1, 0, 2)
    return torch.softmax(torch.einsum("hid,hjd->hij", qh, kh) * scale, -1).mean(0)


def test_reference_against_softmax_mean():
    """Ragged cases with k_len = 1 and a tie: P, the first-maximum peak, and the two statistics."""
    H = 4
    g = torch.Generator().manual_seed(3)
    Q = torch.randn(40, H * 64, generator=g) * 0.3
    K = torch.randn(90, H * 64, generator=g)
    K[60] = K[52]                                             # two identical key rows inside segment 2 (keys 12 and 20 of it)
    Q[30:36] = K[52] * 0.3
    segs = [(0, 7, 0, 1), (7, 20, 1, 33), (27, 13, 40, 50)]
    q_first = [0, 5, 2]
    for (qs, ql, ks, kl), f, (P, peak, stat) in zip(segs, q_first, R.ragged_probs_ref(Q, K, H, 0.7, segs, q_first)):
        want = _softmax_mean(Q[qs + f:qs + ql], K[ks:ks + kl], H, 0.7)
        assert P.shape == (ql - f, kl) and P.dtype == torch.float64
        assert float((P - want).abs().max()) < 1e-14
        assert float((P.sum(1) - 1).abs().max()) < 1e-13
        assert torch.equal(peak, torch.max(P, dim=1).indices)                  # torch.max: the first maximum
        assert torch.equal(stat[:, 0], P.max(1).values)
        assert float((stat[:, 1] - (want * torch.arange(kl, dtype=torch.float64)).sum(1)).abs().max()) < 1e-11
        if kl == 1:
            assert torch.equal(P, torch.ones_like(P)) and int(peak.max()) == 0
    P, peak, _ = R.ragged_probs_ref(Q, K, H, 0.7, segs, q_first)[2]
    assert torch.equal(P[1:7, 12], P[1:7, 20]) and peak[1:7].tolist() == [12] * 6       # rows 30 .. 35: the tie, the lower index
    f32 = R.probs_ref(Q[7:27], K[1:34], H, 0.7, torch.float32)
    assert f32.dtype == torch.float32 and float((f32.double() - R.probs_ref(Q[7:27], K[1:34], H, 0.7)).abs().max()) < 1e-6


@pytest.mark.parametrize("name", list(R.op_cases()))
def test_gpu_cases_are_decisive_on_the_reference_alone(name):
    """The GPU test asks for equal peaks wherever the float64 top-2 gap exceeds twice the bound, and for 90 % such rows per case:
    the reference alone meets that on the chosen seeds (the tie case pins the tie rule instead: its maximum is held twice)."""
    c = R.op_cases()[name]
    data = R.case_data(c)
    P64 = [R.probs_ref(q[f:], k, R.H_OP, c["scale"]) for (q, k), f in zip(data, c["q_first"])]
    P32 = [R.probs_ref(q[f:], k, R.H_OP, c["scale"], torch.float32) for (q, k), f in zip(data, c["q_first"])]
    bound = R.case_bound(c, P64, P32)
    assert bound >= R.TOL
    if name == "tie":
        for s, (j1, j2) in c["ties"].items():
            assert torch.equal(R.peak_ref(P64[s]), torch.full((P64[s].shape[0],), j1)) and torch.equal(P64[s][:, j1], P64[s][:, j2])
        return
    gaps = torch.cat([R.top2_gap(p) for p in P64])
    assert float((gaps > 2 * bound).float().mean()) >= 0.9
    for p32, p64 in zip(P32, P64):                             # the float32 run of the reference is inside the bound itself
        assert float((p32.double() - p64).abs().max()) <= bound


class _Syms:
    def __init__(self, table):
        self.t = table

    def __getitem__(self, i):
        return self.t[int(i)]


def test_words_from_attention():
    syms = _Syms(["<s>", "<pad>", "</s>", "<unk>", "▁he", "llo", "▁wor", "ld", "▁x", "tail"])
    # a leading subword without the mark starts the first word; </s> is dropped wherever it stands
    toks = [9, 4, 5, 2, 6, 7, 8, 2]
    peak = [3, 7, 5, 0, 10, 12, 11, 99]
    prob = [0.5, 0.25, 0.75, 0.1, 1.0, 0.5, 0.125, 0.9]
    w = words_from_attention(toks, peak, prob, syms)
    assert w == [AlignedWord("tail", 120, 160, 0.5), AlignedWord("hello", 200, 320, 0.5), AlignedWord("world", 400, 520, 0.75),
                 AlignedWord("x", 440, 480, 0.125)]
    assert words_from_attention(toks, peak, prob, syms, eos=2) == w
    w2 = words_from_attention(toks[:3], peak[:3], prob[:3], syms, frame_ms=10, t0_ms=1000)
    assert w2 == [AlignedWord("tail", 1030, 1040, 0.5), AlignedWord("hello", 1050, 1080, 0.5)]
    assert words_from_attention([], [], [], syms) == [] and words_from_attention([2], [1], [0.5], syms) == []
    with pytest.raises(ValueError):
        words_from_attention([4, 5], [1], [0.5, 0.5], syms)


def test_fixture_shapes_and_columns():
    g = np.load(GOLD)
    assert int(g["n"]) == 4 and os.path.getsize(GOLD) < (1 << 20)
    from streamspeech_amd import lib as L
    lib = L.load()
    for u in range(4):
        fb, toks, a32, a64 = g[f"fbank{u}"], g[f"tokens{u}"], g[f"attn32_{u}"], g[f"attn64_{u}"]
        assert fb.dtype == np.float32 and fb.shape[1] == 80 and toks.dtype == np.int32 and toks[-1] == 2
        Tp = lib.ss_encoder_out_len(fb.shape[0])
        assert a32.shape == a64.shape == (Tp, len(toks)), "[src_len, tgt_len]"
        for a in (a32, a64):
            assert np.abs(a.astype(np.float64).sum(0) - 1).max() < 1e-5, "every column is a distribution over the source"
            assert (a >= 0).all()


def test_fixture_regenerates():
    if not os.path.isdir("/root/reference"):
        pytest.skip("no reference tree")
    from tests import make_golden_mt_attention as M
    new, g = M.generate(), np.load(GOLD)
    assert sorted(new) == sorted(g.files)
    for k in g.files:                     # tokens and shapes exactly; the float arrays to 1e-6: the reference's float32 GEMMs sum in an
        assert new[k].dtype == g[k].dtype and new[k].shape == g[k].shape, k      # order that depends on the BLAS thread count (1e-8 seen)
        if k.startswith("attn") or k.startswith("fbank"):
            assert np.abs(new[k].astype(np.float64) - g[k].astype(np.float64)).max() <= 1e-6 * max(1.0, np.abs(g[k]).max()), k
        else:
            assert np.array_equal(new[k], g[k]), k


def test_new_symbols_exported_and_prototyped():
    from streamspeech_amd import lib as L
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    for name, nargs in (("ss_batch_mt_attention", 15), ("ss_op_attention_probs", 2)):
        assert f"int {name}(" in hdr and hasattr(lib, name)
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
    assert lib.ss_abi_version() == 2
    assert [f for f, _ in L.SSOpAttnProbsArgs._fields_] == ["Q", "K", "ldq", "ldk", "H", "scale", "segs", "nseg", "q_first", "row_off",
                                                            "p_off", "P", "peak", "stat", "max_rows"]


def test_mt_alignment_flag():
    """--mt-alignment is parsed by the offline driver and the two translation agents (default off), and refused by the ASR agent."""
    from streamspeech_amd import offline
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", "/tmp/x"]
    assert offline.build_parser().parse_args(base).mt_alignment is False
    assert offline.build_parser().parse_args(base + ["--mt-alignment"]).mt_alignment is True
    for cls in (StreamSpeechS2STAgent, StreamSpeechS2TTAgent):
        p = argparse.ArgumentParser()
        cls.add_args(p)
        req = ["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0"]
        assert p.parse_args(req).mt_alignment is False and p.parse_args(req + ["--mt-alignment"]).mt_alignment is True
        assert cls.alignment is None
    p = argparse.ArgumentParser()
    StreamSpeechASRAgent.add_args(p)
    args = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--mt-alignment"])
    with pytest.raises(ValueError, match="mt-alignment"):      # before anything is loaded: the refusal needs no GPU
        StreamSpeechASRAgent(args)


def test_generator_and_pool_switches_default_off():
    import inspect
    from streamspeech_amd.generators import SequenceGenerator
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd.text_pool import TextSessionPool
    assert inspect.signature(SequenceGenerator.__init__).parameters["want_attention"].default is False
    for cls in (TextSessionPool, SpeechSessionPool):
        assert inspect.signature(cls.__init__).parameters["align"].default is False
