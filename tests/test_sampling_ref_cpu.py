"""Host side of the sampling search: the numpy restatement of the rule (tests/sampling_ref.py) against the known Philox vectors and
against the reference's own Sampling._sample_topp / topk where the reference tree is present, the monotone draw, the refusals of
check_sampling_options, the pinned struct size, and the Python surfaces that carry the arguments."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import sampling_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PHILOX_VECTORS = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def _reference_available():
    from oracle import ref_loader
    return ref_loader.available()


def peaked_rows(rng, R, V):
    return (rng.standard_normal((R, V)) * 4).astype(np.float32)


def test_philox_known_vectors():
    for ctr, key, out in PHILOX_VECTORS:
        assert SR.philox4x32_10(ctr, key) == out
    # the rule's counter / key layout: (step, j, key_lo, key_hi) under (seed_lo, seed_hi)
    ctr, key, out = PHILOX_VECTORS[2]
    assert SR.words(key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, ctr[0], ctr[1]) == out
    assert SR.uniform(key[0] | key[1] << 32, ctr[2] | ctr[3] << 32, ctr[0], ctr[1]) == (out[0] >> 8) / 2.0 ** 24
    assert SR.words(0, -1, 0, 0) == SR.words(0, 2 ** 64 - 1, 0, 0)          # keys are bit patterns


def test_uniform_is_a_float32_in_the_unit_interval():
    us = np.array([SR.uniform(7, k, s, j) for k in range(8) for s in range(8) for j in range(8)])
    assert np.all((us >= 0) & (us < 1)) and np.array_equal(us.astype(np.float32).astype(np.float64), us)
    assert len(set(us.tolist())) == len(us) and 0.35 < us.mean() < 0.65


@pytest.mark.skipif(not _reference_available(), reason="the reference tree is not present")
@pytest.mark.parametrize("V", [9, 97, 600])
def test_kept_sets_agree_with_the_reference(V):
    import torch
    from oracle import ref_offline
    from oracle.ref_loader import _load_file
    ref_offline._install()
    Sampling = _load_file("fairseq.search", "fairseq/fairseq/search.py").Sampling

    class D:
        def pad(self): return 1
        def unk(self): return 3
        def eos(self): return 2
        def __len__(self): return V

    rng = np.random.default_rng(V)
    rows = peaked_rows(rng, 24, V)
    v = np.stack([SR.row_values(r, pad=-1, unk=-1) for r in rows])
    n_checked = 0
    for P in (0.3, 0.9, 1.0):
        s = Sampling(D(), sampling_topp=P)
        probs, idx = s._sample_topp(torch.from_numpy(v).double()[:, None, :].clone())
        for r in range(len(rows)):
            kept, before = SR.kept_set(v[r], topp=P)
            if not SR.topp_decided(before, P, 1e-12):
                continue
            ref = sorted(int(i) for i, p in zip(idx[r, 0], probs[r, 0]) if p > 0)
            assert ref == kept, (P, r)
            n_checked += 1
    assert n_checked >= 60
    for K in (1, 5, V):
        _, idx = torch.from_numpy(v).double().topk(K)
        for r in range(len(rows)):
            assert sorted(idx[r].tolist()) == SR.kept_set(v[r], topk=K)[0]


def test_kept_set_rules():
    with np.errstate(divide="ignore"):
        v = np.log(np.array([0.1, 0.4, 0.0, 0.2, 0.2, 0.1]))
    assert SR.order(v) == [1, 3, 4, 0, 5]
    assert SR.kept_set(v)[0] == [0, 1, 3, 4, 5]                             # a -inf token is never kept
    assert SR.kept_set(v, topk=2)[0] == [1, 3] and SR.kept_set(v, topk=3)[0] == [1, 3, 4]    # ties go to the lower id
    assert SR.kept_set(v, topk=6)[0] == [0, 1, 3, 4, 5]
    assert SR.kept_set(v, topp=0.3)[0] == [1]                               # the token that crosses P is included
    assert SR.kept_set(v, topp=0.5)[0] == [1, 3] and SR.kept_set(v, topp=1.0)[0] == [0, 1, 3, 4, 5]
    at_max = SR.row_values(np.zeros(7, np.float32), step=5, max_len=5)
    for kw in (dict(), dict(topk=3), dict(topp=0.5)):
        assert SR.kept_set(at_max, **kw)[0] == [2]                          # a row at max_len keeps </s> alone
    below_min = SR.row_values(np.zeros(7, np.float32), step=0, min_len=1)
    assert 2 not in SR.kept_set(below_min)[0] and 1 not in SR.kept_set(below_min)[0]


def test_draw_is_monotone_in_u_and_covers_the_kept_set():
    rng = np.random.default_rng(3)
    for V, kw in ((9, {}), (97, dict(topk=5)), (97, dict(topp=0.9)), (300, {})):
        v = SR.row_values(peaked_rows(rng, 1, V)[0])
        kept, _ = SR.kept_set(v, **kw)
        us = np.sort(np.concatenate([[0.0, 1 - 2.0 ** -24], rng.random(400)]))
        toks = [SR.draw(v, kept, u) for u in us]
        assert all(a <= b for a, b in zip(toks, toks[1:])) and set(toks) <= set(kept)
        assert toks[0] == kept[0]
        for t, u in zip(toks, us):
            lo, hi, Z = SR.draw_interval(v, kept, t)
            assert lo <= u * Z < hi or (t == kept[-1] and u * Z >= lo)
    assert SR.draw(np.full(4, -np.inf), [], 0.5) is None


def test_chain_is_reproducible_and_ends_in_eos():
    rng = np.random.default_rng(11)
    table = peaked_rows(rng, 40, 30)

    def values(toks):
        return SR.row_values(table[len(toks)], step=len(toks), min_len=1, max_len=12)
    a = SR.sample_chain(values, 5, 77, 0)
    assert a == SR.sample_chain(values, 5, 77, 0) and a[0][-1] == 2 and 2 not in a[0][:-1] and len(a[0]) <= 13
    others = [SR.sample_chain(values, 5, 77, j)[0] for j in range(1, 6)] + [SR.sample_chain(values, 6, 77, 0)[0]]
    assert any(o != a[0] for o in others)


def test_check_sampling_options_refuses_what_the_library_refuses():
    from streamspeech_amd.engine import SamplingOptions, check_sampling_options, sampling_from_fairseq
    o = check_sampling_options(5, 0.0, 2 ** 64 - 1)
    assert (o.size, o.topk, o.topp, o.seed) == (24, 5, 0.0, 2 ** 64 - 1)
    assert check_sampling_options(0, 1.0, 0).topp == 1.0 and check_sampling_options().seed == 1
    assert check_sampling_options(6000, 0.0, 1, vocab=6000).topk == 6000
    for bad in (dict(topk=-1), dict(topk=2.5), dict(topp=-0.1), dict(topp=1.5), dict(topp=math.nan), dict(topp=math.inf),
                dict(topk=3, topp=0.5), dict(seed=-1), dict(seed=2 ** 64), dict(topk=6001, vocab=6000)):
        with pytest.raises(ValueError):
            check_sampling_options(**bad)
    with pytest.raises(ValueError):
        SamplingOptions(topk=2, topp=0.2)
    assert SamplingOptions(topp=0.9, seed=4).kwargs() == {"topk": 0, "topp": 0.9, "seed": 4}
    # fairseq's names: -1 is off; top-k / top-p without --sampling is refused as build_generator refuses it
    assert sampling_from_fairseq(False) is None
    assert sampling_from_fairseq(True, -1, -1.0, 3).kwargs() == {"topk": 0, "topp": 0.0, "seed": 3}
    assert sampling_from_fairseq(True, 10, -1.0).kwargs()["topk"] == 10
    with pytest.raises(ValueError):
        sampling_from_fairseq(False, 10)
    with pytest.raises(ValueError):
        sampling_from_fairseq(True, 10, 0.5)


def test_struct_size_and_symbols():
    from streamspeech_amd import lib as L
    assert C.sizeof(L.SSMtSampleOpts) == 24 and L.SSMtSampleOpts.seed.offset == 16
    assert C.sizeof(L.SSMtSearchOpts) == 16                                 # sampling did not extend the search options
    lib = L.load()
    header = open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8").read()
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header
    for sym in ("ss_batch_mt_sample", "ss_batch_mt_sample_continue", "ss_op_sample_step", "ss_op_sample_uniform"):
        assert sym in header and hasattr(lib, sym)


def test_library_refusals_come_before_everything_else():
    """Every sampling refusal is made with a NULL model and NULL buffers: nothing else has been looked at."""
    from streamspeech_amd import lib as L
    lib = L.load()
    keys = (C.c_int64 * 1)(5)

    def call(opts, k=keys):
        return lib.ss_batch_mt_sample(None, None, 0, 0, None, None, None, 1, 0.0, 1, None, 0, None, None, None, None, 0, None, k,
                                      C.byref(opts) if opts is not None else None)
    mk = lambda size=24, topk=0, topp=0.0: L.SSMtSampleOpts(size, topk, topp, 0, 1)   # noqa: E731
    for bad in (None, mk(size=16), mk(topk=-1), mk(topp=math.nan), mk(topp=-0.5), mk(topp=1.25), mk(topk=4, topp=0.5)):
        assert call(bad) == L.SS_ERR_ARG
    assert call(mk(), k=None) == L.SS_ERR_ARG
    assert call(mk(topk=3)) == L.SS_ERR_ARG                                 # the NULL model, after the options
    bad_search = L.SSMtSearchOpts(16, 1, 1.0, 1.0)
    assert lib.ss_batch_mt_sample_continue(None, None, 0, 0, None, None, None, None, None, 1, 0.0, 1, None, 0, None, None, None, None, 0,
                                           C.byref(bad_search), keys, C.byref(mk(size=8))) == L.SS_ERR_ARG


class _Dict:
    def eos(self):
        return 2

    def pad(self):
        return 1


class _Engine:
    """Records the search SequenceGenerator asks for."""

    def __init__(self):
        from streamspeech_amd.config import ModelConfig
        self.cfg, self.calls = ModelConfig(), []

    def batch_mt_sample_continue(self, enc, Tp, prefixes, max_len, n_samples, keys, **kw):
        import torch
        self.calls.append(("sample", n_samples, prefixes, list(keys), kw))
        return [[{"tokens": prefixes[0] + [9, 2], "score": -1.0, "positional_scores": [-0.5] * (len(prefixes[0]) + 2)}] * n_samples], \
            [torch.zeros(len(prefixes[0]) + 2, 4)]

    def mt_greedy(self, enc, prefix, max_len, min_len):
        import torch
        self.calls.append(("greedy", prefix))
        return [9, 2], torch.zeros(len(prefix) + 2, 4)


def test_sequence_generator_takes_fairseq_s_sampling_arguments():
    import torch
    from streamspeech_amd.generators import SequenceGenerator
    enc = [{"encoder_out": [torch.zeros(6, 1, 4)]}]
    eng = _Engine()
    gen = SequenceGenerator(eng, _Dict(), beam_size=3, sampling=True, sampling_topk=10, seed=7, temperature=1.7)
    out = gen.generate_decoder(enc, torch.zeros(1, 24, 80), None, prefix_tokens=torch.tensor([[5, 6]]))
    assert len(out[0]) == 3
    (kind, n, prefixes, keys, kw), = eng.calls
    assert (kind, n, prefixes, keys) == ("sample", 3, [[5, 6]], [0])
    assert kw["topk"] == 10 and kw["topp"] == 0.0 and kw["seed"] == 7 and kw["temperature"] == 1.7
    eng.calls.clear()
    SequenceGenerator(eng, _Dict(), beam_size=1).generate_decoder(enc, torch.zeros(1, 24, 80), None)
    assert eng.calls == [("greedy", [])]                                     # sampling off: the call it always made
    for bad in (dict(sampling_topk=5), dict(sampling=True, sampling_topk=5, sampling_topp=0.5), dict(sampling=True, sampling_topp=1.5)):
        with pytest.raises(ValueError):
            SequenceGenerator(eng, _Dict(), **bad)


def test_offline_parser_accepts_the_flags():
    from streamspeech_amd.offline import build_parser
    base = ["--path", "synthetic:0", "--vocoder", "v", "--results-path", "r"]
    a = build_parser().parse_args(base + ["--sampling", "--sampling-topk", "10", "--seed", "5", "--beam-mt", "4"])
    assert (a.sampling, a.sampling_topk, a.sampling_topp, a.seed, a.beam_mt) == (True, 10, -1.0, 5, 4)
    d = build_parser().parse_args(base)
    assert (d.sampling, d.sampling_topk, d.sampling_topp, d.seed) == (False, -1, -1.0, 1)


def test_agent_parsers_accept_the_flags_and_sampling_disarms_the_greedy_step():
    import argparse
    from streamspeech_amd.agent import StreamSpeechS2STAgent, _beam_kwargs, _greedy_mt
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.engine import sampling_stream_key
    for cls in (StreamSpeechS2STAgent, StreamSpeechS2TTAgent):
        ap = argparse.ArgumentParser()
        cls.add_args(ap)
        flags = {s for act in ap._actions for s in act.option_strings}
        assert {"--sampling", "--sampling-topk", "--sampling-topp", "--seed", "--sampling-session"} <= flags
    ns = argparse.Namespace(beam_mt=1, lenpen=1.0, temperature=1.0, no_repeat_ngram_size=0, unkpen=0.5)
    assert _greedy_mt(ns) and _beam_kwargs(ns) == {}                         # everything off: nothing changes
    ns.sampling, ns.sampling_topp, ns.seed = True, 0.9, 4
    assert not _greedy_mt(ns)
    assert _beam_kwargs(ns) == {"sampling": True, "sampling_topk": -1, "sampling_topp": 0.9, "seed": 4}
    keys = {sampling_stream_key(s, n) for s in range(50) for n in range(50)}
    assert len(keys) == 2500 and sampling_stream_key(3, 7) == sampling_stream_key(3, 7)


def test_pools_take_sampling_options_as_search():
    from streamspeech_amd.engine import SamplingOptions, SearchOptions
    o = SamplingOptions(topp=0.9, seed=2, search=SearchOptions(temperature=1.7))
    assert o.kwargs() == {"topk": 0, "topp": 0.9, "seed": 2} and o.search.kwargs()["temperature"] == 1.7
