"""Host side of the text search controls (no-repeat n-grams, length penalty, temperature): the numpy restatement of the rules
(tests/search_ref.py) against the reference's own NGramRepeatBlock where the reference tree is present, the refusals of the
library's planner, and the Python surfaces that carry the three arguments (SequenceGenerator, the drivers' flags, the pools)."""
import argparse
import math
import os
import random

import numpy as np
import pytest

from tests import search_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_available():
    from oracle import ref_loader
    return ref_loader.available()


def _rows(rng, n_rows, length, V):
    # token 2 (</s>) at position 0 only, as in a hypothesis row; few symbols, so windows repeat often
    return [[2] + [rng.choice([t for t in range(V) if t != 2]) for _ in range(length - 1)] for _ in range(n_rows)]


@pytest.mark.skipif(not _reference_available(), reason="the reference tree is not present")
@pytest.mark.parametrize("n", [2, 3, 4])
def test_restatement_agrees_with_the_reference_block(n):
    import torch
    from oracle import ref_offline
    from oracle.ref_loader import _load_file
    ref_offline._install()
    Block = _load_file("fairseq.ngram_repeat_block", "fairseq/fairseq/ngram_repeat_block.py").NGramRepeatBlock
    block = Block(n, use_extension=False)
    rng = random.Random(100 + n)
    V, bsz, beam = 11, 8, 4
    banned_any = 0
    for length in range(1, 25):                  # step = length - 1: below n - 2, at n - 2, above
        rows = _rows(rng, bsz * beam, length, V)
        lp = np.array([[rng.uniform(-9, 0) for _ in range(V)] for _ in rows], dtype=np.float32)
        ref = block(torch.tensor(rows, dtype=torch.long), torch.tensor(lp), bsz, beam, length - 1).numpy()
        mine = SR.apply_ban(rows, lp, n)
        assert np.array_equal(ref, mine), (n, length)
        if length - 1 < n - 1:                   # no window can hold n - 1 earlier tokens and a banned one
            assert np.array_equal(mine, lp)
        banned_any += int(np.isinf(mine).sum())
    assert banned_any > 0                        # the rows do repeat


@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_eos_is_never_banned(n):
    rng = random.Random(7 * n)
    for length in range(1, 40):
        for row in _rows(rng, 20, length, 5):
            assert 2 not in SR.banned_tokens(row, n)


def test_restatement_on_a_hand_example():
    # </s> a b a b a: one more b would repeat the bigram a b, the trigram b a b and the 4-gram a b a b; no 5-gram stands twice
    row = [2, 7, 8, 7, 8, 7]
    assert SR.banned_tokens(row, 2) == {8}
    assert SR.banned_tokens(row, 3) == {8}
    assert SR.banned_tokens(row, 4) == {8}
    assert SR.banned_tokens(row, 5) == set()
    assert SR.banned_tokens([2, 7, 8, 9, 7], 2) == {8} and SR.banned_tokens([2, 7, 7, 7], 2) == {7}
    assert SR.banned_tokens([2], 2) == set() and SR.banned_tokens([2, 7], 3) == set()
    assert SR.prefix_repeats([7, 8, 7, 8], 2) and not SR.prefix_repeats([7, 8, 7], 2) and not SR.prefix_repeats([7, 8, 7, 8], 4)


def _plan(**kw):
    from streamspeech_amd.engine import plan_mt_beam_continue
    a = dict(Tp=[10, 12], n_prefix=[0, 0], max_len=[8, 8], beam=4)
    a.update(kw)
    return plan_mt_beam_continue(a.pop("Tp"), a.pop("n_prefix"), a.pop("max_len"), a.pop("beam"), **a)


def _refused(**kw):
    from streamspeech_amd.engine import ContinueRefused
    with pytest.raises(ContinueRefused) as e:
        _plan(**kw)
    return e.value.code


def test_plan_refuses_the_options_the_library_refuses():
    from streamspeech_amd import lib as L
    base = _plan()
    assert _plan(no_repeat_ngram_size=3, len_penalty=0.6, temperature=1.7) == base     # the options change no table
    for bad in (dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=33), dict(no_repeat_ngram_size=-2),
                dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=math.nan), dict(temperature=math.inf),
                dict(len_penalty=math.nan)):
        assert _refused(**bad) == L.SS_ERR_ARG, bad
    assert _plan(no_repeat_ngram_size=2) == base and _plan(no_repeat_ngram_size=32) == base


def test_plan_refuses_a_prefix_that_repeats_an_ngram():
    from streamspeech_amd import lib as L
    pre = dict(n_prefix=[4, 2], prefix_ids=[7, 8, 7, 8, 5, 6])
    _plan(**pre)                                                        # no ban: any prefix
    _plan(**pre, no_repeat_ngram_size=3)                                # no trigram stands twice in </s> 7 8 7 8
    assert _refused(**pre, no_repeat_ngram_size=2) == L.SS_ERR_ARG      # the bigram 7 8 does
    assert _refused(n_prefix=[2, 3], prefix_ids=[5, 6, 9, 9, 9], no_repeat_ngram_size=2) == L.SS_ERR_ARG   # the second utterance's
    _plan(n_prefix=[2, 3], prefix_ids=[5, 6, 9, 9, 4], no_repeat_ngram_size=2)      # 9 9 once is a bigram once


def test_plan_refusals_keep_their_order():
    """Options first, then the call's own checks in their order (argument, capacity), the repeated prefix last."""
    from streamspeech_amd import lib as L
    rep = dict(n_prefix=[4, 0], prefix_ids=[7, 8, 7, 8], no_repeat_ngram_size=2)
    assert _refused(**rep) == L.SS_ERR_ARG
    # a capacity refusal (B * beam > 256) comes before the repeated prefix ...
    big = dict(Tp=[10] * 65, n_prefix=[4] + [0] * 64, max_len=[8] * 65, prefix_ids=[7, 8, 7, 8], no_repeat_ngram_size=2)
    assert _refused(**big) == L.SS_ERR_CAPACITY
    assert _refused(**dict(rep, feat_rows=4)) == L.SS_ERR_CAPACITY
    # ... and a refused option before the capacity refusal
    assert _refused(**dict(big, no_repeat_ngram_size=1)) == L.SS_ERR_ARG
    assert _refused(**dict(big, temperature=0.0)) == L.SS_ERR_ARG


def test_a_short_options_struct_is_refused():
    import ctypes as C
    from streamspeech_amd import lib as L
    lib = L.load()
    i32 = lambda v: (C.c_int32 * len(v))(*v)      # noqa: E731
    dims, n_tab = (C.c_int32 * 8)(), C.c_int64(0)
    args = (1, 2, i32([9]), i32([0]), i32([0]), i32([6]), 1, 7, 7, 1026, 6000, 2, 1, dims, None, 0, C.byref(n_tab))
    ok = L.SSMtSearchOpts(C.sizeof(L.SSMtSearchOpts), 2, 1.0, 1.0)
    assert lib.ss_batch_mt_beam_continue_plan_opts(*args, C.byref(ok)) == 0
    assert lib.ss_batch_mt_beam_continue_plan_opts(*args, None) == 0
    short = L.SSMtSearchOpts(8, 2, 1.0, 1.0)
    assert lib.ss_batch_mt_beam_continue_plan_opts(*args, C.byref(short)) == L.SS_ERR_ARG
    assert C.sizeof(L.SSMtSearchOpts) == 16


class _Dict:
    def eos(self):
        return 2

    def pad(self):
        return 1


class _Engine:
    """Records the search SequenceGenerator asks for."""

    def __init__(self):
        from streamspeech_amd.config import ModelConfig
        self.cfg = ModelConfig()
        self.calls = []

    def batch_mt_beam_continue(self, enc, Tp, prefixes, max_len, beam, min_len=1, unk_penalty=0.0, normalize=True, **kw):
        import torch
        self.calls.append((beam, prefixes, kw))
        return [[{"tokens": prefixes[0] + [9, 2], "score": -1.0, "positional_scores": [-0.5] * (len(prefixes[0]) + 2)}]], \
            [torch.zeros(len(prefixes[0]) + 2, 4)]

    def mt_greedy(self, enc, prefix, max_len, min_len):
        import torch
        self.calls.append(("greedy", prefix))
        return [9, 2], torch.zeros(len(prefix) + 2, 4)


def _generate(gen, prefix=()):
    import torch
    enc = [{"encoder_out": [torch.zeros(6, 1, 4)]}]
    pt = torch.tensor([list(prefix)], dtype=torch.long) if prefix else None
    return gen.generate_decoder(enc, torch.zeros(1, 24, 80), None, prefix_tokens=pt)


def test_sequence_generator_honours_the_arguments():
    from streamspeech_amd.generators import SequenceGenerator
    eng = _Engine()
    _generate(SequenceGenerator(eng, _Dict(), beam_size=1))
    assert eng.calls == [("greedy", [])]                       # nothing set: the greedy search, as always
    eng.calls.clear()
    _generate(SequenceGenerator(eng, _Dict(), beam_size=1, no_repeat_ngram_size=3), prefix=(5, 6))
    assert eng.calls == [(1, [[5, 6]], {"len_penalty": 1.0, "temperature": 1.0, "no_repeat_ngram_size": 3})]
    eng.calls.clear()
    _generate(SequenceGenerator(eng, _Dict(), beam_size=4, len_penalty=0.6, temperature=1.7))
    assert eng.calls == [(4, [[]], {"len_penalty": 0.6, "temperature": 1.7, "no_repeat_ngram_size": 0})]
    eng.calls.clear()
    _generate(SequenceGenerator(eng, _Dict(), beam_size=4))
    assert eng.calls == [(4, [[]], {})]                        # a beam without options: the call it always made


@pytest.mark.parametrize("kw", [dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=33), dict(temperature=0.0),
                                dict(temperature=math.nan), dict(len_penalty=math.inf), dict(match_source_len=True)])
def test_sequence_generator_refuses(kw):
    from streamspeech_amd.generators import SequenceGenerator
    with pytest.raises(ValueError):
        SequenceGenerator(_Engine(), _Dict(), **kw)


def test_offline_parser_accepts_the_flags():
    from streamspeech_amd.offline import build_parser
    base = ["--path", "synthetic:0", "--vocoder", "v", "--results-path", "r"]
    a = build_parser().parse_args(base + ["--lenpen", "0.6", "--no-repeat-ngram-size", "3"])
    assert (a.lenpen, a.no_repeat_ngram_size) == (0.6, 3)
    d = build_parser().parse_args(base)
    assert (d.lenpen, d.no_repeat_ngram_size) == (1.0, 0)
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--match-source-len"])


def test_agent_parser_accepts_the_flags_and_leaves_the_greedy_step_unarmed():
    from streamspeech_amd.agent import StreamSpeechS2STAgent, _beam_kwargs, _greedy_mt
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    for cls in (StreamSpeechS2STAgent, StreamSpeechS2TTAgent):
        ap = argparse.ArgumentParser()
        cls.add_args(ap)
        flags = {s for act in ap._actions for s in act.option_strings}
        assert {"--lenpen", "--temperature", "--no-repeat-ngram-size"} <= flags
    ns = argparse.Namespace(beam_mt=1, lenpen=1.0, temperature=1.0, no_repeat_ngram_size=0, unkpen=0.5)
    assert _greedy_mt(ns) and _beam_kwargs(ns) == {}
    ns.no_repeat_ngram_size = 2
    assert not _greedy_mt(ns) and _beam_kwargs(ns) == {"len_penalty": 1.0, "temperature": 1.0, "no_repeat_ngram_size": 2}
    ns.beam_mt = 4
    assert _beam_kwargs(ns)["unk_penalty"] == 0.5
    assert _greedy_mt(argparse.Namespace())                    # an args object from before the flags


class _OfflineStandIn:
    """offline.generate's model: records the first-pass search it is asked for."""

    def __init__(self, cfg):
        self.cfg, self.calls = cfg, []

    def batch_fbank_cmvn(self, pcm, lens):
        import torch
        T = [n // 160 for n in lens]
        return torch.zeros(sum(T), 80), T

    def batch_encoder_forward(self, feat, T):
        import torch
        Tp = [t // 4 for t in T]
        return torch.zeros(sum(Tp), self.cfg.enc_dim), Tp

    def batch_ctc_greedy(self, head, enc, Tp):
        return [([10 + head], [0]) for _ in Tp]

    def batch_mt_greedy(self, enc, Tp, mx, min_len=1):
        import torch
        self.calls.append(("greedy",))
        return [[20, self.cfg.eos] for _ in Tp], torch.zeros(len(Tp), 4, self.cfg.dec_dim), [2] * len(Tp)

    def batch_mt_beam(self, enc, Tp, mx, beam, min_len=1, unk_penalty=0.0, normalize=True, **kw):
        import torch
        self.calls.append(("beam", beam, kw))
        nb = [[{"tokens": [30, self.cfg.eos], "score": -1.0, "positional_scores": [-0.5, -0.5]}] for _ in Tp]
        return nb, torch.zeros(len(Tp), 4, self.cfg.dec_dim), [2] * len(Tp)

    def batch_t2u_units(self, feats, n, t2u_causal=False, mask_eos=False):
        return [[] for _ in n]


def test_offline_generate_takes_the_beam_route_at_beam_1(tmp_path):
    import torch
    from oracle.ref_agent import make_dicts
    from streamspeech_amd import offline
    from streamspeech_amd.config import ModelConfig
    cfg = ModelConfig()
    items = [(4, torch.zeros(16000))]
    m = _OfflineStandIn(cfg)
    offline.generate(m, None, items, make_dicts(cfg), str(tmp_path / "a"), max_len_b_mt=12, dump_wav=False)
    assert m.calls == [("greedy",)]
    m = _OfflineStandIn(cfg)
    offline.generate(m, None, items, make_dicts(cfg), str(tmp_path / "b"), max_len_b_mt=12, dump_wav=False, no_repeat_ngram_size=2)
    assert m.calls == [("beam", 1, {"len_penalty": 1.0, "temperature": 1.0, "no_repeat_ngram_size": 2})]
    with pytest.raises(ValueError):
        offline.generate(m, None, items, make_dicts(cfg), str(tmp_path / "c"), max_len_b_mt=12, dump_wav=False, no_repeat_ngram_size=1)


def test_search_options_object():
    from streamspeech_amd.engine import SearchOptions, check_search_options
    assert SearchOptions().kwargs() == {} and check_search_options() is None
    assert SearchOptions(no_repeat_ngram_size=3).kwargs() == {"len_penalty": 1.0, "temperature": 1.0, "no_repeat_ngram_size": 3}
    o = check_search_options(0.6, 1.7, 2)
    assert (o.size, o.no_repeat_ngram, round(o.len_penalty, 6), round(o.temperature, 6)) == (16, 2, 0.6, 1.7)
    for bad in (dict(no_repeat_ngram_size=1), dict(temperature=0), dict(len_penalty=math.nan), dict(no_repeat_ngram_size=2.5)):
        with pytest.raises(ValueError):
            SearchOptions(**bad)


def test_golden_fixture_holds_what_the_tests_need():
    import json
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "search_options.json"), encoding="utf-8"))
    want = {"beam4_ngram2", "beam5_ngram3_lenpen0.6", "beam10_early_eos_lenpen1.5_temp1.7", "beam10_early_eos_lenpen0.5_temp1.7",
            "beam1_ngram2", "prefix_beam4_ngram2"}
    assert set(fix["groups"]) == want
    for name, grp in fix["groups"].items():
        recs = grp["cases"] if "cases" in grp else list(grp["hypotheses"].values())
        pinned = [r for r in recs if r["margin"] > r["tau"]]
        assert len(pinned) >= 6, name
        n = grp["no_repeat_ngram_size"]
        for r in pinned:
            for h in r["nbest"]:
                toks = [2] + h["tokens"]
                assert len(h["positional_scores"]) == len(h["tokens"])
                if n:       # the fixture obeys the rule it pins: no token of a hypothesis was banned when it was chosen
                    assert all(toks[q] not in SR.banned_tokens(toks[:q], n) for q in range(1, len(toks))), (name, toks)
    assert {len(c["prefix"]) for c in fix["groups"]["prefix_beam4_ngram2"]["cases"] if c["margin"] > c["tau"]} == {0, 1, 3}
