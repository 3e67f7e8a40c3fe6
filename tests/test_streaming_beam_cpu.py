"""Host side of the beam search in the streaming path: the agents' --beam-mt / --unkpen flags, SequenceGenerator's routing at
beam > 1, the refusals and layout of ss_batch_mt_beam_continue read from the library's own planner
(ss_batch_mt_beam_continue_plan, the code the call runs), the pools' beam_mt argument, and the fixture against the reference where
the reference tree exists.  No GPU (the library loads without one)."""
import argparse
import json
import os

import pytest
import torch

from streamspeech_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(L.LIB_PATH):            # a clean checkout before build(): the planner lives in the library
        import __graft_entry__
        __graft_entry__.build()


# ---- the agents' flags ------------------------------------------------------------------------------------------------------------
BASE = ["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0", "--sample-rate", "16000"]


def _agents():
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    return [StreamSpeechS2STAgent, StreamSpeechS2TTAgent]


def _parser(agent):
    p = argparse.ArgumentParser()
    agent.add_args(p)
    return p


@pytest.mark.parametrize("i", [0, 1])
def test_parsers_take_the_beam_flags(i, capsys):
    p = _parser(_agents()[i])
    a = p.parse_args(BASE)
    assert a.beam_mt == 1 and a.unkpen == 0.0
    a = p.parse_args(BASE + ["--beam-mt", "4", "--unkpen", "0.5"])
    assert a.beam_mt == 4 and a.unkpen == 0.5
    assert p.parse_args(BASE + ["--beam-mt", "32"]).beam_mt == 32
    for bad in ("0", "33"):
        with pytest.raises(SystemExit):
            p.parse_args(BASE + ["--beam-mt", bad])
        assert "--beam-mt must be in [1, 32]" in capsys.readouterr().err


@pytest.mark.parametrize("i", [0, 1])
@pytest.mark.parametrize("flags,want", [([], dict(beam_size=1)), (["--beam-mt", "4", "--unkpen", "0.25"], dict(beam_size=4, unk_penalty=0.25))])
def test_agents_build_generator_mt_with_the_beam(i, flags, want, synth_weights, monkeypatch):
    from streamspeech_amd import agent as A, agent_text as AT
    from streamspeech_amd.modules import StreamSpeechModel
    from tests.oracle_engine import OracleEngine, OracleVocoder
    cfg, vcfg, sd, vsd = synth_weights
    seen = {}

    class Spy(A.SequenceGenerator):
        def __init__(self, engine, tgt_dict, **kw):
            seen.update(kw)
            super().__init__(engine, tgt_dict, **kw)
    monkeypatch.setattr(A, "SequenceGenerator", Spy)
    monkeypatch.setattr(AT, "SequenceGenerator", Spy)
    a = _parser(_agents()[i]).parse_args(BASE + ["--dur-prediction"] + flags)
    a.source_segment_size, a.device = 320, "cpu"
    model = StreamSpeechModel.from_engine(OracleEngine(sd, cfg))
    if i == 0:
        _agents()[0](a, model=model, vocoder=OracleVocoder(vsd, vcfg))
    else:
        _agents()[1](a, model=model)
    for k, v in want.items():
        assert seen[k] == v
    if not flags:                                  # the default builds exactly what it built before the flags existed
        assert "unk_penalty" not in seen and "normalize_scores" not in seen


# ---- SequenceGenerator --------------------------------------------------------------------------------------------------------------
class _Dict:
    def eos(self):
        return 2

    def pad(self):
        return 1


class _Engine:
    class cfg:
        max_target_positions = 1024

    def __init__(self):
        self.calls = []

    def mt_greedy(self, enc, prefix, max_len, min_len):
        self.calls.append(("mt_greedy", list(prefix), max_len, min_len))
        return [9, 2], torch.zeros((len(prefix) + 2, 4))

    def batch_mt_beam_continue(self, enc, Tp, prefixes, max_len, beam, min_len=1, unk_penalty=0.0, normalize=True):
        self.calls.append(("beam", list(Tp), [list(p) for p in prefixes], list(max_len), beam, min_len, unk_penalty, normalize))
        pre = list(prefixes[0])
        nbest = [{"tokens": pre + [9 + i, 2], "score": -1.0 - i, "positional_scores": [-0.5] * (len(pre) + 2)} for i in range(beam)]
        return [nbest], [torch.zeros((len(pre) + 2, 4))]


def _generate(gen, prefix, max_new):
    enc = {"encoder_out": [torch.zeros((7, 1, 4))]}
    return gen.generate_decoder([enc], torch.zeros((1, 30, 80)), torch.tensor([30]), {"id": 1},
                                torch.tensor([prefix]) if prefix else None, None, None, aux_task_name="", max_new_tokens=max_new)


def test_generator_routes_a_beam_to_the_forced_beam_search():
    from streamspeech_amd.generators import SequenceGenerator
    greedy_eng, eng = _Engine(), _Engine()
    g1 = SequenceGenerator(greedy_eng, _Dict(), beam_size=1, max_len_a=1, max_len_b=200)
    g4 = SequenceGenerator(eng, _Dict(), beam_size=4, max_len_a=1, max_len_b=200, unk_penalty=0.5, normalize_scores=False)
    for prefix, new in (([5, 6, 7], 2), ([], -1), ([5], 1)):
        _generate(g1, prefix, new)
        out = _generate(g4, prefix, new)
        kind, pre1, max_len1, min_len1 = greedy_eng.calls[-1]
        assert kind == "mt_greedy"
        assert eng.calls[-1] == ("beam", [7], [prefix], [max_len1], 4, min_len1, 0.5, False)      # B = 1, the greedy path's max_len
        hyps = out[0]
        assert len(hyps) == 4 and [h["score"] for h in hyps] == sorted((h["score"] for h in hyps), reverse=True)
        assert all(h["tokens"].tolist()[:len(prefix)] == prefix for h in hyps)
        assert hyps[0]["features"] is not None and all(h["features"] is None for h in hyps[1:])
        assert all(len(h["positional_scores"]) == len(h["tokens"]) for h in hyps)
    assert all(c[0] == "mt_greedy" for c in greedy_eng.calls) and all(c[0] == "beam" for c in eng.calls)
    with pytest.raises(ValueError):
        SequenceGenerator(eng, _Dict(), beam_size=33)


# ---- the host planner -----------------------------------------------------------------------------------------------------------------
# One call per refusal of ss_batch_mt_beam_continue, in the order the call checks them (Tp None = a valid encoder length);
# tests/test_streaming_beam_gpu.py sends the same calls to the device.
def _case(name, code, B=1, beam=4, Tp=None, n_prefix=None, max_len=None, ids=None, feat_rows=11, out_stride=11, **kw):
    n_prefix = [2] * B if n_prefix is None else n_prefix
    return dict(name=name, code=code, B=B, beam=beam, Tp=[None] * B if Tp is None else Tp, n_prefix=n_prefix,
                max_len=[10] * B if max_len is None else max_len, ids=[5] * sum(max(n, 0) for n in n_prefix) if ids is None else ids,
                feat_rows=feat_rows, out_stride=out_stride, **kw)


REFUSALS = [
    _case("no utterance", L.SS_ERR_ARG, B=0, n_prefix=[], max_len=[], Tp=[]),
    _case("beam 0", L.SS_ERR_ARG, beam=0),
    _case("beam 33", L.SS_ERR_ARG, beam=33),
    _case("B * beam = 260 rows", L.SS_ERR_CAPACITY, B=65, beam=4),
    _case("B * beam = 288 rows", L.SS_ERR_CAPACITY, B=9, beam=32),
    _case("rows before the per-row checks", L.SS_ERR_CAPACITY, B=65, beam=4, Tp=[0] * 65),
    _case("no encoder rows", L.SS_ERR_ARG, Tp=[0]),
    _case("prefix longer than max_len", L.SS_ERR_ARG, n_prefix=[3], max_len=[2]),
    _case("negative prefix length", L.SS_ERR_ARG, n_prefix=[-1], ids=[]),
    _case("min_len above max_len", L.SS_ERR_ARG, n_prefix=[0], max_len=[2], min_len=3),
    _case("prefix id past the vocabulary", L.SS_ERR_ARG, ids=[5, 6000]),
    _case("negative prefix id", L.SS_ERR_ARG, ids=[-1, 5]),
    _case("</s> inside a prefix", L.SS_ERR_ARG, ids=[5, 2]),
    _case("<pad> inside a prefix", L.SS_ERR_ARG, ids=[1, 5]),
    _case("</s> in a prefix before the capacity checks", L.SS_ERR_ARG, ids=[2, 5], feat_rows=3),
    _case("feature rows", L.SS_ERR_CAPACITY, feat_rows=10),
    _case("output stride", L.SS_ERR_CAPACITY, out_stride=10),
    _case("positions past the decoder's table", L.SS_ERR_CAPACITY, planner_max_tgt_pos=13),
    _case("positions past the model's table", L.SS_ERR_CAPACITY, max_len=[1023], feat_rows=1024, out_stride=1024),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c["name"] for c in REFUSALS])
def test_planner_refusals(case):
    from streamspeech_amd.engine import ContinueRefused, plan_mt_beam_continue
    with pytest.raises(ContinueRefused) as e:
        plan_mt_beam_continue([7 if t is None else t for t in case["Tp"]], case["n_prefix"], case["max_len"], case["beam"],
                              case.get("min_len", 1), feat_rows=case["feat_rows"], out_stride=case["out_stride"],
                              max_tgt_pos=case.get("planner_max_tgt_pos") or 1026, prefix_ids=case["ids"], vocab=6000, eos=2, pad=1)
    assert e.value.code == case["code"]


def test_planner_layout():
    from streamspeech_amd.engine import plan_mt_beam_continue, plan_mt_continue
    Tp, npre, mx, ids = [7, 3, 5], [2, 0, 4], [4, 6, 4], [11, 12, 13, 14, 15, 16]
    # beam 1: the rows of the greedy continuation -- same longest prefix, lock-step steps, prefix-pass rows, shifts and tables; the
    # cache is one row longer (the ancestry entry of the step after the last)
    p, q = plan_mt_beam_continue(Tp, npre, mx, 1, prefix_ids=ids), plan_mt_continue(Tp, npre, mx, 1, prefix_ids=ids)
    assert (p["S"], p["Tn"], p["Np"], p["Lc"]) == (q["S"], q["Tn"], q["Np"], q["Lcap"] + 1) and p["last_forced_in_prefix_pass"]
    assert p["shift"] == q["shift"] and p["r0"] == q["r0"] and p["last_row"] == q["last_row"]
    assert p["prefix_self"] == q["prefix_self"] and p["prefix_cross"] == q["prefix_cross"] and p["step_cross"] == q["step_cross"]
    assert p["prefix_tokens"] == q["prefix_tokens"] and p["prefix_pos"] == q["prefix_pos"]
    assert p["forced"] == [11, 12, -1, -1, 13, 14, 15, 16, -1]
    for b in range(3):                                  # the same cache rows, counted in rows of Lc instead of Lcap
        rows_p = [r - b * p["Lc"] for r, f in zip(p["cache_row"], p["feat_row"]) if f // p["feat_rows"] == b]
        rows_q = [r - b * q["Lcap"] for r, f in zip(q["cache_row"], q["feat_row"]) if f // q["feat_rows"] == b]
        assert rows_p == rows_q
    for t in range(q["Tn"]):                            # lock-step step t + 1 here feeds what the continuation's step t feeds
        assert [(s[1], s[2], s[3]) for s in p["step_self"][t + 1]] == [(s[1], s[2] - b * q["Lcap"], s[3])
                                                                      for b, s in enumerate(q["step_self"][t])]
    # beam 4: the last forced token is the first lock-step row of all k slots; forced positions live in slot 0 of the utterance
    p = plan_mt_beam_continue(Tp, npre, mx, 4, prefix_ids=ids)
    assert (p["S"], p["Tn"], p["Np"], p["R"], p["c0"], p["Lc"]) == (4, 6, 6, 12, 4, 12) and not p["last_forced_in_prefix_pass"]
    assert p["prefix_segments"] == 2 and p["prefix_self"] == [(0, 2, 0, 2), (2, 4, 2, 4)] and p["prefix_cross"] == [(0, 2, 0, 7), (2, 4, 10, 5)]
    assert p["prefix_tokens"] == [2, 11, 2, 13, 14, 15] and p["forced"] == [11, 12, 13, 14, 15, 16]
    assert p["shift"] == [2] * 4 + [4] * 4 + [0] * 4
    assert p["cache_row"] == [2, 3, 8 * 12, 8 * 12 + 1, 8 * 12 + 2, 8 * 12 + 3]
    assert p["step_self"][0][0] == (0, 1, 2, 3) and p["step_self"][0][4] == (4, 1, 4, 1) and p["step_self"][0][11] == (11, 1, 0, 5)
    assert p["step_cross"][5] == (5, 1, 7, 3)
    # no prefix anywhere: the tables of ss_batch_mt_beam (no shift, no prefix pass, cache index = position)
    p = plan_mt_beam_continue([4, 4], [0, 0], [3, 5], 4)
    assert (p["Np"], p["c0"], p["Lc"], p["prefix_segments"]) == (0, 0, 7, 0) and set(p["shift"]) == {0}
    assert p["step_self"][2][5] == (5, 1, 0, 3)


# ---- the pools -------------------------------------------------------------------------------------------------------------------------
class _StubPool:
    def reset(self, slot):
        pass

    def set_tail(self, slot, n):
        pass


class _PoolEngine:
    class cfg:
        max_target_positions, eos, pad, dec_dim, ctc_upsample = 1024, 2, 1, 8, 25
    device = "cpu"

    def __init__(self):
        self.calls = []

    def stream_pool(self, max_sessions, max_rows):
        return _StubPool()

    def batch_mt_continue(self, enc, Tp, prefixes, max_len, min_len=1):
        self.calls.append(("continue", len(Tp)))
        return [([9, 2], torch.zeros((len(p) + 2, 8))) for p in prefixes]

    def batch_mt_beam_continue(self, enc, Tp, prefixes, max_len, beam, min_len=1, unk_penalty=0.0, normalize=True):
        self.calls.append(("beam", len(Tp), beam))
        return ([[{"tokens": list(p) + [9 + i, 2], "score": -1.0 - i, "positional_scores": [0.0] * (len(p) + 2)} for i in range(beam)]
                 for p in prefixes], [torch.zeros((len(p) + 2, 8)) for p in prefixes])


@pytest.mark.parametrize("which", ["text", "speech"])
def test_pools_route_the_step_continuation(which):
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd.text_pool import TextSessionPool
    make = (lambda e, **kw: TextSessionPool(e, 80, 64, **kw)) if which == "text" else (lambda e, **kw: SpeechSessionPool(e, 80, 64, **kw))
    prefixes = [[5] * (b % 4) for b in range(70)]
    eng = _PoolEngine()
    pool = make(eng, beam_mt=4)
    res, groups = pool._mt_call(torch.zeros((70 * 3, 8)), [3] * 70, prefixes, [12] * 70)
    assert eng.calls == [("beam", 70, 4)]                                   # one continuation call for the step
    assert groups == [(0, 64), (64, 70)]                                    # 70 writers x 4 rows: 64 + 6, nobody refused
    assert [t for t, _ in res] == [[9, 2]] * 70                             # hypothesis 0's tokens after the prefix
    assert all(f.shape[0] == len(p) + 2 for (_, f), p in zip(res, prefixes))
    eng = _PoolEngine()
    pool = make(eng)                                                        # beam_mt = 1: the greedy continuation, as before
    assert pool.beam_mt == 1
    _, groups = pool._mt_call(torch.zeros((70 * 3, 8)), [3] * 70, prefixes, [12] * 70)
    assert eng.calls == [("continue", 70)] and groups == [(0, 70)]
    for bad in (0, 33):
        with pytest.raises(ValueError):
            make(_PoolEngine(), beam_mt=bad)


def test_engine_splits_a_forced_beam_call_at_256_rows(monkeypatch):
    """HipModel.batch_mt_beam_continue makes the sub-calls of plan_beam_groups: 70 rows at beam 4 -> 64 + 6 utterances."""
    from streamspeech_amd import engine as E

    class Lib:
        def __init__(self):
            self.B = []

        def ss_batch_mt_beam_continue(self, h, stream, B, beam, enc, Tp, pre, npre, mx, min_len, unk, norm, out, stride, n_out, sc, pos,
                                      feats, rows):
            self.B.append(B)
            for o in range(B * beam):
                n_out[o], out[o * stride], sc[o] = 1, 2, -float(o % beam)
            return 0

    class M(E.BatchMixin):
        class cfg:
            dec_dim = 8
        device, h, lib = "cpu", None, Lib()
    monkeypatch.setattr(E, "_stream", lambda: None)
    monkeypatch.setattr(E, "_ptr", lambda t: None)
    m = M()
    nbest, feats = m.batch_mt_beam_continue(torch.zeros((210, 8)), [3] * 70, [[5] * (b % 3) for b in range(70)], [6] * 70, 4)
    assert m.lib.B == [64, 6] and len(nbest) == 70 and all(len(h) == 4 for h in nbest)
    assert nbest[5][0]["tokens"] == [5, 5, 2] and feats[5].shape[0] == 3


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------
def _reference_available():
    from oracle import ref_loader
    return os.path.isdir(ref_loader.REF)


def test_fixture_shape():
    from tests import make_golden_beam_prefix as M
    fix = json.load(open(M.OUT, encoding="utf-8"))
    assert os.path.getsize(M.OUT) < 110 * 1024
    assert set(fix["groups"]) == {"beam4", "beam10_early_eos", "beam5_unnorm_unkpen"}
    full = unk = 0
    for name, grp in fix["groups"].items():
        for kind in ("on", "off"):
            assert sum(c["margin"] > c["tau"] for c in grp["cases"][kind]) >= 6, f"{name}/{kind}"
        on = {c["sid"]: c for c in grp["cases"]["on"]}
        for c in grp["cases"]["off"]:                   # an off-path prefix forces a token the unforced best path does not have there
            assert c["prefix"][:2] == on[c["sid"]]["prefix"][:2] and c["prefix"] != on[c["sid"]]["prefix"], f"{name} sample {c['sid']}"
            assert [h["tokens"] for h in c["nbest"]] != [h["tokens"] for h in on[c["sid"]]["nbest"]]
        for kind, cases in grp["cases"].items():
            for c in cases:
                assert all(h["tokens"][:len(c["prefix"])] == c["prefix"] for h in c["nbest"])
                assert all(len(h["positional_scores"]) == len(h["tokens"]) for h in c["nbest"])
                pinned = c["margin"] > c["tau"]
                full += pinned and len(c["prefix"]) == grp["max_len_b_mt"]
                unk += pinned and 3 in c["prefix"] and grp["unk_penalty"] != 0
    assert full >= 1 and unk >= 1
    assert len({len(h["tokens"]) for h in fix["groups"]["beam10_early_eos"]["cases"]["off"][0]["nbest"]}) > 1


@pytest.mark.skipif(not _reference_available(), reason="the reference tree is not present")
def test_fixture_is_what_the_reference_prints_now():
    import numpy as np
    from oracle import kaldi_fbank as K
    from streamspeech_amd.config import ModelConfig
    from tests import make_golden_beam as G, make_golden_beam_prefix as M
    fix = json.load(open(M.OUT, encoding="utf-8"))
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    for name, kind in (("beam4", "off"), ("beam10_early_eos", "on")):
        grp = fix["groups"][name]
        gen, _, _ = G.build_generator(G.state_dict(grp["eos_scale"], cfg), cfg, grp["beam"], grp["max_len_b_mt"], grp["unk_penalty"],
                                      grp["normalize"])
        rec = grp["cases"][kind][0]
        fb = K.global_cmvn(K.fbank(G.sample_pcm(rec["pcm_seed"], rec["n_samples"]) * np.float32(32768.0)), g["mean"], g["std"])
        now = M.run(gen, rec["sid"], fb, grp["beam"], rec["prefix"])
        assert [h["tokens"] for h in now["nbest"]] == [h["tokens"] for h in rec["nbest"]]
        assert np.allclose([h["score"] for h in now["nbest"]], [h["score"] for h in rec["nbest"]], atol=1e-5)
        assert abs(now["margin"] - rec["margin"]) < 1e-5
