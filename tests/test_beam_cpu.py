"""Host side of the offline beam search: the driver's search flags (pred.offline-s2st.sh passes --beam-mt $BEAM --beam 1), the
routing of offline.generate to batch_mt_beam / batch_mt_greedy, the planner that keeps every ss_batch_mt_beam call at
B * beam <= 256 rows, and the committed fixture against the reference generator when the reference tree is present."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parser_accepts_the_reference_search_flags():
    from streamspeech_amd.offline import build_parser
    a = build_parser().parse_args(["--path", "synthetic:0", "--vocoder", "v", "--results-path", "r",
                                   "--beam-mt", "5", "--beam", "1", "--unkpen", "0.5", "--unnormalized"])
    assert (a.beam_mt, a.beam, a.unkpen, a.unnormalized) == (5, 1, 0.5, True)
    d = build_parser().parse_args(["--path", "p", "--vocoder", "v", "--results-path", "r"])
    assert (d.beam_mt, d.beam, d.unkpen, d.unnormalized) == (1, 1, 0.0, False)


@pytest.mark.parametrize("flag", [["--match-source-len"], ["--temperature", "0.5"]])
def test_parser_rejects_options_the_recipe_does_not_pass(flag):
    from streamspeech_amd.offline import build_parser
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--path", "p", "--vocoder", "v", "--results-path", "r"] + flag)


class StandIn:
    """Records which first-pass search offline.generate asks for; every other stage returns fixed small outputs."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.calls = []

    def batch_fbank_cmvn(self, pcm, lens):
        T = [n // 160 for n in lens]
        return torch.zeros(sum(T), 80), T

    def batch_encoder_forward(self, feat, T):
        Tp = [t // 4 for t in T]
        return torch.zeros(sum(Tp), self.cfg.enc_dim), Tp

    def batch_ctc_greedy(self, head, enc, Tp):
        return [([10 + head], [0]) for _ in Tp]

    def _feats(self, B):
        return torch.zeros(B, 4, self.cfg.dec_dim)

    def batch_mt_greedy(self, enc, Tp, mx, min_len=1):
        self.calls.append(("greedy", list(mx), min_len))
        return [[20, 21, self.cfg.eos] for _ in Tp], self._feats(len(Tp)), [3] * len(Tp)

    def batch_mt_beam(self, enc, Tp, mx, beam, min_len=1, unk_penalty=0.0, normalize=True):
        self.calls.append(("beam", list(mx), beam, min_len, unk_penalty, normalize))
        nb = [[{"tokens": [30, 31, self.cfg.eos], "score": -1.0, "positional_scores": [-0.5, -0.25, -0.25]},
               {"tokens": [32, self.cfg.eos], "score": -2.0, "positional_scores": [-1.0, -3.0]}] for _ in Tp]
        return nb, self._feats(len(Tp)), [3] * len(Tp)

    def batch_t2u_units(self, feats, n, t2u_causal=False, mask_eos=False):
        return [[] for _ in n]


def _run(tmp_path, **kw):
    from streamspeech_amd import offline
    from streamspeech_amd.config import ModelConfig
    from oracle.ref_agent import make_dicts
    cfg = ModelConfig()
    m = StandIn(cfg)
    items = [(4, torch.zeros(16000)), (9, torch.zeros(24000))]
    hyps = offline.generate(m, None, items, make_dicts(cfg), str(tmp_path), max_len_b_mt=12, dump_wav=False, **kw)
    return m, hyps, make_dicts(cfg)


def test_generate_routes_beam_mt_to_the_beam_search(tmp_path):
    m, hyps, dicts = _run(tmp_path, beam_mt=5, unk_penalty=0.5, normalize=False)
    assert m.calls == [("beam", [12, 12], 5, 1, 0.5, False)]
    # the D- text is hypothesis 0 of the n-best list
    from streamspeech_amd.offline import detok
    assert hyps[4]["mt"] == detok([dicts["target_unigram"][c] for c in (30, 31)])


def test_generate_beam_mt_1_stays_greedy(tmp_path):
    m, hyps, dicts = _run(tmp_path)
    assert m.calls == [("greedy", [12, 12], 1)]
    m, _, _ = _run(tmp_path / "b1", beam_mt=1, unk_penalty=0.5)
    assert [c[0] for c in m.calls] == ["greedy"]


@pytest.mark.parametrize("B,beam", [(1, 1), (256, 1), (257, 1), (30, 10), (25, 10), (100, 32), (7, 32), (64, 4), (65, 4)])
def test_split_planner_bounds_rows_and_keeps_order(B, beam):
    from streamspeech_amd.engine import plan_beam_groups
    g = plan_beam_groups(B, beam)
    assert all((e - s) * beam <= 256 and e > s for s, e in g)
    assert [i for s, e in g for i in range(s, e)] == list(range(B))
    assert len(g) == -(-B // (256 // beam))


def test_split_planner_refuses_bad_beams():
    from streamspeech_amd.engine import plan_beam_groups
    for beam in (0, 257):
        with pytest.raises(ValueError):
            plan_beam_groups(4, beam)


def _reference_available():
    from oracle import ref_loader
    return os.path.isdir(ref_loader.REF)


@pytest.mark.skipif(not _reference_available(), reason="the reference tree is not present")
def test_fixture_is_what_the_reference_prints_now():
    import numpy as np
    from oracle import kaldi_fbank as K
    from streamspeech_amd.config import ModelConfig
    from tests import make_golden_beam as M
    fix = json.load(open(M.OUT, encoding="utf-8"))
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    for name, grp in fix["groups"].items():
        gen, _, dicts = M.build_generator(M.state_dict(grp["eos_scale"], cfg), cfg, grp["beam"], grp["max_len_b_mt"],
                                          grp["unk_penalty"], grp["normalize"])
        sid, rec = next(iter(grp["hypotheses"].items()))
        fb = K.global_cmvn(K.fbank(M.sample_pcm(rec["pcm_seed"], rec["n_samples"]) * np.float32(32768.0)), g["mean"], g["std"])
        now = M.run(gen, dicts, int(sid), fb, grp["beam"])
        assert now["log"] == rec["log"] and now["units"] == rec["units"]
        assert [h["tokens"] for h in now["nbest"]] == [h["tokens"] for h in rec["nbest"]]
        assert np.allclose([h["score"] for h in now["nbest"]], [h["score"] for h in rec["nbest"]], atol=1e-5)
