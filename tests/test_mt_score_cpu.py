"""Scoring a given translation with the first-pass text decoder, the parts that need no GPU: the float64 reference of the token
score kernel (tests/mt_score_ref.py) against torch, its float32 twin against it, generators.SequenceScorer and
words.words_from_scores on a stand-in engine, the offline driver's --score-reference / --speak-reference on a stand-in model, the new
symbols, and the fixture tests/golden/mt_score.npz (and, where the reference tree exists, its regeneration)."""
import math
import os

import numpy as np
import pytest
import torch

from tests import mt_score_ref as R
from streamspeech_amd.words import ScoredWord, words_from_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mt_score.npz")

_DATA = {}


def _case(name):
    """(case, logits [rows, ld], targets, float64 reference) of a shared op case, computed once."""
    if name not in _DATA:
        c = R.op_cases()[name]
        x, tgt = R.case_data(c, name)
        _DATA[name] = (c, x, tgt, R.score_ref(np.ascontiguousarray(x[:, :c["V"]]), tgt))
    return _DATA[name]


def test_cases_cover_what_they_promise():
    cs = R.op_cases()
    assert {c["V"] for c in cs.values()} >= set(R.WIDTHS) and {c["rows"] for c in cs.values()} >= {1, 5, 300}
    assert any(c["ld"] > c["V"] for c in cs.values()) and {c["scale"] for c in cs.values()} >= {1.0, 40.0}
    assert {c["shift"] for c in cs.values()} >= {-80.0, 80.0} and max(c["rows"] for c in cs.values()) > 65535
    c, x, tgt, ref = _case("edge1005")
    assert ref["bad"].tolist() == [r in (7, 11, 13) for r in range(15)] and ref["skip"].tolist() == [r == 9 for r in range(15)]
    assert np.isneginf(ref["target"][5]) and not ref["bad"][5] and ref["rank"][5] == 1005 - 3 + 1       # a -inf target: below all finite ones
    assert np.isneginf(x[3, :1005]).sum() == 335 and np.isfinite(ref["target"][3])
    c, x, tgt, ref = _case("ties1005")
    assert ref["rank"][3] == 1 and ref["argmax"][3] < tgt[3] and x[3, ref["argmax"][3]] == x[3, tgt[3]]   # two maxima, target the later
    v = x[5, tgt[5]]
    assert (x[5, :tgt[5]] == v).sum() == 1 and (x[5, tgt[5] + 1:1005] == v).sum() == 1 and v < x[5, :1005].max()
    c, x, tgt, ref = _case("ld")
    assert np.isnan(x[:, 1005:]).all()
    for name in cs:                                              # |value| < 256 everywhere: what TOL = 2e-5 needs (module docstring)
        r = _case(name)[3]
        ok = ~(r["bad"] | r["skip"]) & np.isfinite(r["target"])
        assert np.abs(r["target"][ok]).max() < 256 and tgt.dtype == np.int32, name


@pytest.mark.parametrize("name", [n for n in R.op_cases() if n != "rows70000"])
def test_reference_against_torch(name):
    """log_softmax(x.double()).gather, torch.max (the first maximum) and a sort-based rank; the explicit scan on some rows."""
    c, x, tgt, ref = _case(name)
    V = c["V"]
    xt = torch.from_numpy(np.ascontiguousarray(x[:, :V]))
    good = ~(ref["bad"] | ref["skip"])
    assert good.sum() >= 1
    for r in np.nonzero(good)[0]:
        row, tk = xt[r], int(tgt[r])
        lsm = torch.log_softmax(row.double(), 0)
        want_t, want_b = float(lsm[tk]), float(lsm.max())
        for got, want in ((ref["target"][r], want_t), (ref["best"][r], want_b)):
            assert got == want or abs(got - want) < 1e-12, (name, r)
        assert int(ref["argmax"][r]) == int(torch.max(row, 0).indices)
        order = sorted(range(V), key=lambda n: (-float(row[n]), n)) if V <= 1005 else None      # descending, ties by index
        if order is not None:
            assert order.index(tk) == int(ref["rank"][r]), (name, r)
        else:
            st = torch.sort(row, descending=True, stable=True)
            assert int((st.indices == tk).nonzero()[0, 0]) == int(ref["rank"][r]), (name, r)
    for r in list(np.nonzero(good)[0][:4]) + list(np.nonzero(good)[0][-2:]):
        assert R.scan_row(x[r, :V].tolist(), int(tgt[r])) == (int(ref["argmax"][r]), int(ref["rank"][r])), (name, r)
    for r in np.nonzero(ref["bad"])[0]:
        assert math.isnan(ref["target"][r]) and math.isnan(ref["best"][r]) and ref["argmax"][r] == -1 and ref["rank"][r] == -1


@pytest.mark.parametrize("name", list(R.op_cases()))
def test_float32_twin_within_tol(name):
    """The float32 arithmetic in the kernel's summation order stays within 2e-5 of float64 on every case."""
    c, x, tgt, ref = _case(name)
    t32, b32 = R.score_f32(np.ascontiguousarray(x[:, :c["V"]]), tgt)
    assert t32.dtype == np.float32 and b32.dtype == np.float32
    good = ~(ref["bad"] | ref["skip"])
    assert np.isnan(t32[ref["bad"]]).all() and np.isnan(b32[ref["bad"]]).all()
    fin = good & np.isfinite(ref["target"])
    assert np.array_equal(np.isneginf(t32[good]), np.isneginf(ref["target"][good]))
    e_t = np.abs(t32[fin].astype(np.float64) - ref["target"][fin]).max()
    e_b = np.abs(b32[good].astype(np.float64) - ref["best"][good]).max()
    assert e_t <= R.TOL and e_b <= R.TOL, (name, e_t, e_b)


def test_search_utterances_are_decisive_on_the_oracle():
    """The utterances of the GPU consistency test, on the CPU oracle alone: teacher-forced over its own greedy hypothesis the only
    token that is not the plain arg-max is the first one, behind </s> (banned below min_len 1), and everywhere the top-2 gap is far
    beyond what float32 can blur -- the GPU test's cap of one undecidable position an utterance is not needed by the reference."""
    from oracle import streamspeech_oracle as O
    from oracle.engine import OracleEngine
    from streamspeech_amd import synth
    from streamspeech_amd.config import ModelConfig
    cfg = ModelConfig()
    eng = OracleEngine(synth.make_model_state_dict(0, cfg), cfg)
    E = eng.sd["target_unigram_decoder.output_projection.weight"]
    for seed, T in R.SEARCH_UTTS:
        enc = eng.encoder_forward(torch.from_numpy(synth.synth_fbank(seed, T)), 8, 8)
        hyp = [t for t in O.mt_greedy(eng.sd, enc, cfg, max_new_tokens=R.SEARCH_MAX_LEN) if t != cfg.eos]
        assert len(hyp) >= 4
        feats = O.mt_decoder_features(eng.sd, [cfg.eos] + hyp, enc, cfg)[:len(hyp)]
        x = torch.nn.functional.linear(feats, E).numpy().astype(np.float32)
        ref = R.score_ref(x, np.asarray(hyp))
        assert ref["rank"].tolist() == [1] + [0] * (len(hyp) - 1) and int(ref["argmax"][0]) == cfg.eos, (seed, ref["rank"])
        top2 = torch.from_numpy(x).double().log_softmax(-1).topk(2, -1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) > 1.0


# ---- the Python layers -------------------------------------------------------------------------------------------------------------
class _Syms:
    def __init__(self, table):
        self.t = table

    def __getitem__(self, i):
        return self.t[int(i)]


SYM = ["<s>", "<pad>", "</s>", "<unk>", "▁he", "llo", "▁wor", "ld", "▁x", "tail"]


def test_words_from_scores():
    syms = _Syms(SYM)
    toks = [9, 4, 5, 6, 7, 8, 2]
    pos = [-0.5, -1.0, -0.25, -2.0, -0.5, -0.125, -3.0]
    rank = [0, 2, 0, 1, 5, 0, 0]
    w = words_from_scores(toks, pos, rank, syms)
    assert w == [ScoredWord("tail", 1, -0.5, math.exp(-0.5), -0.5, 0), ScoredWord("hello", 2, -1.25, math.exp(-0.625), -1.0, 1),
                 ScoredWord("world", 2, -2.5, math.exp(-1.25), -2.0, 2), ScoredWord("x", 1, -0.125, math.exp(-0.125), -0.125, 0)]
    assert words_from_scores(toks, pos, rank, syms, eos=2) == w
    assert words_from_scores([], [], [], syms) == [] and words_from_scores([2], [-1.0], [0], syms) == []     # the empty text
    assert math.isnan(words_from_scores([4], [float("nan")], [-1], syms)[0].confidence)
    with pytest.raises(ValueError):
        words_from_scores([4, 5], [-1.0], [0, 0], syms)


class _Dict:
    def pad(self):
        return 1

    def eos(self):
        return 2

    def unk(self):
        return 3


class _Engine:
    """batch_mt_score, canned: position p of a text scores -(p + 1) / 4 - its token / 64."""

    def __init__(self):
        self.calls = []

    def batch_mt_score(self, enc, Tp, tokens, src=None, want_feats=False):
        self.calls.append((tuple(enc.shape), list(Tp), [list(t) for t in tokens], src))
        out = []
        for t in tokens:
            full = list(t) + [2]
            pos = torch.tensor([-(p + 1) / 4 - tok / 64 for p, tok in enumerate(full)], dtype=torch.float32)
            out.append({"positional_scores": pos, "score": float(pos.sum()) / len(full), "best": torch.zeros(len(full), dtype=torch.int32),
                        "best_lprob": pos, "rank": torch.ones(len(full), dtype=torch.int32), "feats": None})
        return out


def test_sequence_scorer_surface():
    """fairseq's surface: padded targets that end in </s>, one hypothesis list per sample, </s> counted in `score`, the empty text."""
    from streamspeech_amd.generators import SequenceScorer
    eng = _Engine()
    sc = SequenceScorer(_Dict(), engine=eng)
    target = torch.tensor([[7, 8, 9, 2], [2, 1, 1, 1], [5, 2, 1, 1]])
    encs = [{"encoder_out": [torch.zeros(3 + b, 1, 4)]} for b in range(3)]
    out = sc.generate([object()], {"target": target, "encoder_out": encs})
    assert len(eng.calls) == 1 and eng.calls[0] == ((3 + 4 + 5, 4), [3, 4, 5], [[7, 8, 9], [], [5]], None)
    assert [len(h) for h in out] == [1, 1, 1]
    for h, want in zip(out, ([7, 8, 9, 2], [2], [5, 2])):
        h = h[0]
        assert sorted(h) == ["alignment", "attention", "positional_scores", "score", "tokens"]
        assert h["tokens"].tolist() == want and h["attention"] is None and h["alignment"] is None
        assert h["positional_scores"].shape == (len(want),) and h["positional_scores"].dtype == torch.float32
        assert abs(h["score"] - float(h["positional_scores"].sum()) / len(want)) < 1e-7               # </s> counted
    assert abs(out[1][0]["score"] - (-0.25 - 2 / 64)) < 1e-7                                           # the empty text: only </s>

    class Model:                                                 # the model wrapper's encoder surface
        def __init__(self):
            self.seen = []

        def encoder(self, src_tokens, src_lengths=None):
            self.seen.append(tuple(src_tokens.shape))
            return {"encoder_out": [torch.zeros(src_tokens.shape[1] // 4, 1, 4)]}
    m = Model()
    src = torch.zeros(2, 40, 80)
    out2 = sc.generate([m], {"target": target[:2], "net_input": {"src_tokens": src, "src_lengths": torch.tensor([40, 24])}})
    assert m.seen == [(1, 40, 80), (1, 24, 80)] and eng.calls[-1][1] == [10, 6] and len(out2) == 2
    with pytest.raises(ValueError, match="</s>"):
        sc.generate([m], {"target": torch.tensor([[7, 8, 1]]), "encoder_out": encs[:1]})
    with pytest.raises(ValueError):
        SequenceScorer(_Dict())
    with pytest.raises(ValueError, match="ensembles"):
        sc.generate([m, m], {"target": target, "encoder_out": encs})


class _OffModel:
    """The offline driver's model calls, canned (as tests/test_multispkr_cpu.py): every utterance decodes to [</s>] and three units;
    batch_mt_score scores position p of a text with -(p + 1) / 8 and rank p % 2."""
    class cfg:
        max_target_positions, eos, pad, tgt_vocab, dec_dim = 1024, 2, 1, 20, 4
    max_tgt_pos = 40

    def __init__(self):
        self.score_calls, self.unit_calls = [], []

    def batch_fbank_cmvn(self, pcm, n):
        return None, [10] * len(n)

    def batch_encoder_forward(self, feat, T):
        return torch.zeros(3 * len(T), 4), [3] * len(T)

    def batch_ctc_greedy(self, head, enc, Tp):
        return [([], None)] * len(Tp)

    def batch_mt_greedy(self, enc, Tp, mx):
        return [[2]] * len(Tp), None, [1] * len(Tp)

    def batch_t2u_units(self, feats, n, t2u_causal=False, mask_eos=True):
        self.unit_calls.append((None if feats is None else tuple(feats.shape), list(n)))
        return [[4 + 7, 4 + 8, 4 + 9][:3 if feats is None else k] for k in n]

    def batch_mt_score(self, enc, Tp, tokens, src=None, want_feats=False):
        self.score_calls.append((tuple(enc.shape), list(Tp), [list(t) for t in tokens], want_feats))
        out = []
        for t in tokens:
            n = len(t) + 1
            pos = torch.tensor([-(p + 1) / 8 for p in range(n)], dtype=torch.float32)
            out.append({"positional_scores": pos, "score": float(pos.sum()) / n, "best": torch.zeros(n, dtype=torch.int32),
                        "best_lprob": pos, "rank": torch.tensor([p % 2 for p in range(n)], dtype=torch.int32),
                        "feats": torch.zeros(n, 4) if want_feats else None})
        return out


class _Voc:
    num_speakers = 0

    def __init__(self):
        self.calls = []

    def batch_forward(self, codes, dur_prediction=True, **kw):
        self.calls.append(([list(c) for c in codes], dur_prediction, kw))
        return [torch.full((len(c) * 320,), 0.25) for c in codes], None, [len(c) for c in codes]


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_offline_score_and_speak_reference(tmp_path, monkeypatch):
    """The two files' formats and every status; with neither flag the files are those of a run of the same stand-in without them;
    --speak-reference lays ref_wav/ and .ref.unit out as pred_wav/ and .unit are."""
    from streamspeech_amd import offline
    from streamspeech_amd.modules import Dictionary
    monkeypatch.setattr(offline, "units_from_tokens", lambda t, cfg: [c - 4 for c in t])
    d = Dictionary.placeholder(20)
    dicts = {"source_unigram": d, "ctc_target_unigram": d, "target_unigram": d}
    # ids 10 .. 15: scored (3 pieces, 2 words), the empty text, no reference, an id outside the dictionary, too long, no audio
    items = [(10 + i, torch.zeros(800 + i)) for i in range(5)] + [(15, torch.zeros(100))]
    refs = {10: [d.index("▁w5"), d.index("▁w6"), 3], 11: [], 13: [5, 20], 14: [5] * 38, 15: [5]}
    assert 20 >= _OffModel.cfg.tgt_vocab
    offline.generate(_OffModel(), _Voc(), items, dicts, str(tmp_path / "plain"), batch_size=8)
    m, voc = _OffModel(), _Voc()
    offline.generate(m, voc, items, dicts, str(tmp_path / "score"), batch_size=8, mt_references=refs)
    a, b = _tree(tmp_path / "plain"), _tree(tmp_path / "score")
    assert set(b) - set(a) == {"generate-test.mt.ref.scores", "generate-test.mt.ref.words"} and all(a[k] == b[k] for k in a)
    # one call per batch over the usable rows, in the batch's (length-sorted) order: ids 11 and 10
    assert len(m.score_calls) == 1 and m.score_calls[0] == ((6, 4), [3, 3], [[], refs[10]], False)
    assert len(voc.calls) == 1 and len(m.unit_calls) == 1                                               # the hypotheses' calls only
    rows = [ln.split("\t") for ln in b["generate-test.mt.ref.scores"].decode().splitlines()]
    assert all(len(r) == 6 for r in rows) and [r[0] for r in rows] == [str(i) for i in range(10, 16)]
    assert [r[5] for r in rows] == ["scored", "scored", "no_reference", "invalid_label", "too_long", "no_audio"]
    assert [int(r[1]) for r in rows] == [4, 1, 0, 3, 39, 2]
    sid, n, score, total, acc, _ = rows[0]
    assert float(total) == pytest.approx(-(1 + 2 + 3 + 4) / 8) and float(score) == pytest.approx(float(total) / 4) and float(acc) == 0.5
    assert (float(rows[1][2]), float(rows[1][3]), float(rows[1][4])) == (-0.125, -0.125, 1.0)            # only </s>
    assert all(math.isnan(float(r[2])) and math.isnan(float(r[3])) and math.isnan(float(r[4])) for r in rows[2:])
    words = [ln.split("\t") for ln in b["generate-test.mt.ref.words"].decode().splitlines()]
    assert [w[:3] for w in words] == [["10", "w5", "1"], ["10", "w6<unk>", "2"]] and all(len(w) == 7 for w in words)
    assert float(words[1][3]) == pytest.approx(-5 / 8) and float(words[1][4]) == pytest.approx(math.exp(-5 / 16), rel=1e-5)
    assert float(words[1][5]) == pytest.approx(-3 / 8) and [w[6] for w in words] == ["0", "1"]
    # --speak-reference
    m, voc = _OffModel(), _Voc()
    offline.generate(m, voc, items, dicts, str(tmp_path / "speak"), batch_size=8, mt_references=refs, speak_reference=True,
                     dur_prediction=False)
    c = _tree(tmp_path / "speak")
    assert m.score_calls[0][3] is True and m.unit_calls[1] == ((2, 4, 4), [1, 4])      # the reference rows' states, after the hypotheses'
    assert len(voc.calls) == 2 and voc.calls[0] == ([[7], [7, 8, 9]], False, {})       # the existing call, dur_prediction honoured
    assert set(c) - set(b) == {"generate-test.ref.unit", os.path.join("ref_wav", "0_pred.wav"), os.path.join("ref_wav", "1_pred.wav")}
    assert c["generate-test.mt.ref.scores"] == b["generate-test.mt.ref.scores"]
    unit_lines = c["generate-test.ref.unit"].decode().split("\n")
    assert len(unit_lines) == 7 and unit_lines[0] == "7 8 9" and unit_lines[1] == "7" and unit_lines[2:] == [""] * 5
    assert len(c[os.path.join("ref_wav", "0_pred.wav")]) >= 2 * 3 * 320 > len(c[os.path.join("ref_wav", "1_pred.wav")]) >= 2 * 320
    assert os.path.join("pred_wav", "0_pred.wav") in c
    with pytest.raises(ValueError, match="mt_references"):
        offline.generate(_OffModel(), _Voc(), items, dicts, str(tmp_path / "x"), speak_reference=True)


def test_load_mt_references(tmp_path):
    from streamspeech_amd import offline
    from streamspeech_amd.modules import Dictionary
    data = tmp_path / "data"
    (data / "target_unigram").mkdir(parents=True)
    (data / "target_unigram" / "test.tsv").write_text("id\ttgt_text\nutt_a\t▁w1 ▁w2 nowhere\nutt_b\t\n", encoding="utf-8")
    (data / "test.tsv").write_text("id\tsrc_audio\tsrc_n_frames\nutt_a\ta.wav\t1\nutt_b\tb.wav\t1\nutt_z\tz.wav\t1\n")
    (data / "mt.yaml").write_text("target_unigram:\n  decoder_type: transformer\n  data: /another/machine/target_unigram\n")
    dicts = {"target_unigram": Dictionary.placeholder(10)}
    assert offline.load_mt_references(str(data), "mt.yaml", "test", dicts) == {0: [5, 6, 3], 1: []}
    (data / "none.yaml").write_text("target_unigram:\n  decoder_type: transformer\n")
    assert offline.load_mt_references(str(data), "none.yaml", "test", dicts) is None


def test_score_reference_refusals(tmp_path, capsys):
    """The refusals --align-reference makes, before anything is loaded."""
    from streamspeech_amd import offline
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", str(tmp_path / "out")]
    p = offline.build_parser()
    assert p.parse_args(base).score_reference is False and p.parse_args(base).speak_reference is False
    (tmp_path / "none.yaml").write_text("target_unigram:\n  decoder_type: transformer\n")
    for flag in ("--score-reference", "--speak-reference"):
        for extra in (["--synthetic", "2"], ["--wav-list", str(tmp_path / "list.txt")], [str(tmp_path)],
                      [str(tmp_path), "--multitask-config-yaml", "none.yaml"]):
            with pytest.raises(SystemExit) as e:
                offline.main(base + [flag] + extra)
            assert e.value.code == 2
            assert "--score-reference" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_new_symbols_exported_and_prototyped():
    from streamspeech_amd import lib as L
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    for name, nargs in (("ss_batch_mt_score", 13), ("ss_op_mt_token_scores", 8), ("ss_debug_mt_score_form", 1)):
        assert f"int {name}(" in hdr and hasattr(lib, name)
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert name in hdr.split("#ifndef STREAMSPEECH_HIP_H")[0], f"{name} is not in the header's list of additions since ABI 2"
    assert lib.ss_abi_version() == 2
    import ctypes as C
    assert lib.ss_op_mt_token_scores(None, None, 8, 1, 8, None, None, None) == L.SS_ERR_ARG            # refused on the host: no GPU needed
    one = C.c_void_p(16)
    assert lib.ss_op_mt_token_scores(None, one, 7, 1, 8, one, one, one) == L.SS_ERR_ARG                # ld < V
    assert lib.ss_op_mt_token_scores(None, one, 8, 0, 8, one, one, one) == L.SS_ERR_ARG
    assert lib.ss_op_mt_token_scores(None, one, 8, 16777216, 8, one, one, one) == L.SS_ERR_ARG         # past the stated row limit


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_fixture_shapes():
    g = np.load(GOLD)
    assert int(g["n"]) == 4 and os.path.getsize(GOLD) < (1 << 19)
    for u in range(4):
        assert g[f"fbank{u}"].dtype == np.float32 and g[f"fbank{u}"].shape[1] == 80
        for k in range(3):
            toks, p32, p64 = g[f"tokens{u}_{k}"], g[f"pos32_{u}_{k}"], g[f"pos64_{u}_{k}"]
            assert toks.dtype == np.int32 and toks[-1] == 2 and (toks[:-1] != 1).all()
            assert p32.dtype == p64.dtype == np.float32 and p32.shape == p64.shape == toks.shape and (p64 < 0).all()
            for p, s in ((p32, g[f"score32_{u}_{k}"]), (p64, g[f"score64_{u}_{k}"])):
                assert abs(float(s) - float(p.astype(np.float64).sum()) / len(toks)) < 1e-5              # </s> counted
        assert len(g[f"tokens{u}_1"]) == 18 and len(g[f"tokens{u}_2"]) == 1
        assert g[f"score64_{u}_1"] < g[f"score64_{u}_0"]                                                # the random text is the unlikely one


def test_fixture_regenerates():
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("no reference tree")
    from tests import make_golden_mt_score as M
    new, g = M.generate(), np.load(GOLD)
    assert sorted(new) == sorted(g.files)
    for k in g.files:                     # tokens and shapes exactly; the float arrays to 1e-5 absolute: the reference's float32 GEMMs
        assert np.asarray(new[k]).dtype == g[k].dtype and np.asarray(new[k]).shape == g[k].shape, k      # sum in a BLAS-thread-count order
        if k.startswith(("pos", "score", "fbank")):
            assert np.abs(np.asarray(new[k], dtype=np.float64) - g[k].astype(np.float64)).max() <= 1e-5 * max(1.0, np.abs(g[k]).max()), k
        else:
            assert np.array_equal(new[k], g[k]), k
