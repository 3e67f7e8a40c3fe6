"""Lexically constrained beam search on the GPU (csrc/beam_kernels.hip: beam_topk_cons_kernel, beam_merge_cons_kernel,
beam_cons_select_kernel; ss_batch_mt_beam_cons).

Op level: the selection kernel through ss_op_beam_cons_select against the restatement of the rule in tests/constraint_ref.py, on the
sizes of the host twin's test (tests/test_mt_constraints_cpu.py), every output compared, scores bit for bit.
Search level, on the synthetic checkpoint: the fixture tests/golden/mt_constraints.json (the reference's generator with its own
LexicallyConstrainedBeamSearch, tests/make_golden_mt_constraints.py) through the engine -- identical n-best tokens and order, scores
within tau / 4, positional scores within tau, the bounds of tests/test_beam_gpu.py -- every phrase in every hypothesis, an utterance
alone against the same utterance in the mixed pack, the call without phrases against ss_batch_mt_beam_opts, the refusals, and the
offline driver."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import constraint_ref as CR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "mt_constraints.json")
CAND = 64
SENT = -7
PAD, UNK, EOS = 1, 3, 2
SS_ERR_ARG = 2


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def df(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), np.float32)).cuda()


def di(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), np.int32)).cuda()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _pack(phrases_per_utt):
    from streamspeech_amd.lib import pack_constraints
    return pack_constraints(phrases_per_utt, len(phrases_per_utt))


def _table(lib, phrases_per_utt, V):
    from streamspeech_amd.lib import MT_CONS_TABLE_LD
    toks, off, ends = _pack(phrases_per_utt)
    tab = np.zeros(len(phrases_per_utt) * MT_CONS_TABLE_LD, np.int32)
    p32 = C.POINTER(C.c_int32)
    rc = lib.ss_mt_cons_table_host(len(phrases_per_utt), toks.ctypes.data_as(p32), off.ctypes.data_as(p32), ends.ctypes.data_as(p32),
                                   V, -1, EOS, None, tab.ctypes.data_as(p32))
    assert rc == 0
    return tab


# ---- op level -----------------------------------------------------------------------------------------------------------------------
def _utterance(rng, k, V, C_, step, ties, neg_inf):
    """One utterance of a step: phrases summing to C_ tokens, states, and the rows as the top-2k kernel sees them after step 1 of
    the rule and + cum (the restatement applies both itself)."""
    toks = [int(t) for t in rng.choice([t for t in range(V) if t != EOS], C_, replace=C_ > V - 1)] if C_ else []
    phrases, o = [], 0
    while o < C_:
        n = int(min(C_ - o, rng.integers(1, 5)))
        phrases.append(toks[o:o + n])
        o += n
    states = [-1] * k if step == 0 else [int(s) for s in rng.integers(-1, C_, k)]
    lp = (-rng.random((k, V)) * 8).astype(np.float32)
    if ties:
        lp = (np.round(lp * 2) / 2).astype(np.float32)
    if neg_inf:
        lp[rng.random((k, V)) < (0.9 if neg_inf > 1 else 0.2)] = -np.inf
    cum = (np.round(-rng.random(k) * 12) if ties else -rng.random(k) * 12).astype(np.float32)
    return phrases, states, lp, cum


OP_SIZES = [(k, V, C_) for k in (1, 2, 5, 32) for V in (37, 300) for C_ in (0, 1, 3, 7, 64) if V >= 2 * k + 1]


@pytest.mark.parametrize("step", [0, 1, 4])
def test_selection_kernel_equals_restatement(lib, step):
    """Every size as its own launch of B = 4 utterances (plain, exact ties, some -inf, mostly -inf), with guard rows behind the inputs
    and the outputs poisoned."""
    for k, V, C_ in OP_SIZES:
        rng = np.random.default_rng(7000 + 100 * k + V + C_ + step)
        B, R = 4, 4 * k
        utts = [_utterance(rng, k, V, C_, step, ties, ni) for ties, ni in ((False, 0), (True, 0), (False, 1), (True, 2))]
        cand_s = np.full((R + 1, CAND), np.nan, np.float32)
        cand_t = np.full((R + 1, CAND), SENT, np.int32)
        next_s = np.full((R + 1, 2), np.nan, np.float32)
        next_t = np.full((R + 1, 2), SENT, np.int32)
        state = np.full(R + 1, SENT, np.int32)
        want = []
        for b, (phrases, states, lp, cum) in enumerate(utts):
            cons = CR.Constraints(phrases)
            rows = lp.copy()
            nrow = 1 if step == 0 else k
            for j in range(nrow):
                if step > 0:
                    if not cons.finished(states[j]):
                        rows[j, EOS] = -np.inf
                    rows[j] = rows[j] + cum[j]
                r = b * k + j
                order = sorted(range(V), key=lambda n: (-float(rows[j, n]), n))[:2 * k]
                cand_s[r, :2 * k], cand_t[r, :2 * k] = rows[j, order], order
                nt = cons.next_tokens(states[j])
                next_t[r] = (nt + [-1, -1])[:2]
                next_s[r] = [rows[j, t] for t in nt] + [-np.inf] * (2 - len(nt))
            state[b * k:(b + 1) * k] = states
            want.append(CR.select(cons, lp, cum, states, k, step, EOS))
        tab = _table(lib, [u[0] for u in utts], V)
        out_s = torch.full((B + 1, CAND), float("nan"), dtype=torch.float32, device="cuda")
        out_t, out_b, out_st = (torch.full((B + 1, CAND), SENT, dtype=torch.int32, device="cuda") for _ in range(3))
        keep = [df(cand_s), di(cand_t), df(next_s), di(next_t), di(state), di(tab)]
        rc = lib.ss_op_beam_cons_select(S(), *[P(x) for x in keep], B, k, step, P(out_s), P(out_t), P(out_b), P(out_st))
        assert rc == 0
        torch.cuda.synchronize()
        gs, gt, gb, gst = out_s.cpu().numpy(), out_t.cpu().numpy(), out_b.cpu().numpy(), out_st.cpu().numpy()
        what = f"k {k} V {V} C {C_} step {step}"
        for b in range(B):
            assert bits(gs[b, :2 * k]).tolist() == [int(bits(x[0]).reshape(-1)[0]) for x in want[b]], f"{what} utterance {b}: scores"
            assert gt[b, :2 * k].tolist() == [x[1] for x in want[b]], f"{what} utterance {b}: tokens"
            assert gb[b, :2 * k].tolist() == [x[2] for x in want[b]], f"{what} utterance {b}: beams"
            assert gst[b, :2 * k].tolist() == [x[3] for x in want[b]], f"{what} utterance {b}: states"
        assert np.isnan(gs[:B, 2 * k:]).all() and np.isnan(gs[B]).all(), f"{what}: scores written past the selection"
        for g in (gt, gb, gst):
            assert (g[:B, 2 * k:] == SENT).all() and (g[B] == SENT).all(), f"{what}: written past the selection"
        del keep


# ---- search level -------------------------------------------------------------------------------------------------------------------
def _fix():
    return json.load(open(FIX, encoding="utf-8"))


_MODELS = {}


def _model_for(group, hip_model, synth_weights):
    if group["eos_scale"] == 1.0:
        return hip_model
    if group["eos_scale"] not in _MODELS:
        from streamspeech_amd.engine import HipModel
        from tests.make_golden_beam import state_dict
        cfg = synth_weights[0]
        g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
        _MODELS[group["eos_scale"]] = HipModel(state_dict(group["eos_scale"], cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])
    return _MODELS[group["eos_scale"]]


def _pcm(rec):
    from tests.make_golden_beam import sample_pcm
    return torch.from_numpy(sample_pcm(rec["pcm_seed"], rec["n_samples"]))


def _encode(model, pcms):
    lens = [int(p.numel()) for p in pcms]
    feat, T = model.batch_fbank_cmvn(torch.cat(pcms).cuda(), lens)
    enc, Tp = model.batch_encoder_forward(feat, T)
    return enc, Tp, T


def _compare(name, sid, rec, hyps):
    assert [h["tokens"] for h in hyps] == [h["tokens"] for h in rec["nbest"]], f"{name} sample {sid}: n-best tokens / order"
    worst = 0.0
    for h, r in zip(hyps, rec["nbest"]):
        d = abs(h["score"] - r["score"])
        worst = max(worst, d)
        assert d < rec["tau"] / 4, f"{name} sample {sid}: score {h['score']} vs {r['score']}"
        assert np.abs(np.array(h["positional_scores"]) - np.array(r["positional_scores"])).max() < rec["tau"]
    return worst


GROUPS = ["beam4_one_token", "beam5_two_phrases", "beam10_early_eos_lenpen0.6", "beam1_two_tokens", "beam4_mixed"]


@pytest.mark.parametrize("name", GROUPS)
def test_nbest_equals_reference(name, hip_model, synth_weights):
    """The engine call on the group's pinned utterances as one pack; SequenceGenerator on the first of them, with fairseq's packed
    tensor."""
    from oracle.ref_agent import make_dicts
    from streamspeech_amd.generators import SequenceGenerator
    grp = _fix()["groups"][name]
    model = _model_for(grp, hip_model, synth_weights)
    ids = [i for i, r in grp["hypotheses"].items() if r["margin"] > r["tau"]]
    recs = [grp["hypotheses"][i] for i in ids]
    assert len(ids) >= 6
    enc, Tp, T = _encode(model, [_pcm(r) for r in recs])
    beam, mlb = grp["beam"], grp["max_len_b_mt"]
    cons = [r["phrases"] for r in recs]
    nbest, _, _ = model.batch_mt_beam(enc, Tp, [mlb] * len(ids), beam, 1, 0.0, True, len_penalty=grp["len_penalty"], constraints=cons)
    worst = max(_compare(name, sid, rec, hyps) for sid, rec, hyps in zip(ids, recs, nbest))
    print(f"{name}: {len(ids)} utterances, worst |HIP - reference| score {worst:.3g}")
    for rec, hyps in zip(recs, nbest):
        for h in hyps:
            assert None not in CR.contains_in_order(h["tokens"], rec["phrases"]), f"{name}: a hypothesis misses a phrase"
    # today's search gives something else: the fixture would not pass without the feature
    plain, _, _ = model.batch_mt_beam(enc, Tp, [mlb] * len(ids), beam, 1, 0.0, True, len_penalty=grp["len_penalty"])
    assert sum(p[0]["tokens"] != r["nbest"][0]["tokens"] for p, r in zip(plain, recs)) >= (2 if name == "beam4_mixed" else 4)
    # SequenceGenerator, the packed tensor of fairseq's pack_constraints
    b = next(i for i, r in enumerate(recs) if r["phrases"])
    rec = recs[b]
    row = [len(rec["phrases"])] + [t for p in rec["phrases"] for t in p + [0]]
    gen = SequenceGenerator(model, make_dicts(model.cfg)["target_unigram"], beam_size=beam, max_len_a=0, max_len_b=mlb,
                            len_penalty=grp["len_penalty"])
    off = np.concatenate([[0], np.cumsum(Tp)])
    e = enc[off[b]:off[b + 1]].unsqueeze(1)
    out = gen.generate_decoder([{"encoder_out": [e]}], torch.zeros(1, T[b], 80), None, constraints=torch.tensor([row + [0, 0]]))[0]
    hyps = [{"tokens": h["tokens"].tolist(), "score": h["score"], "positional_scores": h["positional_scores"].tolist()} for h in out]
    _compare(name + " / SequenceGenerator", ids[b], rec, hyps)


def _key(hyps):
    return [(h["tokens"], bits(h["score"]).tolist(), bits(h["positional_scores"]).tolist()) for h in hyps]


def test_alone_and_in_the_mixed_pack_same_bits(hip_model):
    """Pack-invariant arithmetic: an utterance's n-best list has the same bits alone and among constrained and unconstrained
    neighbours; an utterance without phrases has the plain search's bits inside the constrained call."""
    grp = _fix()["groups"]["beam4_mixed"]
    recs = list(grp["hypotheses"].values())[:6]
    assert any(r["phrases"] for r in recs) and any(not r["phrases"] for r in recs)
    model = hip_model
    assert model.pack_invariant()
    enc, Tp, _ = _encode(model, [_pcm(r) for r in recs])
    beam, mlb = grp["beam"], grp["max_len_b_mt"]
    pack, _, _ = model.batch_mt_beam(enc, Tp, [mlb] * len(recs), beam, constraints=[r["phrases"] for r in recs])
    plain, _, _ = model.batch_mt_beam(enc, Tp, [mlb] * len(recs), beam)
    off = np.concatenate([[0], np.cumsum(Tp)])
    for b, r in enumerate(recs):
        if not r["phrases"]:
            assert _key(pack[b]) == _key(plain[b]), f"utterance {b}: no phrases, but not the plain search's bits"
            continue
        alone, _, _ = model.batch_mt_beam(enc[off[b]:off[b + 1]].contiguous(), [Tp[b]], [mlb], beam, constraints=[r["phrases"]])
        assert _key(alone[0]) == _key(pack[b]), f"utterance {b}: alone and in the pack differ"


def _raw_call(lib, model, entry, enc, Tp, mx, beam, tail):
    B = len(Tp)
    stride = max(mx) + 1
    rows = stride + 1
    feats = torch.full((B, rows, model.cfg.dec_dim), 7.0,
                       dtype=torch.float32, device="cuda")
    out = np.full(B * beam * stride, SENT, np.int32)
    n_out = np.full(B * beam, SENT, np.int32)
    sc = np.full(B * beam, 7.0, np.float32)
    pos = np.full(B * beam * stride, 7.0, np.float32)
    p32, pf = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    i32 = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(p32)   # noqa: E731
    tp, ml = np.ascontiguousarray(Tp, np.int32), np.ascontiguousarray(mx, np.int32)
    rc = getattr(lib, entry)(model.h, S(), B, beam, P(enc), tp.ctypes.data_as(p32), ml.ctypes.data_as(p32), 1, 0.0, 1,
                             out.ctypes.data_as(p32), stride, n_out.ctypes.data_as(p32), sc.ctypes.data_as(pf), pos.ctypes.data_as(pf),
                             P(feats), rows, *tail)
    torch.cuda.synchronize()
    return rc, out, n_out, sc, pos, feats.cpu().numpy()


def test_no_phrases_anywhere_equals_the_plain_call_and_refusals(lib, hip_model):
    """ss_batch_mt_beam_cons with empty constraints runs the constrained kernels and returns ss_batch_mt_beam_opts' bits; every
    refusal returns SS_ERR_ARG and leaves the output buffers as they were."""
    model = hip_model
    grp = _fix()["groups"]["beam4_one_token"]
    recs = list(grp["hypotheses"].values())[:3]
    enc, Tp, _ = _encode(model, [_pcm(r) for r in recs])
    beam, mx = 4, [10, 10, 10]
    p32 = C.POINTER(C.c_int32)

    def cons_tail(phrases_per_utt, ends=None):
        toks, off, e = _pack(phrases_per_utt)
        if ends is not None:
            e = np.asarray(ends, np.int32)
        cons_tail.keep = (toks, off, e)
        return (None, toks.ctypes.data_as(p32), off.ctypes.data_as(p32), e.ctypes.data_as(p32))
    plain = _raw_call(lib, model, "ss_batch_mt_beam_opts", enc, Tp, mx, beam, (None,))
    empty = _raw_call(lib, model, "ss_batch_mt_beam_cons", enc, Tp, mx, beam, cons_tail([[], [], []]))
    assert plain[0] == 0 and empty[0] == 0
    assert (plain[2] > 0).any()
    for a, b, what in zip(plain[1:], empty[1:], ("tokens", "lengths", "scores", "positional scores", "features")):
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b), what
    V = model.cfg.tgt_vocab
    for what, tail in (("more than 64 tokens", cons_tail([[[4 + i for i in range(65)]], [], []])),
                       ("a token at V", cons_tail([[], [[V]], []])),
                       ("pad in a phrase", cons_tail([[[5, PAD]], [], []])),
                       ("</s> in a phrase", cons_tail([[], [], [[EOS]]])),
                       ("an open last phrase", cons_tail([[[5, 6]], [], []], ends=[0, 0])),
                       ("C above max_len", cons_tail([[[4 + i for i in range(11)]], [], []])),
                       ("no offsets", (None, None, None, None))):
        rc, out, n_out, sc, pos, feats = _raw_call(lib, model, "ss_batch_mt_beam_cons", enc, Tp, mx, beam, tail)
        assert rc == SS_ERR_ARG, what
        assert (out == SENT).all() and (n_out == SENT).all() and (sc == 7.0).all() and (pos == 7.0).all() and (feats == 7.0).all(), what
    with pytest.raises(ValueError, match="empty"):
        model.batch_mt_beam(enc, Tp, mx, beam, constraints=[[[5], []], [], []])
    with pytest.raises(ValueError):
        model._mt_beam("ss_batch_mt_beam_continue", enc, Tp, [[], [], []], mx, beam, 0, 1, 0.0, True, (1.0, 1.0, 0),
                       constraints=[[[5]], [], []])


# ---- the driver ---------------------------------------------------------------------------------------------------------------------
def test_driver_writes_constrained_translations(hip_model, tmp_path):
    """offline.generate on four utterances with a glossary: C- lines, the report, D- texts that hold the phrases, and, without the
    argument, the files of a run that has never heard of it."""
    from oracle.ref_agent import make_dicts
    from streamspeech_amd import offline
    model = hip_model
    grp = _fix()["groups"]["beam5_two_phrases"]
    ids = [i for i, r in grp["hypotheses"].items() if r["margin"] > r["tau"]][:4]
    recs = [grp["hypotheses"][i] for i in ids]
    dicts = make_dicts(model.cfg)
    d = dicts["target_unigram"]
    items = [(int(i), _pcm(r).cuda()) for i, r in zip(ids, recs)]
    lines = ["\t".join([str(i)] + [" ".join(d[t] for t in p) for p in r["phrases"]]) + "\n" for i, r in zip(ids[:3], recs)]
    glossary = offline.parse_constraints_file(lines, d)
    assert glossary == {int(i): r["phrases"] for i, r in zip(ids[:3], recs)}
    kw = dict(max_len_b_mt=grp["max_len_b_mt"], dump_wav=False, beam_mt=grp["beam"])
    a, b, c = (str(tmp_path / x) for x in "abc")
    hyp = offline.generate(model, None, items, dicts, a, "test", constraints=glossary, **kw)
    log = open(os.path.join(a, "generate-test.log"), encoding="utf-8").read().splitlines()
    report = [ln.split("\t") for ln in open(os.path.join(a, "generate-test.mt.constraints"), encoding="utf-8").read().splitlines()]
    for i, r in zip(ids[:3], recs):
        texts = [offline.detok([d[t] for t in p]) for p in r["phrases"]]
        assert [ln for ln in log if ln.startswith(f"C-{i}\t")] == [f"C-{i}\t{t}" for t in texts]
        want = offline.detok([d[t] for t in r["nbest"][0]["tokens"] if t != EOS])
        assert hyp[int(i)]["mt"] == want and f"D-{i}\t{want}" in log
        rows = [x for x in report if x[0] == str(i)]
        assert [x[1] for x in rows] == texts and all(x[2] == "1" for x in rows)
        best = r["nbest"][0]["tokens"]
        assert [int(x[3]) for x in rows] == CR.contains_in_order(best, r["phrases"])
    assert not [ln for ln in log if ln.startswith(f"C-{ids[3]}\t")] and not [x for x in report if x[0] == str(ids[3])]
    offline.generate(model, None, items, dicts, b, "test", **kw)
    assert "generate-test.mt.constraints" not in os.listdir(b)
    # an empty glossary is the plain search: the same bytes in every file both runs write
    offline.generate(model, None, items, dicts, c, "test", constraints={}, **kw)
    for name in sorted(os.listdir(b)):
        if os.path.isfile(os.path.join(b, name)):
            assert open(os.path.join(b, name), "rb").read() == open(os.path.join(c, name), "rb").read(), name
