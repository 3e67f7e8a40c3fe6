"""The text search controls on the GPU (csrc/beam_kernels.hip: beam_topk_opts_kernel, beam_merge_lenpen_kernel,
beam_prefix_score_temp_kernel and the *_opts entry points).

Op level, each kernel through its ss_op_* entry: the no-repeat ban against the numpy restatement of tests/search_ref.py on rows whose
history crosses hypothesis slots; the temperature against a float64 log-softmax of logits / T at the bound of the existing top-2k
test (1e-5); the length penalty against cum / (step + 1) ** p in float64.
End to end on the synthetic checkpoint: the fixture tests/golden/search_options.json (the reference's generator with the controls
set, tests/make_golden_search_options.py) through the engine, offline.generate and SequenceGenerator -- identical n-best tokens and
order, scores within tau / 4, positional scores within tau, the bounds of tests/test_beam_gpu.py -- and the streaming surfaces (the
S2TT agent's flag, a TextSessionPool with search=) against each other and against the rule itself."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import glue_ref as R
from tests import search_ref as SR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "search_options.json")
CAND = R.CAND
SENT = -7
G = 5
PAD, UNK, EOS = 1, 3, 2


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


def of(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def oi(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the ban ------------------------------------------------------------------------------------------------------------------------
def _ban_case(V, n, t_step, seed):
    """12 utterances x 4 slots.  Utterances 0, 2, 4, ... have a 3-token prefix, the others none; utterance 5 is done, utterance 7 at
    its length limit.  Tokens come from six symbols, so windows repeat, and utterance 0 repeats one symbol throughout (the synthetic
    model's loop): its rows are banned from as early as the rule allows.  The ancestry is a random permutation of the utterance's
    slots at every position, so a row's history crosses slots."""
    rng = np.random.default_rng(seed)
    B, k, c0 = 12, 4, 3
    R_ = B * k
    Lc = c0 + t_step + 2 + 2
    npre = np.array([3 if b % 2 == 0 else 0 for b in range(B)])
    done = np.zeros(B, int)
    done[5] = 1
    mxl = np.full(B, 60)
    mxl[7] = t_step + npre[7]
    row0 = np.concatenate([[0], np.cumsum(npre)])[:-1] + 2                  # two unused rows in front of the prefix-pass tokens
    ptok = np.full(int(npre.sum()) + 2 + G, SENT)
    sym = np.array([4, 5, 6, 7, 8, 9])
    for b in range(B):
        ptok[row0[b]:row0[b] + npre[b]] = [EOS] + list(rng.choice(sym, npre[b] - 1)) if npre[b] else []
    tok = rng.choice(sym, (t_step + 1, R_))
    tok[:, 0:k] = 4
    ptok[row0[0] + 1:row0[0] + npre[0]] = 4
    for b in range(B):
        if npre[b] == 0:
            tok[0, b * k:(b + 1) * k] = EOS                                 # no prefix: the row fed at lock-step index 0 is </s>
    anc = np.full((R_, Lc), SENT)
    for b in range(B):
        for p in range(c0 + t_step + 1):
            anc[b * k:(b + 1) * k, p] = b * k + rng.permutation(k)
    rows = {}
    for r in range(R_):
        b = r // k
        if done[b] or (t_step == 0 and r % k):
            continue
        rows[r] = [int(x) for x in ptok[row0[b]:row0[b] + npre[b]]] + [int(tok[u, anc[r, c0 + u]]) for u in range(t_step + 1)]
        assert rows[r][0] == EOS and EOS not in rows[r][1:] and len(rows[r]) == npre[b] + t_step + 1
    logits = (rng.standard_normal((R_, V)) * 2).astype(np.float32)
    cum = (-rng.random(R_) * 6).astype(np.float32)
    return dict(B=B, k=k, c0=c0, R=R_, Lc=Lc, npre=npre, done=done, mxl=mxl, row0=row0, ptok=ptok, tok=tok, anc=anc, rows=rows,
                logits=logits, cum=cum)


def _topk_opts(lib, c, V, t_step, temp, n, want_rows=True, min_len=1, pen=0.25):
    cs, ct = of(c["R"] + G, CAND), oi(c["R"] + G, CAND)
    rs = of(c["R"] + G, V) if want_rows else None
    keep = [df(c["logits"]), di(c["mxl"]), di(c["npre"]), di(c["done"]), df(c["cum"]), di(c["tok"]), di(c["anc"]), di(c["ptok"]),
            di(c["row0"])]
    rc = lib.ss_op_beam_topk_opts(S(), P(keep[0]), c["R"], V, c["k"], t_step, min_len, P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]),
                                  PAD, UNK, EOS, pen, P(cs), P(ct), temp, n, P(keep[5]), P(keep[6]), c["Lc"], c["c0"], P(keep[7]),
                                  P(keep[8]), P(rs))
    assert rc == 0, f"return code {rc}"
    out = host(cs), host(ct), (host(rs) if want_rows else None)
    del keep
    return out


@pytest.mark.parametrize("V,n,t_step", [(97, n, t) for n in (2, 3, 4) for t in sorted({0, 1, n - 2, n - 1, 17})] + [(6000, 3, 17)])
def test_ngram_ban_against_the_restatement(lib, V, n, t_step):
    c = _ban_case(V, n, t_step, 1000 * n + t_step + V)
    base_s, base_t, base = _topk_opts(lib, c, V, t_step, 1.0, 0)           # options off, the row scores read out
    got_s, got_t, got = _topk_opts(lib, c, V, t_step, 1.0, n)
    k, R_ = c["k"], c["R"]
    n_banned = 0
    for r in range(R_ + G):
        if r not in c["rows"]:                                              # done utterance, beams 1.. at the first step, guard rows
            assert np.isnan(got[r]).all() and np.isnan(got_s[r]).all() and (got_t[r] == SENT).all()
            continue
        b = r // k
        banned = sorted(SR.banned_tokens(c["rows"][r], n))
        assert EOS not in banned
        n_banned += len(banned)
        mask = np.zeros(V, bool)
        mask[banned] = True
        assert np.all(np.isneginf(got[r][mask])), f"row {r}: a banned entry is not -inf"
        assert np.array_equal(bits(got[r][~mask]), bits(base[r][~mask])), f"row {r}: an entry outside the ban changed"
        if c["mxl"][b] <= t_step + c["npre"][b]:                            # at the length limit </s> is all that is left, ban or not
            assert np.isneginf(np.delete(got[r], EOS)).all()
            assert np.isfinite(got[r][EOS]) or t_step + c["npre"][b] < 1     # (below min_len = 1 not even that)
        # the row's 2k best of what the selection saw: score descending, then token ascending
        order = sorted(range(V), key=lambda t: (-got[r][t], t))[:2 * k]
        assert got_t[r, :2 * k].tolist() == order
        assert np.array_equal(bits(got_s[r, :2 * k]), bits(got[r][order]))
        assert np.isnan(got_s[r, 2 * k:]).all()
    if 3 + t_step >= n:                                                     # utterance 0: </s> and 3 + t_step equal tokens
        assert n_banned > 0 and SR.banned_tokens(c["rows"][0], n) == {4}, "the case bans nothing"
    # options off through the option entry: the lists ss_op_beam_topk gives, bit for bit
    cs, ct = of(R_ + G, CAND), oi(R_ + G, CAND)
    keep = [df(c["logits"]), di(c["mxl"]), di(c["npre"]), di(c["done"]), df(c["cum"])]
    assert lib.ss_op_beam_topk(S(), P(keep[0]), R_, V, k, t_step, 1, P(keep[1]), P(keep[2]), P(keep[3]), P(keep[4]), PAD, UNK, EOS, 0.25,
                               P(cs), P(ct)) == 0
    assert np.array_equal(bits(host(cs)), bits(base_s)) and np.array_equal(host(ct), base_t)
    print(f"ban V={V} n={n} t={t_step}: {n_banned} banned entries over {len(c['rows'])} rows")


def test_topk_opts_refusals(lib):
    c = _ban_case(97, 2, 1, 5)
    a = [df(c["logits"]), di(c["mxl"]), di(c["npre"]), di(c["done"]), df(c["cum"]), di(c["tok"]), di(c["anc"]), di(c["ptok"]), di(c["row0"])]
    cs, ct = of(c["R"], CAND), oi(c["R"], CAND)

    def call(temp, n, Lc=c["Lc"], tok=a[5]):
        return lib.ss_op_beam_topk_opts(S(), P(a[0]), c["R"], 97, c["k"], 1, 1, P(a[1]), P(a[2]), P(a[3]), P(a[4]), PAD, UNK, EOS, 0.0,
                                        P(cs), P(ct), temp, n, P(tok), P(a[6]), Lc, c["c0"], P(a[7]), P(a[8]), None)
    for temp, n in ((1.0, 1), (1.0, 33), (0.0, 0), (float("nan"), 0), (-1.0, 2)):
        assert call(temp, n) == 2
    assert call(1.0, 2, Lc=c["c0"] + 1) == 2          # the history would run past the ancestry row
    assert call(1.0, 2, tok=None) == 2
    torch.cuda.synchronize()
    assert torch.isnan(cs).all()


# ---- the temperature ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [2.0, 1.7, 0.5])
@pytest.mark.parametrize("V,k,t_step", [(300, 5, 2), (6000, 4, 0), (9, 4, 3)])
def test_temperature_topk(lib, V, k, t_step, temp):
    """As test_beam_topk of tests/test_glue_ops_gpu.py: logits on a 1/8 lattice, so two candidates of a row have equal logits, hence
    equal quotients and equal scores in any arithmetic, or scores at least 0.125 / T apart; the bound is that test's 1e-5."""
    rng = np.random.default_rng(V + k + int(temp * 10))
    B, min_len, pen = 6, 2, 0.5625
    R_ = B * k
    logits = (rng.integers(-32, 33, (R_, V)) / 8.0).astype(np.float32)
    cum = (rng.integers(-40, 1, R_) / 8.0).astype(np.float32)
    npre, mxl, done = [0, 1, 2, 0, 2, 3], [10, 10, t_step + 2, 10, 10, t_step + 1], [0, 0, 0, 1, 0, 0]
    logits[4 * k, V - 1] = np.nan
    c = dict(R=R_, k=k, c0=0, Lc=0, logits=logits, cum=cum, npre=npre, mxl=mxl, done=done, tok=[0], anc=[0], ptok=[0], row0=[0] * B)
    cs, ct, _ = _topk_opts(lib, c, V, t_step, temp, 0, want_rows=False, min_len=min_len, pen=pen)
    scaled = (logits / np.float32(temp)).astype(np.float32)               # the float32 division; the reference is float64 from here
    want = R.beam_topk(scaled, k, t_step, min_len, mxl, npre, done, cum, PAD, UNK, EOS, pen)
    wt, ws = np.full((R_ + G, CAND), SENT), np.full((R_ + G, CAND), np.nan)
    for r, (s, t) in want.items():
        ws[r, :len(s)], wt[r, :len(t)] = s, t
    assert np.array_equal(ct, wt)
    assert np.array_equal(np.isnan(cs), np.isnan(ws)) and np.array_equal(np.isinf(cs), np.isinf(ws))
    fin = np.isfinite(ws)
    err = np.max(np.abs(cs[fin] - ws[fin]))
    print(f"temperature top-2k V={V} k={k} t={t_step} T={temp}: max score error {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("temp", [1.7, 0.5])
def test_temperature_prefix_score(lib, temp):
    V, rows = 6000, 12
    rng = np.random.default_rng(int(temp * 10))
    logits = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    ftok = rng.integers(4, V, rows)
    ftok[1], ftok[2], ftok[3] = -1, PAD, UNK
    lp = of(rows + G)
    a = [df(logits), di(ftok)]
    assert lib.ss_op_beam_prefix_score_opts(S(), P(a[0]), rows, V, P(a[1]), PAD, UNK, 0.5, P(lp), temp) == 0
    want = np.concatenate([R.beam_prefix_score((logits / np.float32(temp)).astype(np.float32), ftok, PAD, UNK, 0.5), np.full(G, np.nan)])
    lp = host(lp)
    assert np.array_equal(np.isnan(lp), np.isnan(want)) and np.array_equal(np.isinf(lp), np.isinf(want))
    fin = np.isfinite(want)
    assert np.max(np.abs(lp[fin] - want[fin])) <= 1e-5                     # the bound of test_beam_prefix_score
    # T = 1 through the option entry is the plain kernel, bit for bit
    one, plain = of(rows), of(rows)
    assert lib.ss_op_beam_prefix_score_opts(S(), P(a[0]), rows, V, P(a[1]), PAD, UNK, 0.5, P(one), 1.0) == 0
    assert lib.ss_op_beam_prefix_score(S(), P(a[0]), rows, V, P(a[1]), PAD, UNK, 0.5, P(plain)) == 0
    assert np.array_equal(bits(host(one)), bits(host(plain)))
    assert lib.ss_op_beam_prefix_score_opts(S(), P(a[0]), rows, V, P(a[1]), PAD, UNK, 0.5, P(one), 0.0) == 2


# ---- the length penalty ------------------------------------------------------------------------------------------------------------
FLOATS = ("cum", "cand_s", "fin_score", "fin_pos")


@pytest.mark.parametrize("p", [0.6, 1.5, 0.0])
@pytest.mark.parametrize("k,t_step,c0", [(1, 0, 0), (5, 3, 2), (32, 3, 0)])
def test_len_penalty_merge(lib, k, t_step, c0, p):
    """The merge step of tests/test_glue_ops_gpu.py with the penalty: every table but fin_score is what the unnormalised step leaves,
    bit for bit; a finalised score is cum / (step + 1) ** p.  The existing test holds fin_score to its float32 reference bit for
    bit; against a float64 reference the bound is the float32 format's: one rounding of the power and one of the quotient, 2 ** -24
    relative each, and half an ulp of the comparison itself -- 3 * 2 ** -24 |score|."""
    from streamspeech_amd.lib import SSOpBeamState
    from tests.test_glue_ops_gpu import _merge_state
    st, B, Lc, V = _merge_state(k, t_step, c0, 1000 * k + 10 * t_step + c0)
    # utterances 2 and 3 hold earlier finalised entries: give them scores of shorter hypotheses under the same penalty, on a lattice
    # whose steps are far above the bound, so the order of an utterance's table is decided
    for b in (2, 3):
        for e in range(st["fin_cnt"][b]):
            st["fin_score"][b, e] = np.float32(-(3 + e) / 8.0) / np.float32(float(e + 1) ** p)
    d = {n: (df(a) if n in FLOATS else di(a)) for n, a in st.items()}
    x = SSOpBeamState(**{n: d[n].data_ptr() for n in d})
    assert lib.ss_op_beam_merge_opts(S(), C.byref(x), B, k, Lc, V, t_step, c0, EOS, 1, p) == 0
    raw = R.beam_merge(st, B, k, Lc, V, t_step, c0, EOS, 0)                # unnormalised: fin_score = the cumulative score
    for n in st:
        if n != "fin_score":
            want = raw[n].astype(np.float32) if n in FLOATS else raw[n]
            got = host(d[n])
            assert np.array_equal(bits(got) if n in FLOATS else got, bits(want) if n in FLOATS else want.astype(got.dtype)), n
    got = host(d["fin_score"]).astype(np.float64)
    n_new = 0
    for b in range(B):
        step = t_step + int(st["npre"][b])
        for e in range(k):
            new = e >= st["fin_cnt"][b] and e < raw["fin_cnt"][b]
            if not new:                                                    # earlier entries and free slots stay as they were
                assert np.array_equal(bits(got[b, e]), bits(st["fin_score"][b, e]))
                continue
            n_new += 1
            want = SR.final_score(raw["fin_score"][b, e], step, p)
            assert abs(got[b, e] - want) <= 3 * 2.0 ** -24 * abs(want), (b, e, got[b, e], want)
        # the table's order (what the search sorts by at the end) is the float64 one wherever the float64 gaps exceed the bound
        n_e = int(raw["fin_cnt"][b])
        ref = [SR.final_score(raw["fin_score"][b, e], step, p) if e >= st["fin_cnt"][b] else float(st["fin_score"][b, e])
               for e in range(n_e)]
        gaps_ok = all(abs(u - v) > 6 * 2.0 ** -24 * max(abs(u), abs(v)) or u == v for i, u in enumerate(ref) for v in ref[i + 1:])
        if gaps_ok:
            assert sorted(range(n_e), key=lambda e: (-got[b, e], e)) == sorted(range(n_e), key=lambda e: (-ref[e], e)), b
    assert n_new >= 1
    # p = 1 and the unnormalised step through the option entry are the plain kernel
    for norm, pp in ((1, 1.0), (0, 0.6)):
        d1 = {n: (df(a) if n in FLOATS else di(a)) for n, a in st.items()}
        d2 = {n: (df(a) if n in FLOATS else di(a)) for n, a in st.items()}
        x1, x2 = SSOpBeamState(**{n: d1[n].data_ptr() for n in d1}), SSOpBeamState(**{n: d2[n].data_ptr() for n in d2})
        assert lib.ss_op_beam_merge_opts(S(), C.byref(x1), B, k, Lc, V, t_step, c0, EOS, norm, pp) == 0
        assert lib.ss_op_beam_merge(S(), C.byref(x2), B, k, Lc, V, t_step, c0, EOS, norm) == 0
        assert np.array_equal(bits(host(d1["fin_score"])), bits(host(d2["fin_score"])))
    assert lib.ss_op_beam_merge_opts(S(), C.byref(x), B, k, Lc, V, t_step, c0, EOS, 1, float("nan")) == 2


# ---- end to end: the fixture ---------------------------------------------------------------------------------------------------------
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


def _opts(grp):
    return {"len_penalty": grp["len_penalty"], "temperature": grp["temperature"], "no_repeat_ngram_size": grp["no_repeat_ngram_size"]}


def _compare(name, sid, rec, hyps):
    assert [h["tokens"] for h in hyps] == [h["tokens"] for h in rec["nbest"]], f"{name} sample {sid}: n-best tokens / order"
    worst = 0.0
    for h, r in zip(hyps, rec["nbest"]):
        d = abs(h["score"] - r["score"])
        worst = max(worst, d)
        assert d < rec["tau"] / 4, f"{name} sample {sid}: score {h['score']} vs {r['score']}"
        assert np.abs(np.array(h["positional_scores"]) - np.array(r["positional_scores"])).max() < rec["tau"]
    return worst


GROUPS = ["beam4_ngram2", "beam5_ngram3_lenpen0.6", "beam10_early_eos_lenpen1.5_temp1.7", "beam10_early_eos_lenpen0.5_temp1.7",
          "beam1_ngram2"]


@pytest.mark.parametrize("name", GROUPS)
def test_nbest_equals_reference(name, hip_model, synth_weights, tmp_path):
    """The engine call on the whole group as one pack, SequenceGenerator per utterance, and the offline driver."""
    from oracle.ref_agent import make_dicts
    from streamspeech_amd import offline
    from streamspeech_amd.generators import SequenceGenerator
    grp = _fix()["groups"][name]
    model = _model_for(grp, hip_model, synth_weights)
    ids = [i for i, r in grp["hypotheses"].items() if r["margin"] > r["tau"]]
    recs = [grp["hypotheses"][i] for i in ids]
    assert len(ids) >= 6
    enc, Tp, T = _encode(model, [_pcm(r) for r in recs])
    beam, mlb = grp["beam"], grp["max_len_b_mt"]
    nbest, _, _ = model.batch_mt_beam(enc, Tp, [mlb] * len(ids), beam, 1, 0.0, True, **_opts(grp))
    worst = max(_compare(name, sid, rec, hyps) for sid, rec, hyps in zip(ids, recs, nbest))
    print(f"{name}: {len(ids)} utterances, worst |HIP - reference| score {worst:.3g}")
    # today's search gives something else where the ban bites: the fixture would not pass without the feature
    if grp["no_repeat_ngram_size"]:
        plain, _, _ = model.batch_mt_beam(enc, Tp, [mlb] * len(ids), beam)
        assert sum(p[0]["tokens"] != r["nbest"][0]["tokens"] for p, r in zip(plain, recs)) >= 4
    # SequenceGenerator: one utterance at a time, through batch_mt_beam_continue with no prefix
    dicts = make_dicts(model.cfg)
    gen = SequenceGenerator(model, dicts["target_unigram"], beam_size=beam, max_len_a=0, max_len_b=mlb, **_opts(grp))
    off = np.concatenate([[0], np.cumsum(Tp)])
    for b, (sid, rec) in enumerate(zip(ids, recs)):
        e = enc[off[b]:off[b + 1]].unsqueeze(1)
        out = gen.generate_decoder([{"encoder_out": [e]}], torch.zeros(1, T[b], 80), None)[0]
        hyps = [{"tokens": h["tokens"].tolist(), "score": h["score"], "positional_scores": h["positional_scores"].tolist()} for h in out]
        _compare(name + " / SequenceGenerator", sid, rec, hyps)
    # the driver: the D- hypothesis is hypothesis 0
    items = [(int(i), _pcm(r).cuda()) for i, r in zip(ids, recs)]
    hyp = offline.generate(model, None, items, dicts, str(tmp_path), "test", max_len_b_mt=mlb, dump_wav=False, beam_mt=beam, **_opts(grp))
    for sid, rec in zip(ids, recs):
        want = offline.detok([dicts["target_unigram"][t] for t in rec["nbest"][0]["tokens"] if t != EOS])
        assert hyp[int(sid)]["mt"] == want, f"{name} sample {sid}: the driver's D- text"


def test_forced_prefix_nbest_equals_reference(hip_model, synth_weights):
    from oracle.ref_agent import make_dicts
    from streamspeech_amd.generators import SequenceGenerator
    name = "prefix_beam4_ngram2"
    grp = _fix()["groups"][name]
    cases = [c for c in grp["cases"] if c["margin"] > c["tau"]]
    assert {len(c["prefix"]) for c in cases} == {0, 1, 3} and len(cases) >= 6
    enc, Tp, T = _encode(hip_model, [_pcm(c) for c in cases])
    mlb, beam = grp["max_len_b_mt"], grp["beam"]
    nbest, _ = hip_model.batch_mt_beam_continue(enc, Tp, [c["prefix"] for c in cases], [mlb] * len(cases), beam, 1, 0.0, True, **_opts(grp))
    for c, hyps in zip(cases, nbest):
        _compare(name, c["sid"], c, hyps)
    gen = SequenceGenerator(hip_model, make_dicts(hip_model.cfg)["target_unigram"], beam_size=beam, max_len_a=0, max_len_b=mlb, **_opts(grp))
    off = np.concatenate([[0], np.cumsum(Tp)])
    for b, c in enumerate(cases):
        pt = torch.tensor([c["prefix"]], dtype=torch.long) if c["prefix"] else None
        out = gen.generate_decoder([{"encoder_out": [enc[off[b]:off[b + 1]].unsqueeze(1)]}], torch.zeros(1, T[b], 80), None,
                                   prefix_tokens=pt)[0]
        hyps = [{"tokens": h["tokens"].tolist(), "score": h["score"], "positional_scores": h["positional_scores"].tolist()} for h in out]
        _compare(name + " / SequenceGenerator", c["sid"], c, hyps)
    # a prefix that repeats a bigram is refused before anything runs
    from streamspeech_amd import lib as L
    with pytest.raises(L.StreamSpeechHipError) as e:
        hip_model.batch_mt_beam_continue(enc[:Tp[0]], Tp[:1], [[7, 8, 7, 8]], [mlb], beam, no_repeat_ngram_size=2)
    assert e.value.code == L.SS_ERR_ARG


# ---- end to end: properties ---------------------------------------------------------------------------------------------------------
def _synthetic(n, seed0):
    from streamspeech_amd import synth, workload
    utts = sorted(workload.make_utterances(60), key=lambda u: u.seconds)[:n]
    return [torch.from_numpy(synth.synth_pcm(seed0 + u.idx, u.n_samples)) for u in utts]


def _key(h):
    return [(x["tokens"], struct.pack("<f", x["score"]), [struct.pack("<f", p) for p in x["positional_scores"]]) for x in h]


def test_pack_invariance_with_the_ban(hip_model):
    pcms = _synthetic(5, 900)
    enc, Tp, _ = _encode(hip_model, pcms)
    off = np.concatenate([[0], np.cumsum(Tp)])
    kw = dict(no_repeat_ngram_size=3, len_penalty=0.6, temperature=1.7)
    whole, wf, wn = hip_model.batch_mt_beam(enc, Tp, [12, 13, 14, 12, 13], 4, **kw)
    for b in (0, 3, 4):
        alone, af, an = hip_model.batch_mt_beam(enc[off[b]:off[b + 1]], [Tp[b]], [[12, 13, 14, 12, 13][b]], 4, **kw)
        assert _key(alone[0]) == _key(whole[b]), f"utterance {b}: alone vs in a pack of 5"
        assert an[0] == wn[b] and torch.equal(af[0, :an[0]], wf[b, :wn[b]])


@pytest.mark.parametrize("beam", [1, 4])
def test_defaults_are_the_existing_call(beam, hip_model):
    """ss_batch_mt_beam_continue_opts with NULL and with all-default options against ss_batch_mt_beam_continue: every output bit."""
    from streamspeech_amd import lib as L
    lib = L.load()
    pcms = _synthetic(3, 940)
    enc, Tp, _ = _encode(hip_model, pcms)
    B, ml, stride, rows = 3, 12, 13, 13
    prefixes = [[], [9, 4], [11]]
    flat = [t for p in prefixes for t in p]
    i32 = lambda v: (C.c_int32 * len(v))(*v)      # noqa: E731
    D = hip_model.cfg.dec_dim

    def run(fn, *extra):
        out, n_out = (C.c_int32 * (B * beam * stride))(), (C.c_int32 * (B * beam))()
        sc, pos = (C.c_float * (B * beam))(), (C.c_float * (B * beam * stride))()
        feats = torch.zeros((B, rows, D), device="cuda")
        rc = fn(hip_model.h, S(), B, beam, P(enc), i32(Tp), i32(flat), i32([len(p) for p in prefixes]), i32([ml] * B), 1, 0.0, 1, out,
                stride, n_out, sc, pos, P(feats), rows, *extra)
        assert rc == 0
        torch.cuda.synchronize()
        n = list(n_out)
        toks = [list(out[o * stride:o * stride + n[o]]) for o in range(B * beam)]
        return n, toks, bytes(sc), [bytes(pos)[4 * o * stride:4 * (o * stride + len(prefixes[o // beam]) + n[o])] for o in range(B * beam)], \
            [feats[b, :len(prefixes[b]) + n[b * beam]].clone() for b in range(B)]
    want = run(lib.ss_batch_mt_beam_continue)
    default = L.SSMtSearchOpts(C.sizeof(L.SSMtSearchOpts), 0, 1.0, 1.0)
    for extra in (None, C.byref(default)):
        got = run(lib.ss_batch_mt_beam_continue_opts, extra)
        assert got[:4] == want[:4]
        assert all(torch.equal(a, b) for a, b in zip(got[4], want[4]))
    assert any(n > 0 for n in want[0])


def test_max_len_still_finalises_under_the_ban(hip_model):
    """n = 2 and a short max_len: at the limit only </s> is left and it is never banned, so every utterance finalises, with </s> last
    and a finite best score; and no hypothesis holds a bigram twice."""
    pcms = _synthetic(6, 970)
    enc, Tp, _ = _encode(hip_model, pcms)
    for beam in (1, 4):
        nbest, _, _ = hip_model.batch_mt_beam(enc, Tp, [3, 4, 5, 6, 7, 8], beam, no_repeat_ngram_size=2)
        for b, hyps in enumerate(nbest):
            assert len(hyps) >= 1 and np.isfinite(hyps[0]["score"])
            for h in hyps:
                assert h["tokens"][-1] == EOS and len(h["tokens"]) <= [3, 4, 5, 6, 7, 8][b] + 1 and np.isfinite(h["score"])
                assert not SR.prefix_repeats(h["tokens"][:-1], 2), h["tokens"]
        plain, _, _ = hip_model.batch_mt_beam(enc, Tp, [3, 4, 5, 6, 7, 8], beam)
        assert any(SR.prefix_repeats(h[0]["tokens"][:-1], 2) for h in plain)      # the model does repeat when it may


# ---- the streaming surfaces --------------------------------------------------------------------------------------------------------
def _s2tt_agent(hip_model, cfg, flags, ms=320):
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from tests import ref_fixtures as RF
    model = StreamSpeechModel.from_engine(hip_model.new_context())
    return RF.set_dicts(StreamSpeechS2TTAgent(RF.agent_args(StreamSpeechS2TTAgent, ms, 16000, extra=flags), model=model), cfg)


def _run_agent(agent, pcm, ms=320):
    from streamspeech_amd.simuleval_shim import SpeechSegment
    step, pos, recs = 16 * ms, 0, []
    while True:
        chunk = pcm[pos:pos + step]
        pos += step
        fin = pos >= len(pcm)
        o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=16000, finished=fin))
        t = agent.tgt_subwords_indices
        recs.append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished),
                     None if t is None else [int(x) for x in t.view(-1).tolist()]))
        if fin:
            return recs


def test_s2tt_agent_flag_and_pool_search(hip_model, synth_weights):
    """--no-repeat-ngram-size 2 at the agent's beam 1: every write is a search behind the committed prefix under the ban, so the
    committed text never holds a bigram twice (and the prefix is never refused), where the plain agent's text does; two sessions of
    a TextSessionPool with search= give what two single agents with the flag give."""
    from streamspeech_amd import synth
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.engine import SearchOptions
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    from tests import ref_fixtures as RF
    cfg = synth_weights[0]
    pcms = [synth.synth_pcm(4000 + i, int(16000 * (1.6 + 0.8 * i))) for i in range(2)]
    flags = ["--no-repeat-ngram-size", "2"]
    want = []
    for pcm in pcms:
        agent = _s2tt_agent(hip_model, cfg, flags)
        assert agent.generator_mt.search == {"len_penalty": 1.0, "temperature": 1.0, "no_repeat_ngram_size": 2}
        recs = _run_agent(agent, pcm)
        final = next(t for _, _, _, t in reversed(recs) if t is not None)
        assert len(final) >= 3 and not SR.prefix_repeats(final, 2), final
        want.append(recs)
    plain = _run_agent(_s2tt_agent(hip_model, cfg, []), pcms[1])
    assert SR.prefix_repeats(next(t for _, _, _, t in reversed(plain) if t is not None), 2)
    pool = TextSessionPool(hip_model, 4, 256, search=SearchOptions(no_repeat_ngram_size=2))
    d = RF.dictionaries(cfg)
    sids = [pool.open("s2tt", RF.agent_args(StreamSpeechS2TTAgent, 320, 16000), dicts=d) for _ in pcms]
    got, pos, live = [[] for _ in pcms], [0] * len(pcms), set(range(len(pcms)))
    while live:
        segs = {}
        for i in sorted(live):
            chunk = pcms[i][pos[i]:pos[i] + 5120]
            pos[i] += 5120
            segs[sids[i]] = SpeechSegment(content=chunk.tolist(), sample_rate=16000, finished=pos[i] >= len(pcms[i]))
        out = pool.step(segs)
        for i in sorted(live):
            o, s = out[sids[i]], pool.sessions[sids[i]]
            got[i].append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished),
                           None if s.tgt_subwords is None else list(s.tgt_subwords)))
            if segs[sids[i]].finished:
                live.discard(i)
    assert got == want
    with pytest.raises(ValueError):
        TextSessionPool(hip_model, 4, 256, no_repeat_ngram_size=1)
