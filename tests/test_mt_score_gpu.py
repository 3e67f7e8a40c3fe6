"""Scoring a given translation with the first-pass text decoder, on the GPU: the token score kernel (csrc/mt_score.hip through
ss_op_mt_token_scores) against the float64 reference of tests/mt_score_ref.py and bit for bit against ss_log_softmax,
ss_batch_mt_score (features, pack-, sharing- and chunk-invariance, refusals), its agreement with the forced-prefix scores of the
search, the reference's own SequenceScorer run of tests/golden/mt_score.npz, and the surfaces on top (generators.SequenceScorer,
offline --score-reference / --speak-reference).

Every output starts as NaN / a sentinel: a row that answers nothing must still hold it.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import mt_score_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -7777
SS_ERR_ARG, SS_ERR_CAPACITY = 2, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mt_score.npz")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_op(lib, x, tgt, V, ld=None, rows=None, null=None):
    """One ss_op_mt_token_scores call on host logits [rows, ld] -> (rc, stat [rows, 2], idx [rows, 2]) on the host."""
    dx = torch.from_numpy(x).cuda()
    dt = torch.from_numpy(np.asarray(tgt, dtype=np.int32)).cuda()
    n = x.shape[0]
    stat = torch.full((n, 2), NAN).cuda()
    idx = torch.full((n, 2), SENT, dtype=torch.int32).cuda()
    ptr = {"x": P(dx), "t": P(dt), "stat": P(stat), "idx": P(idx)}
    if null:
        ptr[null] = None
    rc = lib.ss_op_mt_token_scores(S(), ptr["x"], x.shape[1] if ld is None else ld, n if rows is None else rows, V, ptr["t"],
                                   ptr["stat"], ptr["idx"])
    torch.cuda.synchronize()
    return rc, stat.cpu(), idx.cpu()


def log_softmax_cols(lib, x, V):
    """ss_log_softmax of the rows' first V columns -> [rows, V] on the host."""
    dx = torch.from_numpy(np.ascontiguousarray(x[:, :V])).cuda()
    out = torch.empty_like(dx)
    assert lib.ss_log_softmax(S(), P(dx), x.shape[0], V, -1, -1, 0, P(out)) == 0
    torch.cuda.synchronize()
    return out.cpu()


_REF = {}


def _case(name):
    if name not in _REF:
        c = R.op_cases()[name]
        x, tgt = R.case_data(c, name)
        _REF[name] = (c, x, tgt, R.score_ref(np.ascontiguousarray(x[:, :c["V"]]), tgt))
    return _REF[name]


def check_against_ref(name, stat, idx, ref, tgt):
    good = torch.from_numpy(~(ref["bad"] | ref["skip"]))
    bad, skip = torch.from_numpy(ref["bad"] & ~ref["skip"]), torch.from_numpy(ref["skip"])
    assert torch.isnan(stat[skip]).all() and (idx[skip] == SENT).all(), f"{name}: a row with a negative target was written"
    assert torch.isnan(stat[bad]).all() and (idx[bad] == -1).all(), f"{name}: NaN rows answer NaN, NaN, -1, -1"
    assert torch.equal(idx[good, 0].long(), torch.from_numpy(ref["argmax"])[good]), f"{name}: arg-max ids"
    assert torch.equal(idx[good, 1].long(), torch.from_numpy(ref["rank"])[good]), f"{name}: ranks"
    want_t, want_b = torch.from_numpy(ref["target"]), torch.from_numpy(ref["best"])
    inf = good & torch.isinf(want_t)
    fin = good & ~torch.isinf(want_t)
    assert torch.equal(stat[inf, 0].double(), want_t[inf])
    e_t = float((stat[fin, 0].double() - want_t[fin]).abs().max())
    e_b = float((stat[good, 1].double() - want_b[good]).abs().max())
    print(f"MTSCORE op {name}: target {e_t:.3e} best {e_b:.3e} (bound {R.TOL:.0e})")
    assert e_t <= R.TOL and e_b <= R.TOL, (name, e_t, e_b)
    return good


@pytest.mark.parametrize("name", list(R.op_cases()))
def test_op_against_float64_and_log_softmax(lib, name):
    """Ids and ranks exact, NaN and skipped rows as specified, both values within 2e-5 of float64 and the bits ss_log_softmax writes
    at those columns."""
    c, x, tgt, ref = _case(name)
    rc, stat, idx = run_op(lib, x, tgt, c["V"])
    assert rc == 0
    good = check_against_ref(name, stat, idx, ref, tgt)
    lsm = log_softmax_cols(lib, x, c["V"])
    rows = torch.arange(x.shape[0])[good]
    assert _bits(stat[good, 0], lsm[rows, torch.from_numpy(tgt).long()[good]]), f"{name}: the target value is not ss_log_softmax's"
    assert _bits(stat[good, 1], lsm[rows, idx[good, 0].long()]), f"{name}: the best value is not ss_log_softmax's"


def test_register_and_strided_forms_bit_equal(lib):
    """V = 8192 runs in registers, 8193 strided: with a -inf last column the two answer the same bits; and on widths both forms can
    run (ss_debug_mt_score_form) they do too."""
    c, x, tgt, ref = _case("v8193")
    x = x.copy()
    x[:, 8192] = -np.inf
    tgt = np.minimum(tgt, 8191).astype(np.int32)
    rc0, s_str, i_str = run_op(lib, x, tgt, 8193)
    rc1, s_reg, i_reg = run_op(lib, x, tgt, 8192)                # the same rows, ld = 8193
    assert rc0 == 0 and rc1 == 0 and _bits(s_str, s_reg) and torch.equal(i_str, i_reg)
    try:
        for name in ("v1", "v257", "v6000", "v8192", "ties6000", "edge1005", "scale40", "ld"):
            c, x, tgt, ref = _case(name)
            assert lib.ss_debug_mt_score_form(0) == 0
            rc0, s0, i0 = run_op(lib, x, tgt, c["V"])
            assert lib.ss_debug_mt_score_form(1) == 0
            rc1, s1, i1 = run_op(lib, x, tgt, c["V"])
            assert rc0 == 0 and rc1 == 0 and _bits(s0, s1) and torch.equal(i0, i1), name
            check_against_ref(name + "/strided", s1, i1, ref, tgt)
    finally:
        lib.ss_debug_mt_score_form(0)


def test_op_refusals_queue_nothing(lib):
    c, x, tgt, ref = _case("v65")
    for kw in (dict(ld=64), dict(rows=0), dict(rows=-1), dict(V=0), dict(rows=16777216), dict(null="x"), dict(null="t"),
               dict(null="stat"), dict(null="idx")):
        V = kw.pop("V", 65)
        rc, stat, idx = run_op(lib, x, tgt, V, **kw)
        assert rc == SS_ERR_ARG and torch.isnan(stat).all() and (idx == SENT).all(), kw
    rc, stat, idx = run_op(lib, x, np.full(len(tgt), 65, np.int32), 65)       # targets past the row: nothing written, nothing read
    assert rc == 0 and torch.isnan(stat).all() and (idx == SENT).all()


# =================================================================================================
# ss_batch_mt_score
# =================================================================================================
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _enc(model, seed, T):
    from streamspeech_amd import synth
    fb = torch.from_numpy(synth.synth_fbank(seed, T)).to(model.device)
    return model.encoder_forward(fb, 8, 8)


def _text(seed, n, V):
    from streamspeech_amd import synth
    return [int(t) for t in synth.uniform(seed, "mt_score_gpu", (n,), 4, V)]


@pytest.fixture(scope="module")
def utts(model):
    """Encoder rows of 4 utterances."""
    return [_enc(model, seed, T) for seed, T in R.SEARCH_UTTS]


def _same(a, b):
    return (_bits(a["positional_scores"], b["positional_scores"]) and _bits(a["best_lprob"], b["best_lprob"])
            and torch.equal(a["best"], b["best"]) and torch.equal(a["rank"], b["rank"]))


def test_batch_feats_and_pack_invariance(model, utts):
    """d_feats = the bits of ss_batch_mt_features (n_tail_pad 0); a row alone = the same row inside a ragged pack of 5
    (0, 1, 17, 17, 40 tokens); positional scores are log-probabilities, score their mean with </s> counted."""
    V = model.cfg.tgt_vocab
    lens = [0, 1, 17, 17, 40]
    encs = [utts[b % 4] for b in range(5)]
    toks = [_text(10 + b, n, V) for b, n in enumerate(lens)]
    enc = torch.cat(encs, 0)
    Tp = [e.shape[0] for e in encs]
    want = model.batch_mt_features(enc, Tp, toks, [0] * 5)
    pack = model.batch_mt_score(enc, Tp, toks, want_feats=True)
    lean = model.batch_mt_score(enc, Tp, toks)
    for b in range(5):
        r = pack[b]
        assert _bits(r["feats"], want[b]) and lean[b]["feats"] is None and _same(lean[b], r)
        n = lens[b] + 1
        assert r["positional_scores"].shape == (n,) and r["positional_scores"].dtype == torch.float32
        assert r["best"].dtype == torch.int32 and r["rank"].dtype == torch.int32
        assert (r["positional_scores"] <= r["best_lprob"]).all() and (r["best_lprob"] <= 0).all()
        assert torch.equal(r["rank"] == 0, r["best"].long() == torch.tensor(toks[b] + [model.cfg.eos]))
        assert abs(r["score"] - float(r["positional_scores"].double().sum()) / n) < 1e-6
        alone = model.batch_mt_score(encs[b], [Tp[b]], [toks[b]], want_feats=True)[0]
        assert _same(alone, r) and _bits(alone["feats"], r["feats"]), f"row {b} differs alone and in the pack"


def test_batch_src_sharing(model, utts):
    """Three texts for one utterance through h_src = three calls' worth on a copied encoder; mixed with another utterance."""
    V = model.cfg.tgt_vocab
    toks = [_text(30 + k, n, V) for k, n in enumerate((5, 0, 12, 7))]
    enc = torch.cat([utts[1], utts[2]], 0)
    Tp = [utts[1].shape[0], utts[2].shape[0]]
    shared = model.batch_mt_score(enc, Tp, toks, src=[1, 0, 1, 1], want_feats=True)
    copied_enc = torch.cat([utts[2], utts[1], utts[2].clone(), utts[2].clone()], 0)
    copied = model.batch_mt_score(copied_enc, [Tp[1], Tp[0], Tp[1], Tp[1]], toks, want_feats=True)
    for b in range(4):
        assert _same(shared[b], copied[b]) and _bits(shared[b]["feats"], copied[b]["feats"]), b
        u = utts[2] if b != 1 else utts[1]
        assert _same(shared[b], model.batch_mt_score(u, [u.shape[0]], [toks[b]])[0]), b


def test_batch_crosses_the_projection_chunk(model, utts):
    """256 rows of 8 tokens over 4 utterances = 2304 positions, past the 2048-row chunk of the projection: every row is the bits of
    that row scored alone (8 distinct texts per utterance, each scored alone once)."""
    V = model.cfg.tgt_vocab
    texts = [_text(50 + k, 8, V) for k in range(8)]
    enc = torch.cat(utts, 0)
    Tp = [u.shape[0] for u in utts]
    src = [(b * 7) % 4 for b in range(256)]
    pick = [(b * 5 + b // 32) % 8 for b in range(256)]
    got = model.batch_mt_score(enc, Tp, [texts[k] for k in pick], src=src)
    assert sum(len(r["positional_scores"]) for r in got) == 2304
    alone = {}
    for b in range(256):
        key = (src[b], pick[b])
        if key not in alone:
            alone[key] = model.batch_mt_score(utts[key[0]], [Tp[key[0]]], [texts[key[1]]])[0]
        assert _same(got[b], alone[key]), f"row {b} (utterance {key[0]}, text {key[1]})"
    assert len(alone) >= 16


def test_batch_refusals_leave_outputs(model, utts):
    from streamspeech_amd.engine import _i32
    cfg = model.cfg
    e = torch.cat([utts[0], utts[1]], 0)
    Tp = [utts[0].shape[0], utts[1].shape[0]]
    stat = torch.full((64, 2), NAN, device=model.device)
    idx = torch.full((64, 2), SENT, dtype=torch.int32, device=model.device)
    feats = torch.full((3, 8, cfg.dec_dim), NAN, device=model.device)

    def call(U=2, B=3, src=(0, 1, 1), toks=((5, 6), (7,), ()), frows=8, tp=Tp, d_stat=stat):
        flat = [t for ts in toks for t in ts] or [0]
        rc = model.lib.ss_batch_mt_score(model.h, S(), U, P(e), _i32(tp), B, _i32(src) if src is not None else None, _i32(flat),
                                         _i32([len(t) for t in toks]), P(feats), frows, P(d_stat), P(idx))
        torch.cuda.synchronize()
        return rc
    assert call(toks=((5, cfg.pad), (7,), ())) == SS_ERR_ARG                   # pad as a text token
    assert call(toks=((5, cfg.tgt_vocab), (7,), ())) == SS_ERR_ARG             # an id outside the dictionary
    assert call(toks=((5, -1), (7,), ())) == SS_ERR_ARG
    assert call(src=(0, 2, 1)) == SS_ERR_ARG and call(src=(0, -1, 1)) == SS_ERR_ARG
    assert call(U=0) == SS_ERR_ARG and call(U=4, tp=Tp + Tp) == SS_ERR_ARG     # U > B
    assert call(src=None) == SS_ERR_ARG                                        # no h_src needs B == U
    assert call(B=257, src=(0,) * 257, toks=((),) * 257) == SS_ERR_ARG
    assert call(tp=[Tp[0], 0]) == SS_ERR_ARG
    assert call(d_stat=None) == SS_ERR_ARG
    assert call(frows=2) == SS_ERR_CAPACITY                                    # feature rows
    long_text = tuple([5] * (model.max_tgt_pos - 2))                           # 1 + n + 2 > the decoder's positions
    stat2 = torch.full((model.max_tgt_pos + 8, 2), NAN, device=model.device)
    rc = model.lib.ss_batch_mt_score(model.h, S(), 2, P(e), _i32(Tp), 2, None, _i32(list(long_text)), _i32([len(long_text), 0]), None, 0,
                                     P(stat2), P(idx))
    torch.cuda.synchronize()
    assert rc == SS_ERR_CAPACITY and torch.isnan(stat2).all()                  # a text past the position limit
    assert torch.isnan(stat).all() and (idx == SENT).all() and torch.isnan(feats).all()
    assert call() == 0
    assert torch.isfinite(stat[:6]).all() and torch.isnan(stat[6:]).all() and (idx[:6] != SENT).all() and (idx[6:] == SENT).all()


def test_consistent_with_the_search(model, utts):
    """On the greedy hypothesis of each utterance the positional scores agree within 2e-5 with the forced-prefix positional scores of
    batch_mt_beam_continue(prefix = the hypothesis, beam 1, unk penalty 0).  The search never chooses <pad>, nor </s> below min_len
    (position 0 at min_len 1); the plain log_softmax scored here masks nothing, so a token of the hypothesis may rank behind exactly
    those ids.  Beyond that the hypothesis was chosen by the lock-step decode rows, whose float32 arithmetic differs from the
    teacher-forced pass in the last bits: a rank > 0 on its own tokens is allowed only where the two candidates are closer than the
    float32 arithmetic can tell (1e-4 in log-probability), at most one position an utterance.  On the CPU oracle the chosen
    utterances have no such position at all (tests/test_mt_score_cpu.py)."""
    cfg = model.cfg
    for u, enc in enumerate(utts):
        Tp = int(enc.shape[0])
        toks, _ = model.mt_greedy(enc, [], R.SEARCH_MAX_LEN, 1)
        hyp = [t for t in toks if t != model.cfg.eos]
        assert hyp, "an empty greedy hypothesis checks nothing"
        r = model.batch_mt_score(enc, [Tp], [hyp])[0]
        nbest, _ = model.batch_mt_beam_continue(enc, [Tp], [hyp], [len(hyp) + 2], 1, 1, 0.0, True)
        forced = torch.tensor(nbest[0][0]["positional_scores"][:len(hyp)], dtype=torch.float32)
        mine = r["positional_scores"][:len(hyp)]
        err = float((mine.double() - forced.double()).abs().max())
        print(f"MTSCORE search {u}: {len(hyp)} forced tokens, max |score - search| {err:.3e}, bit-equal {_bits(mine, forced)}")
        assert err <= 2e-5, (u, err)
        off = []
        for p in (r["rank"][:len(hyp)] > 0).nonzero().flatten().tolist():
            banned = {cfg.pad, cfg.eos} if p < 1 else {cfg.pad}                # what the search (min_len 1) could not choose at p
            if not (int(r["best"][p]) in banned and int(r["rank"][p]) <= len(banned)):
                off.append(p)
        assert len(off) <= 1, f"utterance {u}: positions {off} of the greedy hypothesis are not the arg-max"
        for p in off:
            assert float(r["best_lprob"][p] - r["positional_scores"][p]) < 1e-4, (u, p)


# =================================================================================================
# the reference's own SequenceScorer (tests/golden/mt_score.npz)
# =================================================================================================
def test_against_reference_fixture(model):
    """Per utterance and text: max |HIP - pos64| <= max(2e-5, 2 x max |pos32 - pos64|) -- no farther from the reference's float64
    run than twice its float32 run is (oracle/adjudicate.py) -- and the same bound divided by the token count for `score`.  The three
    texts of an utterance ride in one call through `src`.  -s prints every case's ratio to its bound (profiles/mt_score_accuracy.txt)."""
    g = np.load(GOLD)
    for u in range(int(g["n"])):
        fb = torch.from_numpy(g[f"fbank{u}"]).to(model.device)
        enc = model.encoder_forward(fb)                          # the offline generator: no chunks
        toks = [[int(t) for t in g[f"tokens{u}_{k}"]] for k in range(3)]
        got = model.batch_mt_score(enc, [enc.shape[0]], [t[:-1] for t in toks], src=[0, 0, 0])
        for k in range(3):
            p32, p64 = g[f"pos32_{u}_{k}"].astype(np.float64), g[f"pos64_{u}_{k}"].astype(np.float64)
            hip = got[k]["positional_scores"].double().numpy()
            assert hip.shape == p64.shape
            e_ref, e_hip = np.abs(p32 - p64).max(), np.abs(hip - p64).max()
            bound = max(2e-5, 2 * e_ref)
            s_err, s_bound = abs(got[k]["score"] - float(g[f"score64_{u}_{k}"])), bound / len(p64)
            print(f"MTSCORE fixture u{u} text{k} ({len(p64)} tokens): hip-ref64 {e_hip:.3e} ref32-ref64 {e_ref:.3e} bound {bound:.3e} "
                  f"ratio {e_hip / bound:.3f}; score err {s_err:.3e} bound {s_bound:.3e} ratio {s_err / s_bound:.3f}")
            assert e_hip <= bound, (u, k, e_hip, bound)
            assert s_err <= s_bound, (u, k, s_err, s_bound)


# =================================================================================================
# surfaces
# =================================================================================================
class _Dict:
    def __init__(self, cfg):
        self.cfg = cfg

    def pad(self):
        return self.cfg.pad

    def eos(self):
        return self.cfg.eos

    def unk(self):
        return self.cfg.unk


def test_sequence_scorer_on_the_engine(model, utts):
    """generators.SequenceScorer over the model wrapper's encoder output = batch_mt_score, padded targets and the empty text included."""
    from streamspeech_amd.generators import SequenceScorer
    cfg = model.cfg
    toks = [_text(70, 9, cfg.tgt_vocab), [], _text(71, 3, cfg.tgt_vocab)]
    L_ = max(len(t) for t in toks) + 1
    target = torch.full((3, L_), cfg.pad, dtype=torch.long)
    for b, t in enumerate(toks):
        target[b, :len(t) + 1] = torch.tensor(t + [cfg.eos])
    eo = [{"encoder_out": [utts[b].unsqueeze(1)]} for b in range(3)]
    out = SequenceScorer(_Dict(cfg), engine=model).generate([None], {"target": target, "encoder_out": eo})
    want = model.batch_mt_score(torch.cat(utts[:3], 0), [u.shape[0] for u in utts[:3]], toks)
    for b in range(3):
        h = out[b][0]
        assert h["tokens"].tolist() == toks[b] + [cfg.eos] and h["attention"] is None and h["alignment"] is None
        assert _bits(h["positional_scores"], want[b]["positional_scores"]) and h["score"] == want[b]["score"]


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_offline_score_and_speak_reference(model, hip_vocoder, synth_weights, tmp_path):
    """offline --score-reference --speak-reference on a tiny synthetic pack: without the flags the result directory is what it is
    with them minus the new files, byte for byte; the scores are batch_mt_score's; ref_wav is the vocoder's output for
    batch_t2u_units of the reference states, and for the row whose reference IS its hypothesis ref_wav equals pred_wav bit for bit."""
    import wave
    from tests import ref_fixtures as RF
    from streamspeech_amd import offline, synth
    from streamspeech_amd.pipeline import units_from_tokens
    cfg = synth_weights[0]
    dicts = RF.dictionaries(cfg)
    secs = [1.3, 2.2, 0.01, 0.9]                                 # one utterance too short to decode
    items = [(20 + i, torch.from_numpy(synth.synth_pcm(80 + i, int(16000 * s))).to(model.device)) for i, s in enumerate(secs)]
    kw = dict(batch_size=2, max_len_a_mt=0.0, max_len_b_mt=6, dur_prediction=True)
    a, b = tmp_path / "a", tmp_path / "b"
    plain = offline.generate(model, hip_vocoder, items, dicts, str(a), "test", **kw)
    # id 20: its own hypothesis; 21: another text; 22: no audio; 23: no reference
    feat, T = model.batch_fbank_cmvn(items[0][1], [int(items[0][1].numel())])
    enc, Tp = model.batch_encoder_forward(feat, T)
    toks, _, _ = model.batch_mt_greedy(enc, Tp, [6])
    hyp20 = [t for t in toks[0] if t != cfg.eos]
    refs = {20: hyp20, 21: _text(90, 5, cfg.tgt_vocab), 22: [7, 8]}
    spoken = offline.generate(model, hip_vocoder, items, dicts, str(b), "test", mt_references=refs, speak_reference=True, **kw)
    ta, tb = _tree(a), _tree(b)
    new = {"generate-test.mt.ref.scores", "generate-test.mt.ref.words", "generate-test.ref.unit", os.path.join("ref_wav", "0_pred.wav"),
           os.path.join("ref_wav", "1_pred.wav")}
    assert set(tb) - set(ta) == new and set(ta) <= set(tb)
    for k in ta:
        assert ta[k] == tb[k], f"{k} differs with the flags"
    assert plain.keys() == spoken.keys()
    rows = {int(r[0]): r for r in (ln.split("\t") for ln in tb["generate-test.mt.ref.scores"].decode().splitlines())}
    assert [rows[i][5] for i in (20, 21, 22, 23)] == ["scored", "scored", "no_audio", "no_reference"]
    for sid, k in ((20, 0), (21, 1)):
        feat, T = model.batch_fbank_cmvn(items[k][1], [int(items[k][1].numel())])
        enc, Tp = model.batch_encoder_forward(feat, T)
        r = model.batch_mt_score(enc, Tp, [refs[sid]], want_feats=True)[0]
        assert int(rows[sid][1]) == len(refs[sid]) + 1
        assert float(rows[sid][2]) == pytest.approx(r["score"], abs=2e-6) and float(rows[sid][3]) == pytest.approx(float(r["positional_scores"].double().sum()), abs=2e-6)
        assert float(rows[sid][4]) == pytest.approx(float((r["rank"] == 0).float().mean()), abs=1e-6)
        units = units_from_tokens(model.batch_t2u_units(r["feats"].unsqueeze(0).contiguous(), [len(refs[sid]) + 1], mask_eos=True)[0], cfg)
        assert tb["generate-test.ref.unit"].decode().split("\n")[k] == " ".join(str(x) for x in units)
        wav, _, _ = hip_vocoder.batch_forward([units], dur_prediction=True)
        with wave.open(str(b / "ref_wav" / f"{k}_pred.wav")) as w:
            got = w.readframes(w.getnframes())
        from streamspeech_amd import frontend
        frontend.write_wav(str(tmp_path / "want.wav"), wav[0].detach().cpu().numpy(), 16000)
        with wave.open(str(tmp_path / "want.wav")) as w:
            assert w.readframes(w.getnframes()) == got, f"ref_wav of {sid} is not the vocoder's output for its reference states"
    assert tb["generate-test.ref.unit"].decode().split("\n")[0] == tb["generate-test.unit"].decode().split("\n")[0]
    assert tb[os.path.join("ref_wav", "0_pred.wav")] == tb[os.path.join("pred_wav", "0_pred.wav")]       # reference == hypothesis
    words = [ln.split("\t") for ln in tb["generate-test.mt.ref.words"].decode().splitlines()]
    assert {int(w[0]) for w in words} == {20, 21} and all(len(w) == 7 for w in words)
    log = dict(ln.split("\t", 1) for ln in tb["generate-test.log"].decode().splitlines())
    assert [w[1] for w in words if w[0] == "20"] == log["D-20"].split()
