"""The cross-attention of the first-pass text search on the GPU: the head-averaged attention probabilities kernel
(csrc/attn_probs.hip through ss_op_attention_probs) against the float64 reference of tests/mt_attention_ref.py, its pack-invariance,
ss_batch_mt_attention (features bit-identical to ss_batch_mt_features, pack-invariant attention, refusals), the reference's own
attention of tests/golden/mt_attention.npz, and the surfaces on top (SequenceGenerator(want_attention=True)).

Op-level data and bounds: tests/mt_attention_ref.py (op_cases, case_bound).  Rows no kernel may read hold NaN (guard rows around and
between the segments of Q and K); P, peak and stat start as NaN / a sentinel and must be written on exactly the owned elements.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import mt_attention_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 3                     # guard rows / elements around and between everything
SENT = -7777              # peak sentinel
SS_ERR_ARG, SS_ERR_CAPACITY = 2, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mt_attention.npz")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Pack:
    """The segments (q, k) of a launch laid out with NaN guard rows, in ``order``; outputs with guard gaps as well."""

    def __init__(self, data, q_first, order=None):
        n = len(data)
        order = list(range(n)) if order is None else order
        self.data, self.q_first = data, list(q_first)
        qpos = kpos = G
        ppos, rpos = G, G
        self.segs, self.p_off, self.row_off = [None] * n, [0] * n, [0] * n
        for s in order:
            q, k = data[s]
            rows = q.shape[0] - q_first[s]
            self.segs[s] = (qpos, q.shape[0], kpos, k.shape[0])
            self.p_off[s], self.row_off[s] = ppos, rpos
            qpos += q.shape[0] + G
            kpos += k.shape[0] + G
            ppos += rows * k.shape[0] + G
            rpos += rows + G
        self.n_p, self.n_r = ppos, rpos
        Q, K = torch.full((qpos, R.D_OP), NAN), torch.full((kpos, R.D_OP), NAN)
        for (qs, ql, ks, kl), (q, k) in zip(self.segs, data):
            Q[qs:qs + ql] = q
            K[ks:ks + kl] = k
        self.Q, self.K = Q, K
        self.dQ, self.dK = Q.cuda(), K.cuda()
        self.max_rows = max(q.shape[0] - f for (q, _), f in zip(data, q_first))

    def launch(self, lib, scale, want_p=True, H=R.H_OP):
        """One ss_op_attention_probs call -> (rc, P flat, peak, stat [n_r, 2]) on the host, outputs started as NaN / SENT."""
        from streamspeech_amd import lib as L
        P = torch.full((self.n_p,), NAN).cuda()
        peak = torch.full((self.n_r,), SENT, dtype=torch.int32).cuda()
        stat = torch.full((self.n_r, 2), NAN).cuda()
        segs = torch.tensor(self.segs, dtype=torch.int32).reshape(-1).cuda()
        qf = torch.tensor(self.q_first, dtype=torch.int32).cuda()
        ro = torch.tensor(self.row_off, dtype=torch.int32).cuda()
        po = torch.tensor(self.p_off, dtype=torch.int64).cuda()
        a = L.SSOpAttnProbsArgs()
        a.Q, a.K, a.ldq, a.ldk, a.H, a.scale = self.dQ.data_ptr(), self.dK.data_ptr(), R.D_OP, R.D_OP, H, scale
        a.segs, a.nseg, a.q_first, a.row_off, a.p_off = segs.data_ptr(), len(self.segs), qf.data_ptr(), ro.data_ptr(), po.data_ptr()
        a.P = P.data_ptr() if want_p else None
        a.peak, a.stat, a.max_rows = peak.data_ptr(), stat.data_ptr(), self.max_rows
        rc = lib.ss_op_attention_probs(S(), C.byref(a))
        torch.cuda.synchronize()
        return rc, P.cpu(), peak.cpu(), stat.cpu()

    def seg_out(self, s, P, peak, stat):
        """Segment s's (P [rows, k_len], peak [rows], stat [rows, 2]) views of a launch's outputs."""
        rows, kl = self.data[s][0].shape[0] - self.q_first[s], self.data[s][1].shape[0]
        return (P[self.p_off[s]:self.p_off[s] + rows * kl].view(rows, kl), peak[self.row_off[s]:self.row_off[s] + rows],
                stat[self.row_off[s]:self.row_off[s] + rows])

    def owned_masks(self):
        mp, mr = torch.zeros(self.n_p, dtype=torch.bool), torch.zeros(self.n_r, dtype=torch.bool)
        for s, (q, k) in enumerate(self.data):
            rows = q.shape[0] - self.q_first[s]
            mp[self.p_off[s]:self.p_off[s] + rows * k.shape[0]] = True
            mr[self.row_off[s]:self.row_off[s] + rows] = True
        return mp, mr


_REF = {}


def _ref(name):
    """float64 and float32 reference of a case, computed once and shared."""
    if name not in _REF:
        c = R.op_cases()[name]
        data = R.case_data(c)
        segs = [(0, q.shape[0], 0, k.shape[0]) for q, k in data]
        r64 = [R.ragged_probs_ref(q, k, R.H_OP, c["scale"], [sg], [f])[0] for (q, k), sg, f in zip(data, segs, c["q_first"])]
        P32 = [R.probs_ref(q[f:], k, R.H_OP, c["scale"], torch.float32) for (q, k), f in zip(data, c["q_first"])]
        _REF[name] = (c, data, r64, R.case_bound(c, [r[0] for r in r64], P32))
    return _REF[name]


@pytest.mark.parametrize("name", [n for n in R.op_cases() if n != "tie"])
def test_op_against_float64(lib, name):
    """Every case of op_cases() but the tie: P and stat[0] within the bound, stat[1] within k_len x the bound, peak equal wherever
    the float64 top-2 gap exceeds twice the bound (at least 90 % of the rows do); outputs written on exactly the owned elements;
    without P the peak and stat bits are the same."""
    c, data, r64, bound = _ref(name)
    order = list(reversed(range(len(data))))                 # the memory order is not the segment order
    pk = Pack(data, c["q_first"], order)
    rc, P, peak, stat = pk.launch(lib, c["scale"])
    assert rc == 0
    mp, mr = pk.owned_masks()
    assert torch.isfinite(P[mp]).all() and torch.isnan(P[~mp]).all(), "P: not exactly the owned elements"
    assert torch.isfinite(stat[mr]).all() and torch.isnan(stat[~mr]).all(), "stat: not exactly the owned rows"
    assert (peak[mr] != SENT).all() and (peak[~mr] == SENT).all(), "peak: not exactly the owned rows"
    decisive = total = 0
    worst = [0.0, 0.0, 0.0]
    for s, (Pr, pkr, str_) in enumerate(r64):
        Ps, pks, sts = pk.seg_out(s, P, peak, stat)
        kl = Pr.shape[1]
        e = [float((Ps.double() - Pr).abs().max()), float((sts[:, 0].double() - str_[:, 0]).abs().max()),
             float((sts[:, 1].double() - str_[:, 1]).abs().max()) / kl]
        worst = [max(a, b) for a, b in zip(worst, e)]
        assert (pks >= 0).all() and (pks < kl).all()
        ok = R.top2_gap(Pr) > 2 * bound
        decisive += int(ok.sum())
        total += ok.numel()
        assert torch.equal(pks[ok].long(), pkr[ok]), f"{name}: segment {s}: peak differs on a decisive row"
        # whatever the peak, stat[0] is P at it
        assert torch.equal(sts[:, 0], Ps.gather(1, pks.long()[:, None])[:, 0]), "stat[0] is not P[peak]"
    print(f"MTATTN {name}: P err={worst[0]:.3e} stat0 err={worst[1]:.3e} stat1 err/k_len={worst[2]:.3e} bound={bound:.3e} "
          f"decisive {decisive}/{total}")
    assert decisive >= 0.9 * total, f"{name}: only {decisive}/{total} decisive rows"
    assert worst[0] <= bound and worst[1] <= bound and worst[2] <= bound, (name, worst, bound)
    rc, P2, peak2, stat2 = pk.launch(lib, c["scale"], want_p=False)
    assert rc == 0 and torch.isnan(P2).all()
    assert torch.equal(peak2, peak) and _bits(stat2[mr], stat[mr]) and torch.isnan(stat2[~mr]).all()


def test_op_tie_lowest_index(lib):
    """Two identical key rows that hold the row maximum: the peak is the lower index, across waves (5 / 100) and within a lane's own
    keys (3 / 67); P within the bound."""
    c, data, r64, bound = _ref("tie")
    pk = Pack(data, c["q_first"])
    rc, P, peak, stat = pk.launch(lib, c["scale"])
    assert rc == 0
    for s, (Pr, pkr, str_) in enumerate(r64):
        j1, j2 = c["ties"][s]
        Ps, pks, sts = pk.seg_out(s, P, peak, stat)
        assert torch.equal(pkr, torch.full_like(pkr, j1)), "the case does not tie at its maximum (a bad case, not a kernel bug)"
        assert _bits(Ps[:, j1], Ps[:, j2])
        assert torch.equal(pks.long(), pkr)
        assert float((Ps.double() - Pr).abs().max()) <= bound
        assert float((sts[:, 0].double() - str_[:, 0]).abs().max()) <= bound


def test_op_pack_invariance(lib):
    """A segment's bits are identical alone, in a pack (any memory order), with another q_first, and after a repeated launch."""
    c = R.op_cases()["ragged3"]
    data = R.case_data(c)
    q, k = data[1]                                           # 37 x 250
    alone = Pack([(q, k)], [0])
    rc, P0, peak0, stat0 = alone.launch(lib, 1.0)
    assert rc == 0
    Pa, pa, sa = alone.seg_out(0, P0, peak0, stat0)
    rc, P1, peak1, stat1 = alone.launch(lib, 1.0)            # repeated
    assert rc == 0 and _bits(P1, P0) and torch.equal(peak1, peak0) and _bits(stat1, stat0)
    for order in ([0, 1, 2], [2, 1, 0], [1, 0, 2]):
        for f in (0, 5, 36):
            pack = Pack(data, [0, f, 5], order)
            rc, P, peak, stat = pack.launch(lib, 1.0)
            assert rc == 0
            Pb, pb, sb = pack.seg_out(1, P, peak, stat)
            assert _bits(Pb, Pa[f:]) and torch.equal(pb, pa[f:]) and _bits(sb, sa[f:]), (order, f)


def test_op_refusals(lib):
    """What the launcher refuses (more heads than the kernel holds) leaves the outputs untouched."""
    c = R.op_cases()["ragged3"]
    pk = Pack(R.case_data(c), c["q_first"])
    rc, P, peak, stat = pk.launch(lib, 1.0, H=9)
    assert rc == SS_ERR_ARG and torch.isnan(P).all() and (peak == SENT).all() and torch.isnan(stat).all()


# =================================================================================================
# ss_batch_mt_attention
# =================================================================================================
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _enc(model, seed, T):
    from streamspeech_amd import synth
    fb = torch.from_numpy(synth.synth_fbank(seed, T)).to(model.device)
    return model.encoder_forward(fb, 8, 8)


@pytest.fixture(scope="module")
def mt_rows(model):
    """(encoder rows, tokens without </s>) of 5 utterances: greedy searches of the single-utterance path."""
    rows = []
    for i in range(5):
        enc = _enc(model, 400 + i, 60 + 23 * i)
        toks, _ = model.mt_greedy(enc, [], 3 + 3 * i, 1)
        rows.append((enc, [t for t in toks if t != model.cfg.eos]))
    return rows


def test_batch_feats_bits_and_pack_invariance(model, mt_rows):
    """d_feats of ss_batch_mt_attention = the bits of ss_batch_mt_features on the same rows; an utterance's attention, peak and stat
    bits are the same alone and in the pack of 5, with and without the matrix, and for a later first position."""
    enc = torch.cat([e for e, _ in mt_rows], 0)
    Tp = [e.shape[0] for e, _ in mt_rows]
    toks = [t for _, t in mt_rows]
    want = model.batch_mt_features(enc, Tp, toks, [0] * len(Tp))
    pack = model.batch_mt_attention(enc, Tp, toks, want_feats=True)
    for (attn, peak, prob, mean, feats), w, tp, t in zip(pack, want, Tp, toks):
        assert _bits(feats, w)
        assert attn.shape == (len(t) + 1, tp) and peak.shape == (len(t) + 1,)
        assert float((attn.sum(1) - 1).abs().max()) < 1e-5
        assert torch.equal(peak.long(), attn.argmax(1)) and _bits(prob, attn.gather(1, peak.long()[:, None])[:, 0])
    lean = model.batch_mt_attention(enc, Tp, toks, want_matrix=False)
    first = [min(2, len(t)) for t in toks]
    late = model.batch_mt_attention(enc, Tp, toks, first=first)
    for b, (e, t) in enumerate(mt_rows):
        attn, peak, prob, mean, _ = model.batch_mt_attention(e, [e.shape[0]], [t])[0]
        assert _bits(attn, pack[b][0]) and torch.equal(peak, pack[b][1]) and _bits(prob, pack[b][2]) and _bits(mean, pack[b][3])
        assert lean[b][0] is None and torch.equal(lean[b][1], peak) and _bits(lean[b][2], prob) and _bits(lean[b][3], mean)
        f = first[b]
        assert _bits(late[b][0], attn[f:]) and torch.equal(late[b][1], peak[f:]) and _bits(late[b][3], mean[f:])


def test_batch_refusals_leave_outputs(model, mt_rows):
    """SS_ERR_ARG (a token outside the dictionary, a first position past the tokens, no encoder rows) and SS_ERR_CAPACITY (attention
    buffer, feature rows) are answered before anything is queued: every output still holds what it held."""
    from streamspeech_amd.engine import _i32, _ptr
    e, t = mt_rows[1]
    Tp, n = e.shape[0], len(t)
    D = model.cfg.dec_dim
    attn = torch.full(((n + 1) * Tp,), NAN, device=model.device)
    peak = torch.full((n + 1,), SENT, dtype=torch.int32, device=model.device)
    stat = torch.full((n + 1, 2), NAN, device=model.device)
    feats = torch.full((1, n + 1, D), NAN, device=model.device)
    off = (C.c_int64 * 1)(-1)

    def call(tp=Tp, toks=t, first=0, frows=n + 1, cap=(n + 1) * Tp, d_peak=peak):
        rc = model.lib.ss_batch_mt_attention(model.h, S(), 1, _ptr(e), _i32([tp]), _i32(toks), _i32([len(toks)]), _i32([first]),
                                             _ptr(feats), frows, _ptr(attn), off, cap, _ptr(d_peak), _ptr(stat))
        torch.cuda.synchronize()
        return rc
    assert call(toks=[999999] + t[1:]) == SS_ERR_ARG
    assert call(first=n + 1) == SS_ERR_ARG
    assert call(first=-1) == SS_ERR_ARG
    assert call(tp=0) == SS_ERR_ARG
    assert call(d_peak=None) == SS_ERR_ARG
    assert call(cap=(n + 1) * Tp - 1) == SS_ERR_CAPACITY
    assert call(frows=n) == SS_ERR_CAPACITY
    assert torch.isnan(attn).all() and (peak == SENT).all() and torch.isnan(stat).all() and torch.isnan(feats).all() and off[0] == -1
    assert call() == 0
    assert torch.isfinite(attn).all() and (peak != SENT).all() and torch.isfinite(feats).all() and off[0] == 0


# =================================================================================================
# the reference's own attention (tests/golden/mt_attention.npz)
# =================================================================================================
def test_against_reference_fixture(model, golden_dir):
    """The golden MT tokens fed teacher-forced over the HIP encoder's output of the golden fbank: the attention against the
    reference's .double() run (tests/make_golden_mt_attention.py), bound max(5e-5, 8 x the float32 reference's own distance from
    it); where that run's top-2 gap exceeds twice the bound the hard alignment equals its arg-max.  Both distances are printed, and written as JSON to the path in
    SS_MT_ATTENTION_RECORD when that is set (how profiles/mt_attention.json got its "fixture" entry)."""
    g = np.load(GOLD)
    worst_hip = worst_ref = 0.0
    decisive = total = 0
    for u in range(int(g["n"])):
        fb = torch.from_numpy(g[f"fbank{u}"]).to(model.device)
        enc = model.encoder_forward(fb)                      # the offline generator: no chunks
        toks = [int(t) for t in g[f"tokens{u}"]]
        a64, a32 = torch.from_numpy(g[f"attn64_{u}"]), torch.from_numpy(g[f"attn32_{u}"])      # [Tp, L]
        attn, peak, _, _, _ = model.batch_mt_attention(enc, [enc.shape[0]], [toks[:-1]])[0]
        assert attn.t().shape == a64.shape
        e_ref = float((a32.double() - a64).abs().max())
        e_hip = float((attn.t().double() - a64).abs().max())
        bound = max(R.TOL, 8 * e_ref)
        print(f"MTATTN fixture {u}: hip-ref64 {e_hip:.3e} ref32-ref64 {e_ref:.3e} bound {bound:.3e}")
        worst_hip, worst_ref = max(worst_hip, e_hip), max(worst_ref, e_ref)
        assert e_hip <= bound, (u, e_hip, bound)
        ok = R.top2_gap(a64.t().contiguous()) > 2 * bound
        decisive += int(ok.sum())
        total += ok.numel()
        assert torch.equal(peak.long()[ok], a64.argmax(0)[ok]), f"utterance {u}: hard alignment differs on a decisive column"
    print(f"MTATTN fixture: worst hip-ref64 {worst_hip:.3e}, worst ref32-ref64 {worst_ref:.3e}, decisive columns {decisive}/{total}")
    if os.environ.get("SS_MT_ATTENTION_RECORD"):
        with open(os.environ["SS_MT_ATTENTION_RECORD"], "w") as f:
            json.dump({"hip_vs_reference_double_run": worst_hip, "reference_float32_vs_its_double_run": worst_ref, "decisive_columns": [decisive, total]}, f)


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


@pytest.mark.parametrize("route", ["mt_greedy", "mt_append", "beam4"])
def test_generator_attention(model, route):
    """generate_decoder(want_attention=True) on the three routes: [src_len, tgt_len] attention and [tgt_len, 2] alignment of
    hypothesis 0, equal to batch_mt_attention of its own tokens; the tokens are those of the generator without the switch."""
    from streamspeech_amd.generators import SequenceGenerator

    class NoGreedy:                      # the engine without the one-call search: the mt_append loop
        def __init__(self, m):
            self._m = m

        def __getattr__(self, k):
            if k == "mt_greedy":
                raise AttributeError(k)
            return getattr(self._m, k)
    eng = NoGreedy(model) if route == "mt_append" else model
    beam = 4 if route == "beam4" else 1
    enc = _enc(model, 77, 143)
    src = torch.zeros((1, enc.shape[0]), dtype=torch.long)
    eo = [{"encoder_out": [enc]}]
    kw = dict(beam_size=beam, max_len_a=0, max_len_b=9, min_len=1)
    for prefix in (None, torch.tensor([[17, 23]])):
        off = SequenceGenerator(eng, _Dict(model.cfg), **kw).generate_decoder(eo, src, None, prefix_tokens=prefix)[0]
        on = SequenceGenerator(eng, _Dict(model.cfg), want_attention=True, **kw).generate_decoder(eo, src, None, prefix_tokens=prefix)[0]
        assert len(on) == len(off)
        for a, b in zip(on, off):
            assert torch.equal(a["tokens"], b["tokens"])
            assert b["attention"] is None and b["alignment"] is None
        assert _bits(on[0]["features"], off[0]["features"])
        toks = on[0]["tokens"].tolist()
        L_, Tp = len(toks), enc.shape[0]
        attn, peak, _, _, _ = model.batch_mt_attention(enc, [Tp], [toks[:-1]])[0]
        assert on[0]["attention"].shape == (Tp, L_) and on[0]["attention"].dtype == torch.float32
        assert _bits(on[0]["attention"], attn.t().contiguous())
        assert on[0]["alignment"].shape == (L_, 2)
        assert torch.equal(on[0]["alignment"][:, 0], attn.argmax(1)) and on[0]["alignment"][:, 1].tolist() == list(range(L_))
        for h in on[1:]:
            assert h["attention"] is None and h["alignment"] is None


class _VocSurface:
    """CodeHiFiGANVocoderWithDur call surface over the shared fixture handle (as tests/test_speech_pool_gpu.py)."""

    def __init__(self, hv):
        self.hip = hv

    def __call__(self, x, dur_prediction=False):
        from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
        return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)


def _rec(o):
    return (o.is_empty, None if o.is_empty else o.content, bool(o.finished))


@pytest.mark.parametrize("kind", ["s2tt", "s2st"])
def test_agents_and_pools_with_alignment(model, hip_vocoder, synth_weights, kind):
    """--mt-alignment / align=True on two short utterances of three segments (320 ms and 960 ms ones): the agent's actions and
    contents (text, or samples -- which fix tokens and units) and the pool's segments are bit-identical with the switch on and off;
    a write adds words and never changes one; the words are those of the committed tokens; the pool's words are the agent's."""
    from tests import ref_fixtures as RF
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    cfg = synth_weights[0]
    cls = StreamSpeechS2TTAgent if kind == "s2tt" else StreamSpeechS2STAgent
    kw = {"vocoder": _VocSurface(hip_vocoder)} if kind == "s2st" else {}
    ctx = [model, model.new_context(), model.new_context(), model.new_context()]
    grew = 0
    for u, seg_ms in enumerate((320, 960)):
        a_on = RF.agent_args(cls, seg_ms, 16000, None, ("--mt-alignment",))
        a_off = RF.agent_args(cls, seg_ms, 16000)
        assert a_on.mt_alignment is True and a_off.mt_alignment is False
        on = RF.set_dicts(cls(a_on, model=StreamSpeechModel.from_engine(ctx[0]), **kw), cfg)
        off = RF.set_dicts(cls(a_off, model=StreamSpeechModel.from_engine(ctx[1]), **kw), cfg)
        p_on = SpeechSessionPool(ctx[2], 1, 128, vocoder=hip_vocoder, align=True)
        p_off = SpeechSessionPool(ctx[3], 1, 128, vocoder=hip_vocoder)
        s_on, s_off = p_on.open(kind, a_off, dicts=RF.dictionaries(cfg)), p_off.open(kind, a_off, dicts=RF.dictionaries(cfg))
        step = 16000 * seg_ms // 1000
        pcm = synth.synth_pcm(900 + u, 3 * step)
        assert on.alignment is None and p_on.alignment(s_on) is None and p_off.alignment(s_off) is None
        prev, calls = [], 0
        for k in range(3):
            seg = dict(content=pcm[k * step:(k + 1) * step].tolist(), sample_rate=16000, finished=k == 2)
            o, q = on.pushpop(SpeechSegment(**seg)), off.pushpop(SpeechSegment(**seg))
            x, y = p_on.step({s_on: SpeechSegment(**seg)})[s_on], p_off.step({s_off: SpeechSegment(**seg)})[s_off]
            assert _rec(o) == _rec(q), (kind, u, k)
            assert _rec(x) == _rec(y), (kind, u, k)
            assert off.alignment is None and p_off.alignment(s_off) is None and p_off.last_step["mt_attention"] == 0
            calls += p_on.last_step["mt_attention"]
            words = on.alignment
            if words is None:
                continue
            assert words[:len(prev)] == prev, "a later write changed an earlier word"
            grew += len(words) > len(prev) > 0
            prev = list(words)
            if k < 2:                                            # (the final write resets the agent: its tokens are gone)
                committed = on.tgt_subwords_indices.reshape(-1).tolist()
                syms = [RF.dictionaries(cfg)["target_unigram"][t] for t in committed]
                assert "".join(w.text for w in words) == "".join(syms).replace("▁", "")
            for w in words:
                assert 0 <= w.start_ms < w.end_ms <= (k + 1) * seg_ms + 40 and 0.0 < w.focus <= 1.0
            pw = p_on.alignment(s_on)
            assert pw is not None and [w[:3] for w in pw] == [w[:3] for w in words]
            assert max(abs(a.focus - b.focus) for a, b in zip(pw, words)) < 1e-4
        assert prev, "the utterance wrote nothing"
        assert calls >= 1
        p_on.close(s_on)
        p_off.close(s_off)
    print(f"MTATTN {kind}: writes that added words to earlier ones: {grew}")
    assert grew >= 1, "no write added words to earlier ones: the frozen-words check would be vacuous"
    for c in ctx:
        c.encoder_stream_set_tail(0)


def test_asr_refuses_alignment(model, synth_weights):
    from tests import ref_fixtures as RF
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    from streamspeech_amd.modules import StreamSpeechModel
    args = RF.agent_args(StreamSpeechASRAgent, 320, 16000, None, ("--mt-alignment",))
    with pytest.raises(ValueError, match="mt-alignment"):
        StreamSpeechASRAgent(args, model=StreamSpeechModel.from_engine(model))


def test_offline_mt_words(model, hip_vocoder, synth_weights, tmp_path):
    """--mt-alignment of the offline driver: generate-<subset>.mt.words has one line per word of every D- hypothesis, every other
    file is byte-identical to a run without the flag (greedy and beam 4)."""
    from tests import ref_fixtures as RF
    from streamspeech_amd import offline, synth
    cfg = synth_weights[0]
    dicts = RF.dictionaries(cfg)
    secs = [1.3, 2.2, 0.01, 0.9]                           # one utterance too short to decode: no words, its lines as ever
    items = [(20 + i, torch.from_numpy(synth.synth_pcm(80 + i, int(16000 * s))).to(model.device)) for i, s in enumerate(secs)]
    for beam in (1, 4):
        kw = dict(batch_size=2, max_len_a_mt=0.0, max_len_b_mt=6, dur_prediction=True, dump_wav=False, beam_mt=beam)
        a, b = tmp_path / f"a{beam}", tmp_path / f"b{beam}"
        offline.generate(model, hip_vocoder, items, dicts, str(a), "test", **kw)
        offline.generate(model, hip_vocoder, items, dicts, str(b), "test", mt_alignment=True, **kw)
        names = sorted(p.name for p in a.iterdir())
        assert sorted(p.name for p in b.iterdir()) == sorted(names + ["generate-test.mt.words"])
        for n in names:
            if (a / n).is_file():
                assert (a / n).read_bytes() == (b / n).read_bytes(), n
        log = {}
        for ln in (b / "generate-test.log").read_text().splitlines():
            k, v = ln.split("\t", 1)
            log[k] = v
        per = {}
        for ln in (b / "generate-test.mt.words").read_text().splitlines():
            sid, word, t0, t1, focus = ln.split("\t")
            assert 0 <= int(t0) < int(t1) and 0.0 < float(focus) <= 1.0
            per.setdefault(int(sid), []).append((word, int(t0), int(t1)))
        assert 22 not in per
        for sid, ws in per.items():
            assert [w for w, _, _ in ws] == log[f"D-{sid}"].split(), sid
            assert all(t1 <= int(secs[sid - 20] * 1000) + 40 for _, _, t1 in ws)
        assert set(per) == {sid for sid in (20, 21, 23) if log[f"D-{sid}"].split()}


def test_endpointed_session_alignment_on_the_stream_clock(model, synth_weights):
    """t0_ms of an endpointed session: the pool cuts a continuous 16-kHz stream into two utterances (the stream of
    tests/test_endpoint_gpu.py); a plain pcm_in session with align, fed exactly the samples each step committed, answers the same
    words on its own utterance clock, and the endpointed session's words are those shifted by the utterance's first stream sample."""
    from tests import ref_fixtures as RF
    from tests import vad_ref as V
    from streamspeech_amd import pcm
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.endpoint import Endpoint
    from streamspeech_amd.text_pool import TextSessionPool
    d = RF.dictionaries(synth_weights[0])
    sr, chunk_ms = 16000, 320
    x = V.make_stream(sr, 71, ((300, 1100), (1400, 1900), (2800, 3400)), 4480, dc=0.02)
    data, per = pcm.encode_host(x, "s16le"), sr * chunk_ms // 1000
    args = RF.agent_args(StreamSpeechS2TTAgent, chunk_ms, sr)
    ep_pool, plain = TextSessionPool(model.new_context(), 1, 512, align=True), TextSessionPool(model.new_context(), 1, 512, align=True)
    a = ep_pool.open("s2tt", args, dicts=d, pcm_in=pcm.PcmFormat("s16le"), endpoint=Endpoint())
    b = plain.open("s2tt", args, dicts=d, pcm_in=pcm.PcmFormat("s16le"))
    at, shifts, compared = 0, set(), 0
    while True:
        lo, hi = at * per * 2, (at + 1) * per * 2
        if lo < len(data):
            ep_pool.push_pcm(a, data[lo:hi], finished=hi >= len(data))
        elif not ep_pool.sessions[a].pending:
            break
        ep_pool.step()
        commit = ep_pool.last_step["endpoint_commits"].get(a)
        if commit is not None:
            first, cnt, fin = commit
            plain.push_pcm(b, data[first * 2:(first + cnt) * 2], finished=fin)
            plain.step()
            assert plain.last_step["mt_attention"] == ep_pool.last_step["mt_attention"]
            if plain.last_step["mt_attention"]:
                we, wp = ep_pool.alignment(a), plain.alignment(b)
                ut = ep_pool.utterances(a)
                start = ut[-1]["start"] if fin else ep_pool.sessions[a].ep.utt_start
                t0 = int(start) * 1000 // sr
                assert we and [(w.text, w.start_ms - t0, w.end_ms - t0) for w in we] == [tuple(w[:3]) for w in wp]
                assert max(abs(x.focus - y.focus) for x, y in zip(we, wp)) < 1e-4
                shifts.add(t0)
                compared += len(we)
            if fin:
                plain.reset(b)
        at += 1
        assert at < 200
    print(f"MTATTN endpointed: {compared} words compared, utterance offsets {sorted(shifts)} ms")
    assert len(shifts) == 2 and max(shifts) > 2000, shifts
