"""The scored CTC search on the GPU (csrc/ctc_scores.hip and its entry points): the two kernels through ss_op_* against
tests/ctc_ref.py and against their unscored twins on the same buffers, then ss_ctc_greedy_scored, ss_batch_ctc_greedy_scored and
the scored pool call on a seeded synthetic checkpoint.

Bounds: ids, tokens, indices, counts and span ends are exact; the token sums are bit-equal to the sequential float32 sum the kernel
promises; the per-frame log-probability is within 2e-5 of the float64 log-softmax of the same float32 logits -- the bound the suite
holds ss_row_max_logprob to (same arithmetic: f32 max, f32 sum of <= 8193 accurate expf terms, one logf)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ctc_ref as R

pytestmark = pytest.mark.gpu

SENT, G = -7, 5
PAD, UNK = 1, 3
TOL = 2e-5


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


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype)).cuda()


def oi(n):
    return torch.full((n,), SENT, dtype=torch.int32, device="cuda")


def of(n):
    return torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- masked_argmax_lprob ---------------------------------------------------------------------------------------------------------
def _run_aml(lib, x, N, masks):
    """x [M, ld] float32 (host) -> (ids [M + G], lprob [M + G], ids of ss_op_masked_argmax [M + G]) with the guards behind them."""
    M, ld = x.shape
    m = list(masks) + [-1] * (3 - len(masks))
    dx = dev(x, np.float32)
    ids, ids0, lp = oi(M + G), oi(M + G), of(M + G)
    assert lib.ss_op_masked_argmax_lprob(S(), P(dx), ld, M, N, m[0], m[1], m[2], P(ids), P(lp)) == 0
    assert lib.ss_op_masked_argmax(S(), P(dx), ld, M, N, m[0], m[1], m[2], -1, P(ids0), None, 0, -1, None, -1) == 0
    torch.cuda.synchronize()
    return ids.cpu().numpy(), lp.cpu().numpy(), ids0.cpu().numpy()


def _check_aml(lib, x, N, masks):
    M = x.shape[0]
    ids, lp, ids0 = _run_aml(lib, x, N, masks)
    want_ids, want_lp = R.masked_argmax_lprob(x, N, masks)
    assert np.array_equal(ids, ids0), "ids differ from ss_op_masked_argmax on the same buffer"
    assert np.array_equal(ids[:M], want_ids) and (ids[M:] == SENT).all()
    assert np.isnan(lp[M:]).all(), "wrote behind the last row"
    nan = np.isnan(want_lp)
    assert np.array_equal(np.isnan(lp[:M]), nan)
    err = np.abs(lp[:M][~nan].astype(np.float64) - want_lp[~nan]).max(initial=0.0)
    print(f"masked_argmax_lprob M={M} N={N} ld={x.shape[1]}: max |lprob - f64| = {err:.3e}")
    assert err < TOL, err
    return lp[:M]


@pytest.mark.parametrize("M,N,ld", [(1, 64, 64), (3, 255, 255), (5, 257, 257), (2, 1005, 1005), (4, 6000, 6000), (2, 8193, 8193),
                                    (3, 2049, 2061), (2, 4097, 4100), (2, 6145, 6145)])
def test_masked_argmax_lprob_random_rows(lib, M, N, ld):
    """The issue's shapes, one ld > N case, and a row just past each register form's width (2048 / 4096 / 6144 / 8192)."""
    x = (np.random.default_rng(N).standard_normal((M, ld)) * 6).astype(np.float32)
    x[:, N:] = 1e9                                         # would win every row, and swamp every sum, if it were read
    _check_aml(lib, x, N, (PAD, UNK))


def test_masked_argmax_lprob_constructed_rows(lib):
    N = 300
    x = (np.random.default_rng(1).standard_normal((8, N)) * 6).astype(np.float32)
    x[0, PAD] = 50.0                                       # the maximum on a masked column
    x[1, 7] = x[1, 200] = 30.0                             # two exactly equal maxima
    x[2, 10:40] = -np.inf
    x[3, 5] = np.nan                                       # one NaN: lprob NaN, ids as if it were -inf
    x[4] = 80.0
    x[5] = -80.0
    x[6, 299] = 40.0                                       # the maximum in the last column
    x[7, 0] = np.nan                                       # the NaN in the first candidate column
    lp = _check_aml(lib, x, N, (PAD, UNK))
    assert np.isnan(lp[3]) and np.isnan(lp[7]) and not np.isnan(lp[[0, 1, 2, 4, 5, 6]]).any()
    assert lp[0] < -9.0                                    # log-softmax FIRST: the masked 50.0 is in the denominator
    # all columns but one masked (three masks: a four-column row)
    y = np.array([[3.0, 9.0, -1.0, 2.0]], np.float32)
    ids, _, _ = _run_aml(lib, y, 4, (0, 1, 3))
    assert ids[0] == 2
    _check_aml(lib, y, 4, (0, 1, 3))


@pytest.mark.parametrize("N", [257, 6000, 8193])
def test_masked_argmax_lprob_row_invariance(lib, N):
    """A row alone and the same row at each position of M = 5: bit-identical."""
    x = (np.random.default_rng(N + 1).standard_normal((5, N)) * 6).astype(np.float32)
    _, lp5, _ = _run_aml(lib, x, N, (PAD, UNK))
    for r in range(5):
        _, lp1, _ = _run_aml(lib, x[r:r + 1].copy(), N, (PAD, UNK))
        assert bits(lp1[:1])[0] == bits(lp5[r:r + 1])[0], r


# ---- ctc_collapse_spans ----------------------------------------------------------------------------------------------------------
def _raw(kind, T, rng):
    if kind == "blank":
        return np.zeros(T, np.int64)
    if kind == "one":
        return np.full(T, 9, np.int64)
    raw = np.repeat(rng.integers(0, 6, T), rng.integers(1, 5, T))[:T]
    if kind == "pads":
        raw[rng.random(T) < 0.3] = PAD
    if kind == "cross" and T > 1024:
        raw[1000:min(T, 1100)] = 7                         # a run over the 1024-frame chunk boundary
    return raw


def _run_spans(lib, raw, lp, segs=None):
    n = len(raw)
    nseg = 0 if segs is None else len(segs)
    d_raw, d_lp = dev(raw, np.int32), dev(lp, np.float32)
    d_segs = None if segs is None else dev(np.asarray(segs).ravel(), np.int32)
    tok, idx, last, cnt = oi(n + G), oi(n + G), oi(n + G), oi(max(nseg, 1) + G)
    tok0, idx0, cnt0 = oi(n + G), oi(n + G), oi(max(nseg, 1) + G)
    tl = of(n + G)
    T = 0 if segs is not None else n
    assert lib.ss_op_ctc_collapse_spans(S(), P(d_raw), P(d_lp), T, 0, PAD, P(tok), P(idx), P(last), P(tl), P(cnt), P(d_segs), nseg) == 0
    assert lib.ss_op_ctc_collapse(S(), P(d_raw), T, 0, PAD, P(tok0), P(idx0), P(cnt0), P(d_segs), nseg) == 0
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()  # noqa: E731
    assert np.array_equal(h(tok), h(tok0)) and np.array_equal(h(idx), h(idx0)) and np.array_equal(h(cnt), h(cnt0)), \
        "tokens / index / count differ from ss_op_ctc_collapse on the same buffer"
    return h(tok), h(idx), h(last), h(tl), h(cnt)


@pytest.mark.parametrize("T", [1, 2, 1023, 1024, 1025, 2049])
def test_ctc_collapse_spans(lib, T):
    rng = np.random.default_rng(T)
    for kind in ("runs", "cross", "blank", "one", "pads"):
        raw = _raw(kind, T, rng)
        lp = (-rng.random(T) * 4).astype(np.float32)
        tok, idx, last, tl, cnt = _run_spans(lib, raw, lp)
        t, i, l, _, s32 = R.collapse_spans(raw, lp, 0, PAD)
        n = len(t)
        assert cnt[0] == n and (cnt[1:] == SENT).all(), kind
        assert tok[:n].tolist() == t and idx[:n].tolist() == i and last[:n].tolist() == l, kind
        assert (last[n:] == SENT).all() and np.isnan(tl[n:]).all(), kind
        assert np.array_equal(bits(tl[:n]), bits(s32)), kind
        if kind == "one":
            assert n == 1 and last[0] == T - 1


def test_ctc_collapse_spans_segmented(lib):
    rng = np.random.default_rng(5)
    lens = [1025, 1, 300]
    raws = [_raw("cross", lens[0], rng), np.array([4]), _raw("pads", lens[2], rng)]
    raw = np.concatenate(raws)
    lp = (-rng.random(len(raw)) * 4).astype(np.float32)
    segs, o = [], 0
    for n in lens:
        segs.append((o, n))
        o += n
    tok, idx, last, tl, cnt = _run_spans(lib, raw, lp, segs)
    t, i, l, s32, counts = R.collapse_spans_segmented(raw.tolist(), lp, segs, 0, PAD)
    assert cnt[:3].tolist() == counts and (cnt[3:] == SENT).all()
    for k in range(len(raw)):
        if t[k] is None:
            assert last[k] == SENT and np.isnan(tl[k])
        else:
            assert (tok[k], idx[k], last[k]) == (t[k], i[k], l[k])
            assert bits([tl[k]])[0] == bits([s32[k]])[0]
    assert (last[len(raw):] == SENT).all() and np.isnan(tl[len(raw):]).all()


# ---- entry points ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _fbank(seed, T, device):
    from streamspeech_amd import synth
    return torch.from_numpy(synth.synth_fbank(seed, T)).to(device)


@pytest.fixture(scope="module")
def encs(model):
    return [model.encoder_forward(_fbank(60 + k, T, model.device), 16, 16) for k, T in enumerate((40, 133, 330))]


def _check_record(rec, raw, what):
    """(tokens, index, last, tok_lprob, lprob) against the collapse of its own raw ids and lprob."""
    t, i, l, _, s32 = R.collapse_spans(raw, rec[4], 0, PAD)
    assert (rec[0], rec[1], rec[2]) == (t, i, l), what
    assert np.array_equal(bits(rec[3]), bits(s32)), what


def test_ctc_greedy_scored(model, encs):
    cfg = model.cfg
    for enc in encs:
        for hd in (0, 1):
            toks0, idx0, raw0, _ = model.ctc_greedy(hd, enc)
            toks, idx, raw, logits, last, tok_lp, lp = model.ctc_greedy(hd, enc, want_logits=True, want_scores=True)
            assert toks == toks0 and idx == idx0 and torch.equal(raw, raw0)
            ids, want = R.masked_argmax_lprob(logits.cpu().numpy(), logits.shape[1], (cfg.pad, cfg.unk))
            assert ids.tolist() == raw.tolist()
            err = np.abs(lp.astype(np.float64) - want).max()
            print(f"ss_ctc_greedy_scored head {hd} Tp {enc.shape[0]}: max |lprob - f64| = {err:.3e}")
            assert err < TOL
            assert (lp <= 0).all()
            _check_record((toks, idx, last, tok_lp, lp), raw.tolist(), (hd, enc.shape[0]))
            # without the logits: the same answer from the library's own scratch
            again = model.ctc_greedy(hd, enc, want_scores=True)
            assert again[0] == toks and again[4] == last and np.array_equal(bits(again[6]), bits(lp))


def test_batch_ctc_greedy_scored_and_its_pack_invariance(model, encs):
    assert model.pack_invariant()
    Tp = [e.shape[0] for e in encs]
    for hd in (0, 1):
        alone = [model.batch_ctc_greedy(hd, e.contiguous(), [e.shape[0]], return_raw=True, return_scores=True)[0] for e in encs]
        for k, e in enumerate(encs):
            _check_record(alone[k], alone[k][5], (hd, k))
        for rot in range(3):                               # every utterance at every position of the pack
            order = [(rot + j) % 3 for j in range(3)]
            packed = torch.cat([encs[k] for k in order], 0).contiguous()
            tp = [Tp[k] for k in order]
            plain = model.batch_ctc_greedy(hd, packed, tp, return_raw=True)
            got = model.batch_ctc_greedy(hd, packed, tp, return_raw=True, return_scores=True)
            for j, k in enumerate(order):
                assert (got[j][0], got[j][1], got[j][5]) == plain[j], (hd, rot, j)
                a = alone[k]
                assert got[j][:3] == a[:3] and got[j][5] == a[5], (hd, rot, j)
                assert np.array_equal(bits(got[j][3]), bits(a[3])) and np.array_equal(bits(got[j][4]), bits(a[4])), (hd, rot, j)


# 4 sessions, 5 steps of the schedule shape of tests/test_stream_pool_gpu.py: chunks of 8 / 16 / 24 rows, 32 fbank frames per step,
# different start offsets, late joins and skipped steps
MAX_ROWS = 96


def _schedule(n_sess=4, n_steps=5):
    sess = []
    for i in range(n_sess):
        sess.append({"seed": 100 + i, "chunk": (8, 16, 24)[i % 3], "join": i % 4, "first": 40 + 7 * i, "skip": (3 + i) % 5})
    steps = []
    for st in range(n_steps):
        row = []
        for i, s in enumerate(sess):
            k = st - s["join"]
            if k < 0 or (k > 0 and k == s["skip"]):
                continue
            row.append((i, s["first"] + 32 * k))
        steps.append(row)
    return sess, steps


@pytest.fixture(scope="module")
def sched(model):
    sess, steps = _schedule()
    fb = [_fbank(s["seed"], s["first"] + 32 * 5, model.device) for s in sess]
    return sess, steps, fb


def _run_pool(model, sess, steps, fb, order="fwd", alone=False, check=False):
    """-> {session: [(n_final, head-0 record, head-1 record)] per step it took part in}, records with raw ids."""
    pool = model.stream_pool(len(sess), MAX_ROWS, scores=True)
    res = {i: [] for i in range(len(sess))}
    for row in steps:
        row = list(reversed(row)) if order == "rev" else list(row)
        for g in ([[x] for x in row] if alone else [row]):
            slots = [i for i, _ in g]
            ch = [sess[i]["chunk"] for i in slots]
            out, views, nf, nc = pool.forward(slots, [fb[i][:T].contiguous() for i, T in g], ch, ch)
            T2 = [v.shape[0] for v in views]
            if check:                                      # one head through ctc(), against the ragged-batch call on the packed output
                for hd in (0, 1):
                    ref = model.batch_ctc_greedy(hd, out, T2, return_raw=True, return_scores=True)
                    got = pool.ctc(hd, return_raw=True)
                    for k in range(len(slots)):
                        assert got[k][:3] == ref[k][:3] and got[k][5] == ref[k][5], (slots[k], hd)
                        for q in (3, 4):                   # both under CANON_SEQ: the same bits
                            assert np.array_equal(bits(got[k][q]), bits(ref[k][q])), (slots[k], hd, q)
            src, tgt = pool.ctc_both()
            for k, i in enumerate(slots):
                res[i].append((nf[k], src[k], tgt[k]))
    return res


def _same_records(a, b):
    return a[:3] == b[:3] and np.array_equal(bits(a[3]), bits(b[3])) and np.array_equal(bits(a[4]), bits(b[4]))


def test_pool_scored_against_the_batch_call_and_across_groupings(model, sched):
    sess, steps, fb = sched
    assert model.pack_invariant()
    a = _run_pool(model, sess, steps, fb, check=True)
    b = _run_pool(model, sess, steps, fb, order="rev")
    c = _run_pool(model, sess, steps, fb, alone=True)
    for i in a:
        assert len(a[i]) == len(b[i]) == len(c[i]) > 0
        prev = None
        for (nf, s0, t0), (nfb, s1, t1), (nfc, s2, t2) in zip(a[i], b[i], c[i]):
            assert nf == nfb == nfc
            for x, y, z in ((s0, s1, s2), (t0, t1, t2)):
                assert _same_records(x, y) and _same_records(x, z), i
            if prev is not None:                           # a final row keeps the bits it had when it became final
                pnf, ps, pt = prev
                assert pnf <= nf
                assert np.array_equal(bits(s0[4][:pnf]), bits(ps[4][:pnf])) and np.array_equal(bits(t0[4][:pnf]), bits(pt[4][:pnf])), i
            prev = (nf, s0, t0)


def test_pool_scored_cache_launches_and_refusals(model):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    # an all-final repeat step runs no head rows
    p = model.stream_pool(4, MAX_ROWS, scores=True)
    x256 = _fbank(7, 256, model.device)
    _, v, nf, nc = p.forward([0], [x256], [8], [8])
    assert nf == [64] and nc == [64]
    first = p.ctc_both()
    rows = p.stats()[1]
    assert rows == 2 * 64
    p.forward([0], [x256], [8], [8])
    again = p.ctc_both()
    assert p.stats()[1] == rows
    for hd in (0, 1):
        assert _same_records(first[hd][0], again[hd][0])
    # an unscored call in between advances only the arg-max cache: the scored call after it still answers every row
    q = model.stream_pool(1, MAX_ROWS, scores=True)
    q.forward([0], [x256], [8], [8])
    q.scores = False
    q.ctc(0)
    q.scores = True
    assert _same_records(q.ctc(0)[0], first[0][0])
    # at most one launch more than the unscored call, whatever the number of sessions
    xs = [_fbank(30 + k, 120, model.device) for k in range(4)]
    extra = []
    for n in (1, 4):
        cost = []
        for scored in (False, True):
            pool = model.stream_pool(4, MAX_ROWS, scores=scored)
            pool.forward(list(range(n)), [x.contiguous() for x in xs[:n]], [16] * n, [16] * n)
            l0 = pool.stats()[0]
            pool.ctc(0)
            cost.append(pool.stats()[0] - l0)
        extra.append(cost[1] - cost[0])
    assert extra[0] == extra[1] and 0 <= extra[0] <= 1, extra
    # refusals
    with pytest.raises(L.StreamSpeechHipError) as e:       # a slot holds rows
        pool.set_scores(False)
    assert e.value.code == L.SS_ERR_ARG and pool.scores
    plain = model.stream_pool(2, MAX_ROWS)
    plain.forward([0], [xs[0]], [16], [16])
    with pytest.raises(L.StreamSpeechHipError) as e:
        plain.set_scores(True)
    assert e.value.code == L.SS_ERR_ARG
    tot = plain._last[1][0]
    with pytest.raises(L.StreamSpeechHipError) as e:       # the scored call without scores on
        plain._ctc_scored(0, 1, [0], plain._last[2], torch.empty(6 * tot + 1, dtype=torch.int32, device=model.device), tot)
    assert e.value.code == L.SS_ERR_ARG
    plain.reset(0)
    plain.set_scores(True)                                 # no slot holds rows any more
    plain.forward([0], [xs[0]], [16], [16])
    assert len(plain.ctc(0)[0]) == 5
    # the float cache is booked on the pool's scratch set; past the cap it is refused and the set stays usable
    sc = Scratch(model.device)
    ctx = model.new_context(sc)
    cp = ctx.stream_pool(4, MAX_ROWS)
    sc.set_cap(sc.bytes() + 64)
    before = sc.bytes()
    with pytest.raises(L.StreamSpeechHipError) as e:
        cp.set_scores(True)
    assert e.value.code == L.SS_ERR_SCRATCH_CAP and sc.bytes() == before and sc.audit()[0] == sc.audit()[1] and not cp.scores
    sc.set_cap(0)
    cp.forward([0], [xs[0]], [16], [16])
    assert cp.ctc(0)[0] == plain.ctc(0)[0][:2]
    cp.reset(0)
    b0 = sc.bytes()
    cp.set_scores(True)
    assert sc.bytes() - b0 == 2 * 4 * MAX_ROWS * 4 and sc.audit()[0] == sc.audit()[1]
    cp.forward([0], [xs[0]], [16], [16])
    assert _same_records(cp.ctc(0)[0], plain.ctc(0)[0])
    cp.reset(0)
    cp.set_scores(False)
    assert sc.bytes() == b0 and sc.audit()[0] == sc.audit()[1]
