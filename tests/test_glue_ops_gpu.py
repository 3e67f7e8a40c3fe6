"""The kernels that turn numbers into decisions and addresses (masked argmax, CTC collapse, durations, the row movers, conv_post,
the beam-search kernels), each run directly through its ss_op_* entry point against the plain references of tests/glue_ref.py.

Outputs start as a sentinel (NaN for floats, -7 for ints) with guard space behind them, and every comparison is over the whole
buffer: what the operation defines must be there and nothing else may have been written.  Ids, counts, copies and the float32
chains are compared exactly; the two kernels with transcendental arithmetic have the bounds the suite already uses for them
(2e-5 for the FP32 elementwise kernels, 1e-5 for log-softmax values).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_ref as R

pytestmark = pytest.mark.gpu

NAN = np.float32("nan")
SENT = -7
G = 5                # guard elements / rows behind every output
CAND = R.CAND


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype)).cuda()


def df(a):
    return dev(a, np.float32)


def di(a):
    return dev(a, np.int32)


def of(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def oi(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


_ALIVE = []


@pytest.fixture(autouse=True)
def _release():
    yield
    torch.cuda.synchronize()
    _ALIVE.clear()


def P(t):
    """Device address of a tensor, which stays allocated to the end of the test: an input built inside a call's argument list would
    otherwise hand its memory to the next one before the kernel has run."""
    if t is None:
        return None
    _ALIVE.append(t)
    return C.c_void_p(t.data_ptr())


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want):
    """Bit-for-bit over the whole buffer (NaN sentinels included)."""
    got, want = host(got) if torch.is_tensor(got) else got, np.asarray(want)
    if got.dtype == np.float32:
        want = np.ascontiguousarray(want, np.float32)
        bad = np.nonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())[0]
    else:
        bad = np.nonzero(got.ravel() != want.astype(got.dtype).ravel())[0]
    assert got.shape == want.shape and bad.size == 0, \
        f"{bad.size} elements differ, first at {bad[:5]}: got {got.ravel()[bad[:5]]} want {want.ravel()[bad[:5]]}"


def ok(rc):
    assert rc == 0, f"return code {rc}"


# ---- masked argmax ---------------------------------------------------------------------------------------------------------------
def _argmax_rows(N, ld):
    """~300 rows: random ones, then the tie / NaN / infinity rows the width allows.  Columns N .. ld - 1 hold a value that would
    win every row if it were read."""
    rng = np.random.default_rng(N)
    x = rng.standard_normal((300, ld)).astype(np.float32)
    r = 260
    for a, b in ((5, 69), (255, 256), (7, 263), (200, 300)):
        if b < N:
            x[r, a] = x[r, b] = 9.0
            x[r + 1, a] = x[r + 1, b] = np.inf                     # +inf ties
            r += 2
    x[r] = 2.0                                                      # all equal
    x[r + 1] = np.nan
    x[r + 2] = -np.inf
    x[r + 3, ::3] = np.nan                                          # scattered NaN
    x[r + 4, 1::2] = np.nan
    x[r + 5] = np.nan
    x[r + 5, N - 1] = -np.inf                                       # NaN and -inf only: still the first unmasked column
    x[r + 6, : N // 2] = -np.inf
    x[:, N:] = 3e38
    return x


@pytest.mark.parametrize("N", [1, 63, 64, 255, 256, 257, 1005, 6000])
def test_masked_argmax(lib, N):
    ld = N + 3
    x = _argmax_rows(N, ld)
    M = x.shape[0]
    dx = df(x)
    rng = np.random.default_rng(N + 1)
    masksets = [(-1, -1, -1)]
    if N >= 4:
        m = (N // 2, 0, N - 1)
        # the maximum under each of the three masks, row by row
        for i in range(0, 240, 4):
            x[i, m[(i // 4) % 3]] = 50.0
        dx = df(x)
        masksets += [m, (m[1], -1, m[0]), (2, 2, 2), (-1, 3, -1)]
    lens = rng.integers(2, 5, M)
    for mk in masksets:
        calls = [dict(), dict(force=min(7, N - 1)), dict(row_max_len=lens, step=3, force_id=min(2, N - 1))]
        if N >= 4:
            calls.append(dict(row_min_len=lens, step=3, ban_id=1))
            calls.append(dict(row_max_len=lens, step=2, force_id=0, row_min_len=lens[::-1].copy(), ban_id=N - 2))
        for kw in calls:
            ids = oi(M + G)
            rml = di(kw["row_max_len"]) if "row_max_len" in kw else None
            rmn = di(kw["row_min_len"]) if "row_min_len" in kw else None
            ok(lib.ss_op_masked_argmax(S(), P(dx), ld, M, N, mk[0], mk[1], mk[2], kw.get("force", -1), P(ids), P(rml),
                                       kw.get("step", 0), kw.get("force_id", -1), P(rmn), kw.get("ban_id", -1)))
            want = np.full(M + G, SENT)
            want[:M] = R.masked_argmax(x, N, mk, **kw)
            same(ids, want)


# ---- CTC collapse ----------------------------------------------------------------------------------------------------------------
def _ctc_inputs(T, V, blank):
    """Named frame sequences of length T: random runs, the chunk-boundary runs the length allows, all blank, all pad (= 1)."""
    out = {"runs": R.ctc_frames(T, V, T + blank)}
    other = 5 if blank != 5 else 6
    if T > 1026:
        a = R.ctc_frames(T, V, T + 7)
        a[1022:1027] = other                     # one id over 1022 .. 1026: kept once, at 1022 (or earlier)
        a[1021], a[1027] = other + 1, other + 2
        out["run over 1024"] = a
    if T > 1024:
        a = R.ctc_frames(T, V, T + 8)
        a[1000:1024] = other                     # a run that ends at 1023, a different id at 1024
        a[1024] = other + 1
        out["run to 1023"] = a
        a = a.copy()
        a[1024] = other                          # ... and the same id at 1024: must not be kept twice
        out["run through 1023|1024"] = a
    if T > 64:
        a = R.ctc_frames(T, V, T + 9)
        a[60:68] = other
        out["run over 63|64"] = a
        a = a.copy()
        a[64:68] = other + 1
        out["run to 63"] = a
    out["all blank"] = np.full(T, blank)
    out["all pad"] = np.full(T, 1)
    return out


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 3000])
def test_ctc_collapse(lib, T):
    V = 10
    for blank in (0, V - 1):
        for name, raw in _ctc_inputs(T, V, blank).items():
            tok, idx, cnt = oi(T + G), oi(T + G), oi(1 + G)
            ok(lib.ss_op_ctc_collapse(S(), P(di(raw)), T, blank, 1, P(tok), P(idx), P(cnt), None, 0))
            wt, wi = R.ctc_collapse(raw, blank, 1)
            want_t, want_i, want_c = np.full(T + G, SENT), np.full(T + G, SENT), np.full(1 + G, SENT)
            want_t[:len(wt)], want_i[:len(wi)], want_c[0] = wt, wi, len(wt)
            for got, want in ((cnt, want_c), (tok, want_t), (idx, want_i)):
                try:
                    same(got, want)
                except AssertionError as e:
                    raise AssertionError(f"T={T} blank={blank} {name}: {e}") from None


def _pack(lens, gap=2):
    """Segment starts for the lengths, `gap` unused elements between neighbours."""
    starts, o = [], gap
    for n in lens:
        starts.append(o)
        o += n + gap
    return starts, o


def test_ctc_collapse_segs(lib):
    V, lens = 10, [1, 700, 0, 1024, 2500]
    starts, total = _pack(lens)
    for blank in (0, V - 1):
        raw = np.full(total, 3)                  # gap frames equal to a plausible id: a segment's first frame never looks back
        for s, (st, n) in enumerate(zip(starts, lens)):
            raw[st:st + n] = R.ctc_frames(n, V, 31 * s + blank)
        raw[starts[4] + 1020:starts[4] + 1030] = 4
        raw[starts[3]] = 3                       # first frame of a segment equal to the gap frame before it: still kept
        segs = np.array([[st, n] for st, n in zip(starts, lens)])
        tok, idx, cnt = oi(total + G), oi(total + G), oi(len(lens) + G)
        ok(lib.ss_op_ctc_collapse(S(), P(di(raw)), max(lens), blank, 1, P(tok), P(idx), P(cnt), P(di(segs)), len(lens)))
        want_t, want_i, want_c = np.full(total + G, SENT), np.full(total + G, SENT), np.full(len(lens) + G, SENT)
        for s, (st, n) in enumerate(zip(starts, lens)):
            wt, wi = R.ctc_collapse(raw[st:st + n], blank, 1)
            want_t[st:st + len(wt)], want_i[st:st + len(wi)], want_c[s] = wt, wi, len(wt)
        same(cnt, want_c)
        same(tok, want_t)
        same(idx, want_i)


# ---- durations, repeat_interleave ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 64, 65, 1024, 1025, 2500])
def test_dur_predict(lib, K):
    x = R.dur_inputs(K, K)
    forced = R.forced_durs(K, K)
    for kw, dx, dfc in ((dict(logdur=x), df(x), None), (dict(forced=forced), df(np.full(K, np.nan)), di(forced))):
        dur, cum = oi(K + G), oi(K + 1 + G)
        ok(lib.ss_op_dur_predict(S(), P(dx), P(dfc), K, P(dur), P(cum), None, 0))
        wd, wc = R.dur_predict(**kw)
        same(dur, np.concatenate([wd, np.full(G, SENT)]))
        same(cum, np.concatenate([wc, np.full(G, SENT)]))


def _dur_segs(lens, forced):
    """Packed units of several utterances: values, segs {start, len}, expected dur (packed) and cum (segment s at start + s)."""
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    total = int(np.sum(lens))
    vals = np.concatenate([(R.forced_durs(n, 7 + s) if forced else R.dur_inputs(n, 7 + s)) for s, n in enumerate(lens)])
    want_d, want_c = np.full(total + G, SENT), np.full(total + len(lens) + G, SENT)
    for s, (st, n) in enumerate(zip(starts, lens)):
        d, c = R.dur_predict(forced=vals[st:st + n]) if forced else R.dur_predict(vals[st:st + n])
        want_d[st:st + n] = d
        want_c[st + s:st + s + n + 1] = c
    return vals, np.stack([starts, lens], 1), want_d, want_c


@pytest.mark.parametrize("forced", [False, True])
def test_dur_predict_segs(lib, forced):
    lens = [1, 700, 0, 1024, 2500]
    vals, segs, want_d, want_c = _dur_segs(lens, forced)
    dur, cum = oi(len(want_d)), oi(len(want_c))
    x = df(np.full(len(vals), np.nan)) if forced else df(vals)
    ok(lib.ss_op_dur_predict(S(), P(x), P(di(vals)) if forced else None, 0, P(dur), P(cum), P(di(segs)), len(lens)))
    same(dur, want_d)
    same(cum, want_c)


@pytest.mark.parametrize("D", [1, 128, 257])
def test_repeat_rows(lib, D):
    rng = np.random.default_rng(D)
    durs = [R.dur_predict(R.dur_inputs(K, K))[0] for K in (1, 65, 1025)] + [R.forced_durs(K, K) for K in (8, 65, 1025)]
    durs.append(np.array([0, 0, 3, 0, 0, 2, 0, 0]))          # zeros at the front, in the middle, at the end
    for d in durs:
        K, cum = len(d), R.dur_predict(forced=d)[1]
        F = int(cum[-1])
        emb = rng.standard_normal((K, D)).astype(np.float32)
        out = of(F + G, D)
        ok(lib.ss_op_repeat_rows(S(), P(df(emb)), P(di(cum)), K, D, P(out), F, None, 0))
        same(out, np.concatenate([R.repeat_rows(emb, d), np.full((G, D), NAN)]))


@pytest.mark.parametrize("D", [1, 257])
def test_repeat_rows_segs(lib, D):
    lens = [1, 700, 0, 1024, 300]
    vals, segs, _, want_c = _dur_segs(lens, True)
    rng = np.random.default_rng(D)
    emb = rng.standard_normal((len(vals), D)).astype(np.float32)
    frames = [int(np.sum(vals[st:st + n])) for st, n in segs]
    fstart, ftotal = _pack(frames)
    rs = np.array([[st, n, fs, nf] for (st, n), fs, nf in zip(segs, fstart, frames)])
    out = of(ftotal + G, D)
    ok(lib.ss_op_repeat_rows(S(), P(df(emb)), P(di(want_c)), 0, D, P(out), max(frames), P(di(rs)), len(lens)))
    want = np.full((ftotal + G, D), NAN)
    for (st, n), fs, nf in zip(segs, fstart, frames):
        want[fs:fs + nf] = R.repeat_rows(emb[st:st + n], vals[st:st + n])
    same(out, want)


# ---- embeddings and row movers ---------------------------------------------------------------------------------------------------
def _lattice(rng, *shape):
    """Multiples of 2^-8 in [-4, 4]: 16 * a + b is exact in float32 whether or not the kernel fuses it."""
    return (rng.integers(-1024, 1025, shape) / 256.0).astype(np.float32)


@pytest.mark.parametrize("D", [256, 300])
def test_embed_tokens(lib, D):
    rng = np.random.default_rng(D)
    vocab, pos_rows, pad = 50, 40, 1
    emb, pos = _lattice(rng, vocab, D), _lattice(rng, pos_rows, D)
    tok = np.concatenate([rng.integers(0, vocab, 20), [pad, -3, vocab, 1000, pad, 0, vocab - 1]])
    n = len(tok)
    for stride in (0, 1):
        for pad_id in (pad, -1):
            out = of(n + G, D)
            ok(lib.ss_op_embed_tokens(S(), P(di(tok)), P(df(emb)), P(df(pos)), 16.0, 2, P(out), n, D, stride, pad_id, vocab))
            same(out, np.concatenate([R.embed_tokens(tok, emb, pos, 16.0, 2, stride, pad_id), np.full((G, D), NAN)]))
    row_pos = rng.integers(0, 30, n)
    row_pos[3], row_pos[7], row_pos[8] = pos_rows - 3, pos_rows - 2, 500       # the last row exactly, one past it, far past it
    for pad_id in (pad, -1):
        out = of(n + G, D)
        ok(lib.ss_op_embed_tokens_rows(S(), P(di(tok)), P(df(emb)), P(df(pos)), pos_rows, 16.0, 2, P(di(row_pos)), P(out), n, D,
                                       pad_id, vocab))
        same(out, np.concatenate([R.embed_tokens(tok, emb, pos, 16.0, 2, 0, pad_id, row_pos=row_pos), np.full((G, D), NAN)]))


@pytest.mark.parametrize("up", [1, 25])
@pytest.mark.parametrize("D", [300, 512])
def test_upsample_add_pos(lib, up, D):
    rng = np.random.default_rng(up + D)
    n = 9
    src, pos = _lattice(rng, n, D), _lattice(rng, D)
    src[2, 0] = src[8, 0] = 1.0                  # rows that start with the pad value get no position
    src[3, 1] = 1.0                              # ... the value elsewhere in the row does not count
    out = of(n * up + G, D)
    ok(lib.ss_op_upsample_add_pos(S(), P(df(src)), n, up, P(df(pos)), 1.0, P(out), D))
    same(out, np.concatenate([R.upsample_add_pos(src, up, pos, 1.0), np.full((G, D), NAN)]))


@pytest.mark.parametrize("D", [300, 512])
def test_gather_scatter_rows(lib, D):
    rng = np.random.default_rng(D)
    rows = 37
    table = rng.standard_normal((rows, D)).astype(np.float32)
    idx = np.concatenate([rng.integers(0, rows, 30), [-1, rows, 10 ** 6, 0, rows - 1]])
    out = of(len(idx) + G, D)
    ok(lib.ss_op_gather_rows(S(), P(di(idx)), P(df(table)), D, P(out), len(idx), rows))
    same(out, np.concatenate([R.gather_rows(idx, table), np.full((G, D), NAN)]))
    lds, ldd, n = D + 3, D + 7, 30
    src = rng.standard_normal((n, lds)).astype(np.float32)
    dst_row = rng.permutation(rows + 4)[:n] - 2                                 # distinct; some below 0, some past the end
    dst_row[0], dst_row[1] = -(2 ** 31), 2 ** 31 - 1
    dst = of(rows + G, ldd)
    ok(lib.ss_op_scatter_rows(S(), P(di(dst_row)), P(df(src)), lds, P(dst), ldd, D, n, rows))
    want = R.scatter_rows(np.where(dst_row >= rows, -1, dst_row), src, np.full((rows + G, ldd), NAN), D)
    same(dst, want)


# ---- rows past 65535 -------------------------------------------------------------------------------------------------------------
BIG = [65535, 65536, 70001]


@pytest.mark.parametrize("n", BIG)
def test_rows_past_the_y_extent(lib, n):
    """The row-indexed launchers at row counts around and past 65535 (the y extent other launchers of the project stop at)."""
    D = 4
    rng = np.random.default_rng(n)
    vocab = 50
    emb, pos = _lattice(rng, vocab, D), _lattice(rng, 40, D)
    tok = rng.integers(0, vocab, n)
    out = of(n + G, D)
    ok(lib.ss_op_embed_tokens(S(), P(di(tok)), P(df(emb)), P(df(pos)), 16.0, 2, P(out), n, D, 0, 1, vocab))
    same(out, np.concatenate([R.embed_tokens(tok, emb, pos, 16.0, 2, 0, 1), np.full((G, D), NAN)]))
    row_pos = rng.integers(0, 60, n)
    out = of(n + G, D)
    ok(lib.ss_op_embed_tokens_rows(S(), P(di(tok)), P(df(emb)), P(df(pos)), 40, 16.0, 2, P(di(row_pos)), P(out), n, D, -1, vocab))
    same(out, np.concatenate([R.embed_tokens(tok, emb, pos, 16.0, 2, 0, -1, row_pos=row_pos), np.full((G, D), NAN)]))

    src = _lattice(rng, n, D)
    src[::5, 0] = 1.0
    out = of(n + G, D)
    ok(lib.ss_op_upsample_add_pos(S(), P(df(src)), n, 1, P(df(pos[3])), 1.0, P(out), D))
    same(out, np.concatenate([R.upsample_add_pos(src, 1, pos[3], 1.0), np.full((G, D), NAN)]))

    table = rng.standard_normal((n, D)).astype(np.float32)
    idx = rng.integers(0, n, n)
    out = of(n + G, D)
    ok(lib.ss_op_gather_rows(S(), P(di(idx)), P(df(table)), D, P(out), n, n))
    same(out, np.concatenate([R.gather_rows(idx, table), np.full((G, D), NAN)]))

    dst_row = rng.permutation(n + 10)[:n] - 5
    dst = of(n + G, D)
    ok(lib.ss_op_scatter_rows(S(), P(di(dst_row)), P(df(table)), D, P(dst), D, D, n, n))
    same(dst, R.scatter_rows(np.where(dst_row >= n, -1, dst_row), table, np.full((n + G, D), NAN), D))

    K = 1000
    d = rng.multinomial(n, np.ones(K) / K)
    cum = R.dur_predict(forced=d)[1]
    out = of(n + G, D)
    ok(lib.ss_op_repeat_rows(S(), P(df(table[:K])), P(di(cum)), K, D, P(out), n, None, 0))
    same(out, np.concatenate([R.repeat_rows(table[:K], d), np.full((G, D), NAN)]))


def test_upsample_rows_past_the_y_extent(lib):
    """2801 tokens x 25: what 128 utterances of 22 tokens make of the unit decoder's input."""
    D, n, up = 4, 2801, 25
    rng = np.random.default_rng(2801)
    src, pos = _lattice(rng, n, D), _lattice(rng, D)
    src[::7, 0] = 1.0
    out = of(n * up + G, D)
    ok(lib.ss_op_upsample_add_pos(S(), P(df(src)), n, up, P(df(pos)), 1.0, P(out), D))
    same(out, np.concatenate([R.upsample_add_pos(src, up, pos, 1.0), np.full((G, D), NAN)]))


# ---- conv_post + tanh ------------------------------------------------------------------------------------------------------------
CP_T = [1, 3, 4, 255, 256, 257, 1000]


def _conv_post_case(C_):
    rng = np.random.default_rng(C_)
    starts, total = _pack(CP_T)
    x = np.full((total, C_), NAN, np.float32)       # NaN between the segments: a tap that reaches over an edge shows
    for st, T in zip(starts, CP_T):
        x[st:st + T] = rng.standard_normal((T, C_))
    w = (rng.standard_normal((7, C_)) * (7 * C_) ** -0.5).astype(np.float32)
    return x, w, np.array([0.1], np.float32), starts, total


@pytest.mark.parametrize("C_", [16, 32])
def test_conv_post_tanh_and_crop(lib, C_):
    x, w, bias, starts, total = _conv_post_case(C_)
    dx, dw, db = df(x), df(w), df(bias)
    want = np.full(total + G, np.nan)
    for st, T in zip(starts, CP_T):
        want[st:st + T] = R.conv_post_tanh(x[st:st + T], w, bias[0])
    segs = np.array([[st, T] for st, T in zip(starts, CP_T)])
    full = of(total + G)
    ok(lib.ss_op_conv_post_tanh(S(), P(dx), max(CP_T), C_, P(dw), P(db), 0.01, P(full), P(di(segs)), len(CP_T)))
    full = host(full)
    assert np.array_equal(np.isnan(full), np.isnan(want))                       # exactly the segments' samples were written
    err = np.nanmax(np.abs(full - want))
    print(f"conv_post_tanh C={C_}: max abs error {err:.3e}")
    assert err <= 2e-5
    # the single-utterance form of every length: the same bits as the ragged launch
    for st, T in zip(starts, CP_T):
        one = of(T + G)
        ok(lib.ss_op_conv_post_tanh(S(), C.c_void_p(dx.data_ptr() + 4 * st * C_), T, C_, P(dw), P(db), 0.01, P(one), None, 0))
        same(one, np.concatenate([full[st:st + T], np.full(G, NAN)]))
    # the crop form: every first the issue names, per segment; outputs staggered with gaps
    crops = []
    for st, T in zip(starts, CP_T):
        for first in sorted({f for f in (0, 1, 255, 256, T - 1) if f < T}):
            crops.append((st, T, first))
    o0, ototal = _pack([T - f for _, T, f in crops], gap=3)
    cs = np.array([[st, T, f, o] for (st, T, f), o in zip(crops, o0)])
    out = of(ototal + G)
    ok(lib.ss_op_conv_post_tanh_crop(S(), P(dx), C_, P(dw), P(db), 0.01, P(out), P(di(cs)), len(cs), max(T - f for _, T, f in crops)))
    wantc = np.full(ototal + G, NAN)
    for (st, T, f), o in zip(crops, o0):
        wantc[o:o + T - f] = full[st + f:st + T]
    same(out, wantc)


# ---- beam search: per-row top 2k -------------------------------------------------------------------------------------------------
PAD, UNK, EOS = 1, 3, 2


@pytest.mark.parametrize("t_step,pen", [(0, 0.0), (2, 0.5625)])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
@pytest.mark.parametrize("Vn", ["2k+1", 300, 6000])
def test_beam_topk(lib, Vn, k, t_step, pen):
    """Logits on a 1/8 lattice (the penalty on a 1/16 one): two candidates of a row have equal logits, hence equal scores in any
    arithmetic, or scores at least 0.0625 apart."""
    V = 2 * k + 1 if Vn == "2k+1" else Vn
    unk = UNK if V > UNK else -1                                                # V = 3 (k = 1): a vocabulary without <unk>
    rng = np.random.default_rng(V * 64 + k + t_step)
    B, min_len = 6, 2
    R_ = B * k
    logits = (rng.integers(-32, 33, (R_, V)) / 8.0).astype(np.float32)
    logits[:, V // 2:] = np.minimum(logits[:, V // 2:], 1.0)                    # plenty of duplicates of the best values
    cum = (rng.integers(-40, 1, R_) / 8.0).astype(np.float32)
    #        free     prefix    at max_len      done   NaN row     past max_len
    npre = [0,       1,        2,              0,     2,          3]
    mxl = [10,       10,       t_step + 2,     10,    10,         t_step + 1]
    done = [0,       0,        0,              1,     0,          0]
    logits[4 * k, V - 1] = np.nan
    if k > 1:
        logits[4 * k + 1, 0] = np.nan
    cs, ct = of(R_ + G, CAND), oi(R_ + G, CAND)
    ok(lib.ss_op_beam_topk(S(), P(df(logits)), R_, V, k, t_step, min_len, P(di(mxl)), P(di(npre)), P(di(done)), P(df(cum)),
                           PAD, unk, EOS, pen, P(cs), P(ct)))
    want = R.beam_topk(logits, k, t_step, min_len, mxl, npre, done, cum, PAD, unk, EOS, pen)
    assert set(want) == {r for r in range(R_) if not done[r // k] and (t_step > 0 or r % k == 0)}
    wt = np.full((R_ + G, CAND), SENT)
    ws = np.full((R_ + G, CAND), np.nan)
    for r, (s, t) in want.items():
        assert len(t) == min(2 * k, V - 1)
        ws[r, :len(s)], wt[r, :len(t)] = s, t
    same(ct, wt)
    cs = host(cs)
    assert np.array_equal(np.isnan(cs), np.isnan(ws))
    inf = np.isinf(ws)
    assert np.array_equal(cs[inf], ws[inf].astype(np.float32))
    fin = np.isfinite(ws)
    err = np.max(np.abs(cs[fin] - ws[fin])) if fin.any() else 0.0
    print(f"beam_topk V={V} k={k} t={t_step}: max score error {err:.3e}")
    assert err <= 1e-5
    # at the length limit: </s> first, then -inf entries in index order
    nc = min(2 * k, V - 1)
    for r in [u * k + j for u in (2, 5) for j in range(k if t_step > 0 else 1)]:
        assert wt[r, 0] == EOS and np.isfinite(ws[r, 0]) and np.all(np.isinf(ws[r, 1:nc]))
        assert wt[r, 1:nc].tolist() == [n for n in range(V) if n != EOS][:nc - 1]


# ---- beam search: merge + step logic ---------------------------------------------------------------------------------------------
def _cand_list(rng, V, nc, n_finite, eos_at=None):
    """One sorted per-row list as beam_topk_kernel makes it: scores from a handful of 1/8 multiples (many ties, within the list and
    with the other lists), descending, equal scores in token order; entries from n_finite on are -inf in token order."""
    tok = rng.choice(np.setdiff1d(np.arange(V), [EOS]), nc, replace=False)
    s = np.sort(rng.integers(-6, 0, nc) / 8.0)[::-1].copy()
    s[n_finite:] = -np.inf
    if eos_at is not None:
        tok[eos_at] = EOS
        if eos_at == 0:
            s[0] = 0.0                           # above every other score: among the first k of the merge whatever the other lists hold
    for v in np.unique(s):                       # equal scores: ascending token
        m = s == v
        tok[m] = np.sort(tok[m])
    return s.astype(np.float32), tok


def _merge_state(k, t_step, c0, seed):
    rng = np.random.default_rng(seed)
    V = max(40, 2 * k + 8)
    # utterance:  0 ties, no </s>   1 mostly -inf, no </s>   2 </s> on top + an ignored slot   3 </s> on top, table one short of full
    #             4 </s> only past the first k, the first k all ignored   5 done   6 at its length limit (</s>, then -inf)   7 </s> at -inf: not a candidate
    B = 8
    R_, nc, Lc = B * k, 2 * k, c0 + t_step + 2 + 3
    ci = c0 + t_step
    st = dict(
        tok=np.full((t_step + 2, R_), SENT), cum=np.full((t_step + 2, R_), np.nan, np.float32),
        anc=np.full((2, R_, Lc), SENT), cand_s=np.full((R_, CAND), np.nan, np.float32), cand_t=np.full((R_, CAND), SENT),
        ignore=np.zeros(R_, int), done=np.zeros(B, int), max_len=np.full(B, 50), npre=np.zeros(B, int),
        fin_cnt=np.zeros(B, int), fin_score=np.full((B, k), np.nan, np.float32), fin_len=np.full((B, k), SENT),
        fin_tok=np.full((B, k, Lc), SENT), fin_pos=np.full((B, k, Lc), np.nan, np.float32), fin_anc=np.full((B, k, Lc), SENT))
    st["tok"][:t_step + 1] = rng.integers(4, V, (t_step + 1, R_))
    st["cum"][:t_step + 1] = rng.integers(-80, 1, (t_step + 1, R_)) / 8.0
    st["npre"][:] = rng.integers(0, c0 + 1, B)
    for b in range(B):
        st["anc"][t_step & 1, b * k:(b + 1) * k, :ci + 1] = rng.integers(b * k, (b + 1) * k, (k, ci + 1))
    nl = 1 if t_step == 0 else k
    for b in range(B):
        for l in range(nl):
            r = b * k + l
            if b == 0:
                s, t = _cand_list(rng, V, nc, nc)
            elif b == 1:
                s, t = _cand_list(rng, V, nc, 1 if l else min(2, nc))
            elif b == 2:
                s, t = _cand_list(rng, V, nc, nc, eos_at=0 if l < 2 else None)
            elif b == 3:
                s, t = _cand_list(rng, V, nc, nc, eos_at=0 if l == 0 else None)
            elif b == 4:                         # the merge is list 0: k ignored candidates, </s>, k - 1 others -> one ignored slot survives
                s, t = _cand_list(rng, V, nc, nc if l == 0 else 0)
                if l == 0:
                    s = (-(np.arange(nc) + 1) / 8.0).astype(np.float32)
                    t[k] = EOS
            elif b == 5:
                s, t = _cand_list(rng, V, nc, nc)
            elif b == 6:
                s = np.full(nc, -np.inf, np.float32)
                s[0] = -(l + 3) / 8.0
                t = np.array([EOS] + [n for n in range(V) if n != EOS][:nc - 1])
            else:
                s, t = _cand_list(rng, V, nc, max(nc - 1, 1), eos_at=nc - 1 if nc > 1 else None)
            st["cand_s"][r, :nc], st["cand_t"][r, :nc] = s, t
    if k > 1:
        st["ignore"][2 * k + 1] = 1
        st["ignore"][0 * k + k - 1] = 1
    st["ignore"][4 * k:5 * k] = 1
    st["fin_cnt"][3] = k - 1
    st["fin_cnt"][2] = 1 if k > 2 else 0
    st["done"][5] = 1
    st["max_len"][6] = t_step + st["npre"][6]
    return st, B, Lc, V


FLOATS = ("cum", "cand_s", "fin_score", "fin_pos")


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("c0", [0, 2])
@pytest.mark.parametrize("t_step", [0, 3])
@pytest.mark.parametrize("k", [1, 2, 5, 32])
def test_beam_merge_step(lib, k, t_step, c0, normalize):
    from streamspeech_amd.lib import SSOpBeamState
    st, B, Lc, V = _merge_state(k, t_step, c0, 1000 * k + 10 * t_step + c0)
    d = {n: (df(a) if n in FLOATS else di(a)) for n, a in st.items()}
    x = SSOpBeamState(**{n: d[n].data_ptr() for n in d})
    ok(lib.ss_op_beam_merge(S(), C.byref(x), B, k, Lc, V, t_step, c0, EOS, normalize))
    want = R.beam_merge(st, B, k, Lc, V, t_step, c0, EOS, normalize)
    # the hand-built cases are what they claim to be
    if k > 1:
        assert want["fin_cnt"][2] > st["fin_cnt"][2] and want["fin_cnt"][3] == k and want["done"][3] == 1
        assert want["fin_cnt"][4] == 0 and want["fin_cnt"][0] == 0 and want["fin_cnt"][7] == 0
    assert want["done"][6] == 1 and want["fin_cnt"][6] >= 1 and want["done"][0] == 0
    assert want["fin_cnt"][4] == 0 and want["ignore"][4 * k:5 * k].tolist() == [0] * (k - 1) + [1]
    for n in st:
        try:
            same(d[n], want[n].astype(np.float32) if n in FLOATS else want[n])
        except AssertionError as e:
            raise AssertionError(f"{n}: {e}") from None


# ---- beam search: forced prefix --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [5, 300, 6000])
def test_beam_prefix_score(lib, V):
    rng = np.random.default_rng(V)
    rows = 12
    logits = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    ftok = rng.integers(4, V, rows) if V > 5 else np.full(rows, 4)
    ftok[1], ftok[2], ftok[3], ftok[5], ftok[7], ftok[8] = -1, PAD, UNK, V - 1, -5, 0
    logits[6, V - 1] = np.nan
    for pen in (0.0, 0.5):
        lp = of(rows + G)
        ok(lib.ss_op_beam_prefix_score(S(), P(df(logits)), rows, V, P(di(ftok)), PAD, UNK, pen, P(lp)))
        want = np.concatenate([R.beam_prefix_score(logits, ftok, PAD, UNK, pen), np.full(G, np.nan)])
        lp = host(lp)
        assert np.array_equal(np.isnan(lp), np.isnan(want))                     # ftok < 0 rows and the guard are untouched
        assert np.array_equal(np.isinf(lp), np.isinf(want)) and lp[2] == -np.inf and lp[6] == -np.inf
        fin = np.isfinite(want)
        assert np.max(np.abs(lp[fin] - want[fin])) <= 1e-5


def test_beam_prefix_chain(lib):
    rng = np.random.default_rng(11)
    k = 3
    npre = np.array([0, 1, 4, 0, 17, 2])
    row0 = np.concatenate([[0], np.cumsum(npre)])[:-1] + 1                      # one unused row in front
    Np = int(npre.sum()) + 1
    lp = (-rng.random(Np) * 5).astype(np.float32)
    lp[row0[5]] = -np.inf                                                       # -inf - -inf in the differences: NaN in both
    B = len(npre)
    cum0, pos = of(B * k + G), of(Np + G)
    ok(lib.ss_op_beam_prefix_chain(S(), P(df(lp)), P(di(row0)), P(di(npre)), B, k, P(cum0), P(pos)))
    wc, wp = R.beam_prefix_chain(lp, row0, npre, k, np.full(B * k + G, NAN), np.full(Np + G, NAN))
    same(cum0, wc)
    got, wp = host(pos), np.asarray(wp, np.float32)
    nan = np.isnan(wp)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), wp[~nan].view(np.uint32))
