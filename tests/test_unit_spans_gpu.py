"""Unit spans on the GPU (csrc/unit_spans.hip): the kernel through ss_op_unit_spans and the production entry ss_batch_unit_spans
against tests/spans_ref.py on the cases the host twin passes in tests/test_unit_spans_cpu.py.  Equality is exact (integers).  Every
output buffer is filled with a sentinel first: the kernel writes every span of its rows and nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import spans_ref as R

pytestmark = pytest.mark.gpu
BLANK, PAD, EOS, BOS = R.BLANK, R.PAD, R.EOS, R.BOS
SENT = -777
GUARD = 64            # sentinel int32s in front of and behind every output


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _p(t):
    return C.c_void_p(t.data_ptr())


def run_op(lib, up, rows, K=None, dur=None):
    """-> (rc, spans [sum n, 4], counted [B]) with the guards around both outputs checked."""
    raw, K0, d0, u0, dur0 = R.pack_rows(rows)
    K = K0 if K is None else K
    dur = dur0 if dur is None else dur
    n = [r["raw"].size // up for r in rows]
    N, B = sum(n), len(rows)
    spans = torch.full((GUARD + 4 * N + GUARD,), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((GUARD + B + GUARD,), SENT, dtype=torch.int32, device="cuda")
    d_raw, d_dur = _dev(raw), _dev(dur)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.ss_op_unit_spans(s, B, _p(d_raw), _i32(n), _i32(K), _i32(d0), _i32(u0), _p(d_dur), up, BLANK, PAD, BOS, EOS,
                              _p(spans[GUARD:]), _p(cnt[GUARD:]))
    torch.cuda.synchronize()
    hs, hc = spans.cpu().numpy(), cnt.cpu().numpy()
    for h, m in ((hs, 4 * N), (hc, B)):
        assert (h[:GUARD] == SENT).all() and (h[GUARD + m:] == SENT).all(), "a store outside the call's rows"
    return rc, hs[GUARD: GUARD + 4 * N].reshape(N, 4), hc[GUARD: GUARD + B]


def check_rows(up, rows, spans, counted, skip=()):
    off = 0
    for b, r in enumerate(rows):
        nb = r["raw"].size // up
        want, k = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"], r["d0"], r["u0"])
        assert counted[b] == k == r["K"], b
        if b not in skip:
            assert (spans[off: off + nb] == want).all(), b
            total = int(np.asarray(r["dur"])[r["u0"] - r["d0"]: r["K"] - r["d0"]].sum()) if r["K"] > r["u0"] else 0
            R.check_tiling(spans[off: off + nb], r["u0"], r["K"], total)
        off += nb


@pytest.mark.parametrize("name", sorted(R.op_cases()))
def test_op_cases(lib, name):
    """n = 1 all blank; one run over frames 24 | 25; the same with a blank between; bos / eos inside and last; u0 inside a state with
    d0 < u0; u0 = K; n = [1, 65, 3]; a row of n = 1030 (past one wave, past one 1024-thread pass); up = 1 and up = 3."""
    up, rows = R.op_cases()[name]
    rc, spans, counted = run_op(lib, up, rows)
    assert rc == 0
    check_rows(up, rows, spans, counted)


def test_op_each_row_alone_is_the_row_in_the_pack(lib):
    up, rows = R.op_cases()["row_of_1030"]
    _, pack, _ = run_op(lib, up, rows)
    off = 0
    for r in rows:
        nb = r["raw"].size // up
        _, alone, _ = run_op(lib, up, [r])
        assert (alone == pack[off: off + nb]).all()
        off += nb


def test_op_wrong_count_is_reported_for_its_row_only(lib):
    up, rows = R.op_cases()["ragged_1_65_3"]
    _, K, _, _, dur = R.pack_rows(rows)
    for delta in (2, -1):
        wrong = list(K)
        wrong[1] += delta
        dur2 = np.zeros(sum(wrong) + 1, dtype=np.int32)
        o = o2 = 0
        for k, k2 in zip(K, wrong):
            dur2[o2: o2 + min(k, k2)] = dur[o: o + min(k, k2)]
            o, o2 = o + k, o2 + k2
        rc, spans, counted = run_op(lib, up, rows, K=wrong, dur=dur2)
        assert rc == 0 and counted.tolist() == K and counted[1] != wrong[1]
        check_rows(up, rows, spans, counted, skip=(1,))


def test_op_refusals_launch_and_write_nothing(lib):
    from streamspeech_amd.lib import SS_ERR_ARG
    up, rows = R.op_cases()["ragged_1_65_3"]
    raw, K, d0, u0, dur = R.pack_rows(rows)
    n = [r["raw"].size // up for r in rows]
    d_raw, d_dur = _dev(raw), _dev(dur)
    spans = torch.full((4 * sum(n),), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((3,), SENT, dtype=torch.int32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(B=3, raw=d_raw, n=n, K=K, d0=d0, u0=u0, dur=d_dur, up=up, spans=spans, cnt=cnt):
        return lib.ss_op_unit_spans(s, B, None if raw is None else _p(raw), _i32(n), _i32(K), _i32(d0), _i32(u0),
                                    None if dur is None else _p(dur), up, BLANK, PAD, BOS, EOS,
                                    None if spans is None else _p(spans), None if cnt is None else _p(cnt))

    for kw in (dict(B=0), dict(raw=None), dict(dur=None), dict(spans=None), dict(cnt=None), dict(n=[1, 0, 3]), dict(d0=[0, 5, 0], u0=[0, 4, 0]),
               dict(u0=[0, K[1] + 1, 0]), dict(K=[K[0], -1, K[2]]), dict(up=0), dict(spans=spans[1:])):
        assert call(**kw) == SS_ERR_ARG, kw
    torch.cuda.synchronize()
    assert (spans == SENT).all() and (cnt == SENT).all()


# ---- the production entry point ------------------------------------------------------------------------------------------------------
def _model_rows(cfg, seed, ns, windows):
    """Rows over the model's own ids (blank = unit_vocab - 1, pad, bos 0, eos) at its ctc_upsample."""
    rng = np.random.default_rng(seed)
    blank, up = cfg.unit_vocab - 1, cfg.ctc_upsample
    rows = []
    for n, win in zip(ns, windows):
        raw = R.random_row(rng, n, up, blank, cfg.pad, cfg.eos, 0.55)
        K = int(R.unit_mask(raw, blank, cfg.pad, BOS, cfg.eos).sum())
        d0, u0 = win(K)
        rows.append({"raw": raw, "d0": d0, "u0": u0, "dur": R.random_dur(rng, K - d0), "K": K})
    return rows


def test_batch_entry_device_and_host_durations_agree(hip_model):
    cfg = hip_model.cfg
    up, blank = cfg.ctc_upsample, cfg.unit_vocab - 1
    rows = _model_rows(cfg, 11, (1, 65, 3, 1030 if up == 25 else 2048 // up + 7),
                       (lambda K: (0, 0), lambda K: (K // 5, K // 3), lambda K: (0, min(1, K)), lambda K: (K // 7, K // 2)))
    raw, K, d0, u0, dur = R.pack_rows(rows)
    n = [r["raw"].size // up for r in rows]
    d_raw = _dev(raw)
    host = hip_model.batch_unit_spans(d_raw, n, K, [r["dur"] for r in rows], d0, u0)
    dev = hip_model.batch_unit_spans(d_raw, n, K, _dev(dur), d0, u0)       # the same layout on the device
    for r, h, d in zip(rows, host, dev):
        want, _ = R.unit_spans(r["raw"], up, blank, cfg.pad, BOS, cfg.eos, r["dur"], r["d0"], r["u0"])
        assert h.dtype == np.int32 and h.shape == want.shape
        assert (h == want).all() and (d == want).all()
    # offline's form: d0 = u0 = 0, the durations as batch_forward leaves them
    zero = [dict(r, d0=0, u0=0, dur=R.random_dur(np.random.default_rng(3), r["K"])) for r in rows]
    raw, K, _, _, dur = R.pack_rows(zero)
    for r, got in zip(zero, hip_model.batch_unit_spans(d_raw, n, K, _dev(dur))):
        assert (got == R.unit_spans(r["raw"], up, blank, cfg.pad, BOS, cfg.eos, r["dur"])[0]).all()


def test_batch_entry_wrong_count_names_the_row_and_refusals(hip_model):
    from streamspeech_amd.lib import SS_ERR_ARG, StreamSpeechHipError
    cfg = hip_model.cfg
    up = cfg.ctc_upsample
    rows = _model_rows(cfg, 12, (2, 9, 4), (lambda K: (0, 0),) * 3)
    raw, K, d0, u0, dur = R.pack_rows(rows)
    n = [r["raw"].size // up for r in rows]
    d_raw = _dev(raw)
    wrong = [K[0], K[1] + 1, K[2]]
    with pytest.raises(StreamSpeechHipError, match="row 1 holds %d units" % K[1]):
        hip_model.batch_unit_spans(d_raw, n, wrong, [list(r["dur"]) + [1] for r in rows])
    for kw in (dict(n=[2, 0, 4]), dict(d0=[0, 2, 0], u0=[0, 1, 0]), dict(u0=[0, K[1] + 1, 0])):
        a = dict(n=n, d0=d0, u0=u0)
        a.update(kw)
        with pytest.raises(StreamSpeechHipError) as e:
            hip_model.batch_unit_spans(d_raw, a["n"], K, [r["dur"] for r in rows], a["d0"], a["u0"])
        assert e.value.code == SS_ERR_ARG
    # both or neither duration pointer
    lib = hip_model.lib
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = np.full((sum(n), 4), SENT, dtype=np.int32)
    cnt = np.full(3, SENT, dtype=np.int32)
    d_dur = _dev(dur)
    for dd, hd in ((None, None), (_p(d_dur), dur.ctypes.data_as(C.c_void_p))):
        rc = lib.ss_batch_unit_spans(hip_model.h, s, 3, _p(d_raw), _i32(n), _i32(K), _i32(d0), _i32(u0), dd, hd,
                                     out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p))
        assert rc == SS_ERR_ARG and (out == SENT).all() and (cnt == SENT).all()
