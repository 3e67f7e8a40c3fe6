"""Streaming session pool (csrc/stream_pool.hip, ss_stream_pool_* / ss_encoder_stream_forward_batch): one batched encoder step for many
concurrent streams.  Per slot it must behave exactly like ss_encoder_stream_forward on a context of its own; a session's bits must not
depend on what else is in the step (the streaming analogue of test_pack_invariance_gpu.py); the CTC heads keep the arg-max of final
rows; the pool's memory is booked in its scratch set; a step's launch count does not grow with the number of sessions."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_ROWS = 160


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import synth
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    cfg = ModelConfig()
    return HipModel(synth.make_model_state_dict(0, cfg), cfg)


def _fbank(seed, T, device):
    from streamspeech_amd import synth
    return torch.from_numpy(synth.synth_fbank(seed, T)).to(device)


# 12 sessions: chunks of 8 / 16 / 24 rows (320 / 640 / 960 ms), 32 fbank frames (320 ms) per step, different start offsets, late
# joins and skipped steps; session 5 has an unsettled tail frame (a resampling front-end).
def _schedule(n_sess=12, n_steps=9):
    sess = []
    for i in range(n_sess):
        ch = (8, 16, 24)[i % 3]
        sess.append({"seed": 100 + i, "chunk": ch, "join": i % 4, "first": 40 + 7 * i, "skip": (3 + i) % 5, "tail": 1 if i == 5 else 0})
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


def _run_pool(model, sess, steps, fb, order="fwd", alone=False):
    pool = model.stream_pool(len(sess), MAX_ROWS)
    for i, s in enumerate(sess):
        pool.set_tail(i, s["tail"])
    res = {i: [] for i in range(len(sess))}
    for row in steps:
        row = list(reversed(row)) if order == "rev" else list(row)
        groups = [[x] for x in row] if alone else [row]
        for g in groups:
            slots = [i for i, _ in g]
            fbs = [fb[i][:T].contiguous() for i, T in g]
            ch = [sess[i]["chunk"] for i in slots]
            _, views, nf, nc = pool.forward(slots, fbs, ch, ch)
            for k, i in enumerate(slots):
                res[i].append((g[k][1], views[k].clone(), nf[k], nc[k]))
    return res


@pytest.fixture(scope="module")
def sched(model):
    sess, steps = _schedule()
    fb = [_fbank(s["seed"], s["first"] + 32 * 9, model.device) for s in sess]
    return sess, steps, fb


def test_session_invariance_bitwise(model, sched):
    sess, steps, fb = sched
    a = _run_pool(model, sess, steps, fb)
    b = _run_pool(model, sess, steps, fb, order="rev")
    c = _run_pool(model, sess, steps, fb, alone=True)
    for i in a:
        assert len(a[i]) == len(b[i]) == len(c[i]) > 0
        for (Ta, xa, fa, na), (Tb, xb, fb_, nb), (Tc, xc, fc, ncc) in zip(a[i], b[i], c[i]):
            assert Ta == Tb == Tc
            assert torch.equal(xa, xb) and torch.equal(xa, xc), (i, Ta)
            assert fa == fb_ == fc and na == nb == ncc, (i, Ta)


def test_against_single_session_path(model, sched):
    sess, steps, fb = sched
    got = _run_pool(model, sess, steps, fb)
    ctx = model.new_context()
    worst = 0.0
    for i, s in enumerate(sess):
        ctx.encoder_stream_reset()
        ctx.encoder_stream_set_tail(s["tail"])
        prev_nf = 0
        for T, x, nf, nc in got[i]:
            ref = ctx.encoder_stream_forward(fb[i][:T].contiguous(), s["chunk"], s["chunk"])
            assert ref.shape == x.shape
            assert ctx.stream_stats == (nf, nc), (i, T)
            worst = max(worst, (x - ref).abs().max().item())
            full = model.encoder_forward(fb[i][:T].contiguous(), s["chunk"], s["chunk"])
            assert (x - full).abs().max().item() < 5e-5, (i, T)
            assert nf >= prev_nf
            prev_nf = nf
            for hd in (0, 1):                        # both heads at every step
                assert ctx.ctc_greedy(hd, ref)[0] == ctx.ctc_greedy(hd, x)[0], (i, T, hd)
    assert worst < 2e-5, worst
    ctx.encoder_stream_reset()


def test_ctc_heads_and_their_cache(model, sched):
    sess, steps, fb = sched
    pool = model.stream_pool(len(sess), MAX_ROWS)
    for row in steps:
        slots = [i for i, _ in row]
        ch = [sess[i]["chunk"] for i in slots]
        out, views, nf, nc = pool.forward(slots, [fb[i][:T].contiguous() for i, T in row], ch, ch)
        T2 = [v.shape[0] for v in views]
        for hd in (0, 1):
            got = pool.ctc(hd, return_raw=True)
            ref = model.batch_ctc_greedy(hd, out, T2, return_raw=True)
            assert got == ref
    # a step that follows an all-final step runs no head rows for that session: T = 256 fbank frames at 8-row chunks is all final
    p2 = model.stream_pool(2, MAX_ROWS)
    x256 = _fbank(7, 256, model.device)
    _, v, nf, nc = p2.forward([0], [x256], [8], [8])
    assert nf == [v[0].shape[0]] == [64] and nc == [64]
    first = [p2.ctc(hd, return_raw=True) for hd in (0, 1)]
    l0, r0 = p2.stats()
    assert r0 == 2 * 64
    _, v2, nf, nc = p2.forward([0], [x256], [8], [8])
    assert nc == [0] and torch.equal(v2[0], v[0])
    again = [p2.ctc(hd, return_raw=True) for hd in (0, 1)]
    assert again == first
    assert p2.stats()[1] == r0                       # no head rows at all
    y = _fbank(8, 100, model.device)                 # with another session in the step: only that session's rows
    _, v3, nf3, nc3 = p2.forward([1, 0], [y, x256], [8, 8], [8, 8])
    for hd in (0, 1):
        p2.ctc(hd)
    assert p2.stats()[1] == r0 + 2 * v3[0].shape[0]


def test_lifecycle_and_books(model):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    sc = Scratch(model.device)
    ctx = model.new_context(sc)
    b0 = sc.bytes()
    pool = ctx.stream_pool(4, 96)
    per_row = model.cfg.enc_layers * 4 * model.cfg.enc_dim * 4 + model.cfg.enc_dim * 4 + 8
    assert sc.bytes() - b0 >= 4 * 96 * per_row
    booked, held = sc.audit()
    assert booked == held
    xs = [_fbank(20 + i, 300, model.device) for i in range(3)]
    step = lambda Ts, chs=(16, 16, 16): pool.forward([0, 1, 2], [x[:T].contiguous() for x, T in zip(xs, Ts)], list(chs), list(chs))  # noqa: E731
    _, v, nf, nc = step([100, 120, 140])
    assert nc == [v[k].shape[0] for k in range(3)]
    sc.trim(0)                                     # the pool's state is a fixed piece: trim keeps it
    assert sc.bytes() >= 4 * 96 * per_row
    assert sc.audit()[0] == sc.audit()[1]
    # reference: the same sessions driven without interruption on a pool of their own
    ref = model.stream_pool(4, 96)
    ref.forward([0, 1, 2], [x[:T].contiguous() for x, T in zip(xs, [100, 120, 140])], [16] * 3, [16] * 3)
    _, rv, rnf, rnc = ref.forward([0, 1, 2], [x[:T].contiguous() for x, T in zip(xs, [132, 152, 172])], [16] * 3, [16] * 3)
    # a pool over the cap fails cleanly and leaves the set as it was
    sc.set_cap(sc.bytes() + 1024)
    before = sc.bytes()
    with pytest.raises(L.StreamSpeechHipError) as e:
        ctx.stream_pool(64, 96)
    assert e.value.code == L.SS_ERR_SCRATCH_CAP and sc.bytes() == before and sc.audit()[0] == sc.audit()[1]
    sc.set_cap(0)
    # a step whose session passes max_rows is refused whole, on the host and by the C ABI, and no slot changes
    big = _fbank(22, 400, model.device)             # 99 output rows > 96
    with pytest.raises(ValueError):
        pool.forward([0, 1, 2], [xs[0][:132].contiguous(), xs[1][:152].contiguous(), big], [16] * 3, [16] * 3)
    n = 3
    rc = model.lib.ss_encoder_stream_forward_batch(
        ctx.h, C.c_void_p(torch.cuda.current_stream().cuda_stream), pool.h, n, (C.c_int32 * n)(0, 1, 2),
        (C.c_void_p * n)(xs[0].data_ptr(), xs[1].data_ptr(), big.data_ptr()), (C.c_int32 * n)(132, 152, 400),
        (C.c_int32 * n)(16, 16, 16), (C.c_int32 * n)(16, 16, 16), C.c_void_p(torch.empty(1, device=model.device).data_ptr()), None, None)
    assert rc == L.SS_ERR_ARG
    with pytest.raises(ValueError):
        pool.forward([0, 0], [xs[0][:100].contiguous()] * 2, [16, 16], [16, 16])
    _, v, nf, nc = step([132, 152, 172])           # ... and the step after matches an uninterrupted run
    for k in range(3):
        assert torch.equal(v[k], rv[k])
    assert nf == rnf and nc == rnc
    # reset: a fresh stream; a chunk change does the same implicitly
    pool.reset(1)
    _, v2, nf2, nc2 = step([132, 152, 172])
    assert nc2[1] == v2[1].shape[0]
    assert nc2[0] == v2[0].shape[0] - nf[0] < v2[0].shape[0] and nc2[2] == v2[2].shape[0] - nf[2]
    _, v3, nf3, nc3 = step([132, 152, 172], chs=(16, 8, 16))
    assert nc3[1] == v3[1].shape[0] and nc3[0] == v3[0].shape[0] - nf2[0] and nc3[2] == v3[2].shape[0] - nf2[2]


def _gemm_dispatch(lib):
    """Launches per GEMM-family shape (N, taps, Cin, operands) so far, from the library's own dispatch census.  Summed over kernel
    classes: the pack-invariant routes may pick another kernel of the same bits at another row count (CANON_SEQ, gemm.hpp), but
    not launch more kernels."""
    n = lib.ss_prof_shape_dump(None, 0)
    buf = C.create_string_buffer(n)
    lib.ss_prof_shape_dump(buf, n)
    out = {}
    for line in buf.value.decode().splitlines()[1:]:
        f = [int(v) for v in line.split()[:6]]
        out[tuple(f[1:5])] = out.get(tuple(f[1:5]), 0) + f[5]
    return out


def test_launch_count_does_not_grow_with_sessions(model):
    """Real kernel launches: every GEMM-family launch of a step, by shape, from the library's dispatch census (a launcher that issued
    more kernels at another row count shows up here), and the step's total."""
    lib = model.lib
    counts = (1, 16, 64)
    pool = model.stream_pool(max(counts), 64)
    x = [_fbank(300 + i, 200, model.device) for i in range(max(counts))]
    lib.ss_prof_shape_log(1)
    try:
        per, total = [], []
        for n in counts:
            for s in range(n):
                pool.reset(s)
            T = [96 + (s % 5) * 16 for s in range(n)]
            ch = [(8, 16, 24)[s % 3] for s in range(n)]
            torch.cuda.synchronize()
            d0, l0 = _gemm_dispatch(lib), pool.stats()[0]
            pool.forward(list(range(n)), [x[s][:T[s]].contiguous() for s in range(n)], ch, ch)
            pool.ctc_both()
            d1, l1 = _gemm_dispatch(lib), pool.stats()[0]
            per.append({k: v - d0.get(k, 0) for k, v in d1.items() if v != d0.get(k, 0)})
            total.append(l1 - l0)
    finally:
        lib.ss_prof_shape_log(0)
    assert per[0] == per[1] == per[2], per
    assert len(set(total)) == 1, total
    assert total[0] < 14 * model.cfg.enc_layers, total
