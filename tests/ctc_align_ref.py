"""CTC forced alignment restated in NumPy float64 (csrc/ctc_align.hip): the forward sum, the max-plus pass with the library's tie rule
(stay beats advance beats skip; the trailing blank beats the last label), the spans and the sequential float32 token sums -- plus the
op cases, the runner and the checks tests/test_ctc_align_cpu.py (ss_ctc_align_host) and tests/test_ctc_align_gpu.py (ss_op_ctc_align)
share.  The bounds come from the suite's per-frame bound (TOL = 2e-5 against the float64 log-softmax of the same float32 logits, the
arithmetic of masked_argmax_lprob_kernel) and float64 state: a path of T frames sums T such values."""
import ctypes as C

import numpy as np

TOL = 2e-5                     # tests/test_ctc_scores_gpu.py: TOL
SENT, G = -7, 5                # sentinel value and guard entries behind every output
RESULT = np.dtype([("score", "<f8"), ("viterbi", "<f8"), ("status", "<i4"), ("n_tokens", "<i4")])


def log_softmax(x, V):
    """float64 log-softmax of the first V columns of float32 rows."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = np.asarray(x)[:, :V].astype(np.float64)
        m = x.max(axis=1, keepdims=True)
        return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def extended(y):
    e = np.zeros(2 * len(y) + 1, np.int64)
    e[1::2] = y
    return e


def align(lp, y):
    """lp [T, V] float64 log-probabilities, labels y -> dict(status, score, viterbi, states, path, first, last)."""
    T, L = lp.shape[0], len(y)
    e = extended(y)
    S = len(e)
    can_skip = np.zeros(S, bool)
    can_skip[3::2] = e[3::2] != e[1:-2:2]
    x = lp[:, e]
    ninf = -np.inf
    a = np.full(S, ninf)
    a[:2] = x[0, :2]
    v = a.copy()
    bp = np.zeros((T, S), np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            for vec, fwd in ((a, True), (v, False)):
                adv = np.concatenate([[ninf], vec[:-1]])
                skip = np.where(can_skip, np.concatenate([[ninf, ninf], vec[:-2]])[:S], ninf)
                if fwd:
                    a = np.logaddexp(np.logaddexp(vec, adv), skip) + x[t]
                else:
                    cand = np.stack([vec, adv, skip])
                    k = np.argmax(np.where(np.isnan(cand), ninf, cand), axis=0)      # the first maximum: stay, advance, skip
                    bp[t] = k
                    v = cand[k, np.arange(S)] + x[t]
    out = {"n_tokens": L, "states": None, "path": None, "first": [-1] * L, "last": [-1] * L}
    if np.isnan(x[:, 0]).any():
        out.update(status=2, score=np.nan, viterbi=np.nan)
        return out
    score = np.logaddexp(a[S - 1], a[S - 2]) if S >= 2 else a[0]
    end = S - 2 if (S >= 2 and v[S - 2] > v[S - 1]) else S - 1
    if not v[end] > ninf:
        out.update(status=1, score=ninf, viterbi=ninf)
        return out
    st = np.zeros(T, np.int64)
    s = int(end)
    for t in range(T - 1, 0, -1):
        st[t] = s
        s -= int(bp[t, s])
    st[0] = s
    first, last = [-1] * L, [-1] * L
    for t in range(T):
        if st[t] & 1:
            j = st[t] >> 1
            if first[j] < 0:
                first[j] = t
            last[j] = t
    out.update(status=0, score=float(score), viterbi=float(v[end]), states=st, path=e[st], first=first, last=last)
    return out


def collapse(path):
    """Drop repeats, then blanks."""
    return [int(v) for i, v in enumerate(path) if v != 0 and (i == 0 or v != path[i - 1])]


def path_score(lp, path):
    return float(lp[np.arange(len(path)), np.asarray(path)].sum())


def f32_run_sums(frame_lp, first, last):
    """The sequential float32 sum of frame_lp[first[j] .. last[j]] in ascending frame order."""
    out = np.zeros(len(first), np.float32)
    for j, (a, b) in enumerate(zip(first, last)):
        acc = np.float32(frame_lp[a])
        for t in range(a + 1, b + 1):
            acc = np.float32(acc + np.float32(frame_lp[t]))
        out[j] = acc
    return out


def brute_force(lp, y):
    """Every V^T labelling: (log of the summed probability of those that collapse to y, the best one's log-probability)."""
    T, V = lp.shape
    tot, best = -np.inf, -np.inf
    for n in range(V ** T):
        path = [(n // V ** t) % V for t in range(T)]
        if collapse(path) == list(y):
            s = path_score(lp, path)
            tot, best = np.logaddexp(tot, s), max(best, s)
    return float(tot), float(best)


# ---- the op cases -----------------------------------------------------------------------------------------------------------------
def labels(rng, L, V, repeats=0, pad=1):
    """L labels in [2, V) \\ {pad}, no two adjacent equal but for `repeats` places."""
    y = []
    while len(y) < L:
        c = int(rng.integers(2, V))
        if c != pad and (not y or c != y[-1]):
            y.append(c)
    for j in rng.choice(np.arange(1, L), repeats, replace=False) if repeats else ():
        y[j] = y[j - 1]
    return y


def logits(seed, T, V, ld=None):
    """Seeded float32 rows * 6; columns past V hold 1e9 (they would swamp every sum if they were read)."""
    x = (np.random.default_rng(seed).standard_normal((T, ld or V)) * 6).astype(np.float32)
    x[:, V:] = 1e9
    return x


def small_cases(V=64, ld=None):
    """(name, logits, labels): the smallest shapes at which each piece can go wrong."""
    r = np.random.default_rng(V)
    a, b = 5, 9
    return [
        ("T1_L0", logits(1, 1, V, ld), []),
        ("T1_L1", logits(2, 1, V, ld), [a]),
        ("T2_L2", logits(3, 2, V, ld), [a, b]),
        ("T2_aa_infeasible", logits(4, 2, V, ld), [a, a]),
        ("T3_aa_one_path", logits(5, 3, V, ld), [a, a]),
        ("T17_L17_no_blank_fits", logits(6, 17, V, ld), labels(r, 17, V)),
        ("T37_L9_repeats", logits(7, 37, V, ld), labels(r, 9, V, repeats=3)),
    ]


def block_cases():
    """S = 2L + 1 around one and two passes of the 256-thread block, at T = 320."""
    r = np.random.default_rng(11)
    return [
        ("L127_V64", logits(20, 320, 64), labels(r, 127, 64, repeats=20)),
        ("L128_V257", logits(21, 320, 257, 260), labels(r, 128, 257, repeats=20)),
        ("L129_V64", logits(22, 320, 64), labels(r, 129, 64, repeats=20)),
        ("L300_V6000", logits(23, 320, 6000), labels(r, 300, 6000, repeats=10)),
    ]


def constructed(T=90, V=64, margin=20.0):
    """Logits that follow a known frame labelling with `margin` over every other column -> (logits, labels, frame labelling)."""
    r = np.random.default_rng(31)
    frames, prev = [], 0
    while len(frames) < T:
        gap = int(r.integers(0, 3))
        frames += [0] * gap
        c = int(r.integers(2, V))
        while gap == 0 and c == prev:                          # no blank between two runs: the labels must differ
            c = int(r.integers(2, V))
        frames += [c] * int(r.integers(1, 4))
        prev = c
    frames = np.array(frames[:T], np.int64)
    x = r.standard_normal((T, V)).astype(np.float32)
    x[np.arange(T), frames] = x.max(axis=1) + np.float32(margin)
    return x, collapse(frames), frames


# ---- the runner -------------------------------------------------------------------------------------------------------------------
def run(lib, cases, V, pad=-1, gpu=False, want_path=True, want_frame=True):
    """cases: [(logits [T, ld] float32, labels)] of one ld -> (rc, records); a record is a dict of the utterance's outputs.  The
    buffers carry G sentinel entries behind the last one, checked here.  gpu: ss_op_ctc_align on device copies, else
    ss_ctc_align_host."""
    B = len(cases)
    T = [c[0].shape[0] for c in cases]
    n = [len(c[1]) for c in cases]
    ld = cases[0][0].shape[1]
    x = np.ascontiguousarray(np.concatenate([c[0] for c in cases], 0), np.float32)
    flat = [int(v) for c in cases for v in c[1]]
    tot, nl = sum(T), len(flat)
    res = np.zeros(B + G, RESULT)
    res["status"] = SENT
    path, first, last = (np.full(k + G, SENT, np.int32) for k in (tot, nl, nl))
    tok, frame = (np.full(k + G, np.nan, np.float32) for k in (nl, tot))
    bufs = [res, path, first, last, tok, frame]
    hT, hy, hn = (C.c_int32 * B)(*T), (C.c_int32 * max(nl, 1))(*(flat or [0])), (C.c_int32 * B)(*n)
    use = [True, want_path, True, True, True, want_frame]
    if gpu:
        import torch
        dx = torch.from_numpy(x).cuda()
        dev = [torch.from_numpy(b.view(np.uint8).copy()).cuda() for b in bufs]
        ptr = [C.c_void_p(d.data_ptr()) if u else None for d, u in zip(dev, use)]
        rc = lib.ss_op_ctc_align(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(dx.data_ptr()), ld, V, pad, B, hT, hy,
                                 hn, *ptr)
        torch.cuda.synchronize()
        bufs = [d.cpu().numpy().view(b.dtype) for d, b in zip(dev, bufs)]
    else:
        ptr = [C.c_void_p(b.ctypes.data) if u else None for b, u in zip(bufs, use)]
        rc = lib.ss_ctc_align_host(C.c_void_p(x.ctypes.data), ld, V, pad, B, hT, hy, hn, *ptr)
    res, path, first, last, tok, frame = bufs
    if rc != 0:                                                # a refusal writes nothing
        assert (res["status"] == SENT).all() and (path == SENT).all() and (first == SENT).all() and (last == SENT).all()
        assert np.isnan(tok).all() and np.isnan(frame).all()
        return rc, None
    assert (res["status"][B:] == SENT).all() and (path[tot:] == SENT).all() and (first[nl:] == SENT).all() and (last[nl:] == SENT).all()
    assert np.isnan(tok[nl:]).all() and np.isnan(frame[tot:]).all(), "wrote behind the last entry"
    if not want_path:
        assert (path == SENT).all()
    out, r0, l0 = [], 0, 0
    for b in range(B):
        out.append({"score": float(res["score"][b]), "viterbi": float(res["viterbi"][b]), "status": int(res["status"][b]),
                    "n_tokens": int(res["n_tokens"][b]), "path": path[r0:r0 + T[b]].copy(), "first": first[l0:l0 + n[b]].copy(),
                    "last": last[l0:l0 + n[b]].copy(), "tok_lprob": tok[l0:l0 + n[b]].copy(), "frame_lprob": frame[r0:r0 + T[b]].copy()})
        r0 += T[b]
        l0 += n[b]
    return rc, out


def same_bits(a, b):
    """memcmp of every output of two records."""
    return (np.array([a["score"], a["viterbi"]]).tobytes() == np.array([b["score"], b["viterbi"]]).tobytes()
            and (a["status"], a["n_tokens"]) == (b["status"], b["n_tokens"])
            and all(a[k].tobytes() == b[k].tobytes() for k in ("path", "first", "last", "tok_lprob", "frame_lprob")))


def check(rec, x, V, y, name=""):
    """One utterance's record against the float64 reference on the same logits -> the reference's answer.  Exact: status,
    feasibility, n_tokens, the validity of the path and its spans, the token sums' bits.  Bounded: see the module comment."""
    T = x.shape[0]
    lp = log_softmax(x, V)
    ref = align(lp, y)
    assert rec["status"] == ref["status"] and rec["n_tokens"] == len(y), (name, rec["status"], ref["status"])
    if ref["status"] != 0:
        want = np.isnan if ref["status"] == 2 else (lambda v: v == -np.inf)
        assert want(rec["score"]) and want(rec["viterbi"]), name
        assert (rec["path"] == -1).all() and (rec["first"] == -1).all() and (rec["last"] == -1).all(), name
        assert np.isnan(rec["tok_lprob"]).all() and np.isnan(rec["frame_lprob"]).all(), name
        print(f"ctc_align {name}: T={T} L={len(y)} status {ref['status']}")
        return ref
    e_score = abs(rec["score"] - ref["score"])
    assert e_score <= T * TOL + 1e-9 * max(1.0, abs(ref["score"])), (name, e_score)
    path = rec["path"]
    assert ((path >= 0) & (path < V)).all() and collapse(path) == list(y), f"{name}: the path does not collapse to the labels"
    mine = path_score(lp, path)
    assert mine >= ref["viterbi"] - 2 * T * TOL, (name, mine, ref["viterbi"])
    e_vit = abs(rec["viterbi"] - mine)
    assert e_vit <= T * TOL, (name, e_vit)
    assert rec["score"] >= rec["viterbi"] - 1e-9
    # the spans are the runs of the path, and the token sums the sequential float32 sums of the kernel's own per-frame values
    runs, t = [], 0
    while t < T:
        if path[t] != 0:
            a = t
            while t + 1 < T and path[t + 1] == path[a]:
                t += 1
            runs.append((a, t))
        t += 1
    assert rec["first"].tolist() == [a for a, _ in runs] and rec["last"].tolist() == [b for _, b in runs], name
    e_frame = np.abs(rec["frame_lprob"].astype(np.float64) - lp[np.arange(T), path]).max()
    assert e_frame < TOL, (name, e_frame)
    want = f32_run_sums(rec["frame_lprob"], rec["first"], rec["last"])
    assert rec["tok_lprob"].tobytes() == want.tobytes(), f"{name}: token sums are not the sequential float32 sums"
    print(f"ctc_align {name}: T={T} L={len(y)} |score - f64| = {e_score:.3e}  |viterbi - path f64| = {e_vit:.3e}  "
          f"best - path = {ref['viterbi'] - mine:.3e}  max |frame lp - f64| = {e_frame:.3e}")
    return ref
