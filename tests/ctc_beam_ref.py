"""CTC prefix beam search restated in Python (csrc/ctc_beam.hpp, ctc_beam.hip): hypotheses keyed by their label tuples, float64 state,
the library's order of a frame's entries -- plus the runner and the comparison rule tests/test_ctc_beam_cpu.py (ss_ctc_beam_host) and
tests/test_ctc_beam_gpu.py (ss_op_ctc_beam) share.

The per-frame values come either from a float64 log-softmax of the float32 logits, or from a given den [T, 2] (the row's max and
log-sum as the library computed them) as the float32 expression (x - max) - logsum, which is then the library's own lp bit for bit:
with it the only differences left are float64 roundings of the log-adds, and the ids must agree unless two totals are nearly tied.
`margin` says how nearly: the smallest gap, over all frames, between the last kept and the first dropped prefix, and between
neighbours of the final n-best (the one behind the last included)."""
import ctypes as C

import numpy as np

from tests.ctc_align_ref import TOL, log_softmax, logits  # noqa: F401  (the suite's per-frame bound; the seeded rows)

SENT, G = -7, 5                # sentinel value and guard entries behind every output
HYP = np.dtype([("score", "<f8"), ("n_tokens", "<i4"), ("status", "<i4")])
NINF = -np.inf


def scaled_logits(seed, T, V, scale, ld=None):
    """tests/ctc_align_ref.py:logits with another scale: seeded float32 rows, columns past V hold 1e9."""
    x = (np.random.default_rng(seed).standard_normal((T, ld or V)) * scale).astype(np.float32)
    x[:, V:] = 1e9
    return x


def frame_values(x, V, pad, unk, den=None):
    """lp [T, V] float64: log_softmax over all V columns, pad and unk then -inf."""
    if den is None:
        lp = log_softmax(x, V)
    else:
        with np.errstate(invalid="ignore"):
            x32 = np.asarray(x, np.float32)[:, :V]
            d = np.asarray(den, np.float32)
            lp = ((x32 - d[:, :1]) - d[:, 1:2]).astype(np.float64)
    for m in (pad, unk):
        if 0 <= m < V:
            lp[:, m] = NINF
    return lp


def candidates(row, V, pad, unk, cand):
    """The `cand` unmasked non-blank columns with the largest float32 logits, a tie to the lower id; -inf and NaN never; -1 fills."""
    row = np.asarray(row[:V], np.float64)
    ok = row > NINF                                            # (False for NaN)
    ok[[m for m in (0, pad, unk) if 0 <= m < V]] = False
    ids = np.nonzero(ok)[0]
    ids = ids[np.lexsort((ids, -row[ids]))][:cand].tolist()
    return ids + [-1] * (cand - len(ids))


def collapsed_argmax(lp):
    """The greedy search's labelling: the arg-max per frame (the first maximum), repeats dropped, then blanks."""
    path = np.argmax(lp, axis=1)
    return tuple(int(v) for i, v in enumerate(path) if v != 0 and (i == 0 or v != path[i - 1]))


def search(x, V, pad, unk, beam, cand, nbest, den=None, slot_identity=False):
    """-> dict(status, hyps [(labels tuple, score)] best first, margin, cand_id [T][cand]).

    slot_identity: the MUTANT without the persistent child lookup -- a prefix is known by a node id, and (parent node, token) ->
    node is looked up among the prefixes of the current beam only, so a string that left the beam and is proposed again is a new
    node and its descendants that stayed are strangers to it."""
    x = np.asarray(x, np.float32)
    T = x.shape[0]
    cid = [candidates(x[t], V, pad, unk, cand) for t in range(T)]
    bad = bool(np.isnan(x[:, :V]).any()) or (den is not None and bool(np.isnan(np.asarray(den)).any()))
    if bad:
        return {"status": 2, "hyps": [], "margin": np.inf, "cand_id": cid}
    lp = frame_values(x, V, pad, unk, den)
    if np.isnan(lp).any():
        return {"status": 2, "hyps": [], "margin": np.inf, "cand_id": cid}
    W = cand + 1
    fresh = [0]
    bm = [((), (), 0.0, NINF)]           # (key, labels, pb, pnb), in rank order; the key IS the labels unless slot_identity
    parent = {(): None}                  # slot_identity: key -> (parent key, token)
    margin = np.inf
    with np.errstate(invalid="ignore"):
        for t in range(T):
            ent, where = [], {}          # [key, labels, pb', pnb', place in the frame's order]
            children = {parent[k]: k for k, _, _, _ in bm if parent.get(k) is not None} if slot_identity else None
            for r, (k, p, pb, pnb) in enumerate(bm):
                tot = np.logaddexp(pb, pnb)
                where[k] = len(ent)
                ent.append([k, p, tot + lp[t, 0], pnb + lp[t, p[-1]] if p else NINF, r * W])
            for r, (k, p, pb, pnb) in enumerate(bm):
                tot = np.logaddexp(pb, pnb)
                for j, c in enumerate(cid[t]):
                    if c < 0:
                        continue
                    term = (pb if (p and c == p[-1]) else tot) + lp[t, c]
                    q = p + (c,)
                    if slot_identity:
                        qk = children.get((k, c))
                        if qk is None:
                            fresh[0] += 1
                            qk = ("node", fresh[0])
                            parent[qk] = (k, c)
                    else:
                        qk = q
                    if qk in where:
                        e = ent[where[qk]]
                        e[3] = np.logaddexp(e[3], term)
                    else:
                        where[qk] = len(ent)
                        ent.append([qk, q, NINF, term, r * W + 1 + j])
            live = [(np.logaddexp(e[2], e[3]), e) for e in ent]
            live = [(tot, e) for tot, e in live if tot > NINF]
            live.sort(key=lambda v: (-v[0], v[1][4]))
            if len(live) > beam:
                margin = min(margin, live[beam - 1][0] - live[beam][0])
            bm = [(e[0], e[1], e[2], e[3]) for _, e in live[:beam]]
    tots = [float(np.logaddexp(pb, pnb)) for _, _, pb, pnb in bm]
    for a, b in zip(tots[:nbest], tots[1:nbest + 1]):
        margin = min(margin, a - b)
    return {"status": 0, "hyps": [(p, s) for (_, p, _, _), s in zip(bm[:nbest], tots)], "margin": float(margin), "cand_id": cid}


def labelling_scores(lp):
    """Every V^T path of lp [T, V] (masked columns -inf): {labelling: log of its summed probability}, those above -inf."""
    T, V = lp.shape
    out = {}
    with np.errstate(invalid="ignore"):
        for n in range(V ** T):
            path = [(n // V ** t) % V for t in range(T)]
            s = float(lp[np.arange(T), path].sum())
            if s > NINF:
                y = tuple(v for i, v in enumerate(path) if v != 0 and (i == 0 or v != path[i - 1]))
                out[y] = float(np.logaddexp(out.get(y, NINF), s))
    return out


# ---- the runner -------------------------------------------------------------------------------------------------------------------
def run(lib, xs, V, pad, unk, beam, cand, nbest, gpu=False, out_stride=None, want_den=True):
    """xs: logits [T, ld] float32 of one ld, one per utterance -> (rc, records); a record is dict(hyps [(labels, score)] of its
    status-0 slots, status [nbest], raw: the bytes of its hypothesis records and of the tokens they own, den [T, 2], cand_id
    [T, cand]).  The buffers carry G sentinel entries behind the last one, checked here, and entries of the token rows past
    n_tokens keep the sentinel.  gpu: ss_op_ctc_beam on device copies, else ss_ctc_beam_host."""
    B = len(xs)
    T = [a.shape[0] for a in xs]
    ld = xs[0].shape[1] if B else V
    x = np.ascontiguousarray(np.concatenate(xs, 0), np.float32) if B else np.zeros((1, ld), np.float32)
    tot = sum(T)
    stride = max(T + [1]) if out_stride is None else out_stride
    nb, nc = max(nbest, 1), max(cand, 1)
    hyp = np.zeros(B * nb + G, HYP)
    hyp["status"] = SENT
    toks = np.full(B * nb * max(stride, 1) + G, SENT, np.int32)
    den = np.full(2 * tot + G, np.float32(SENT), np.float32)
    cid = np.full(tot * nc + G, SENT, np.int32)
    bufs = [hyp, toks, den, cid]
    use = [True, True, want_den, want_den]
    hT = (C.c_int32 * max(B, 1))(*T)
    if gpu:
        import torch
        dx = torch.from_numpy(x).cuda()
        dev = [torch.from_numpy(b.view(np.uint8).copy()).cuda() for b in bufs]
        ptr = [C.c_void_p(d.data_ptr()) if u else None for d, u in zip(dev, use)]
        rc = lib.ss_op_ctc_beam(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(dx.data_ptr()), ld, V, pad, unk, B, hT,
                                beam, cand, nbest, ptr[0], ptr[1], stride, ptr[2], ptr[3])
        torch.cuda.synchronize()
        bufs = [d.cpu().numpy().view(b.dtype) for d, b in zip(dev, bufs)]
    else:
        ptr = [C.c_void_p(b.ctypes.data) if u else None for b, u in zip(bufs, use)]
        rc = lib.ss_ctc_beam_host(C.c_void_p(x.ctypes.data), ld, V, pad, unk, B, hT, beam, cand, nbest, ptr[0], ptr[1], stride, ptr[2],
                                  ptr[3])
    hyp, toks, den, cid = bufs
    if rc != 0:                                                # a refusal writes nothing
        assert (hyp["status"] == SENT).all() and (toks == SENT).all() and (den == SENT).all() and (cid == SENT).all()
        return rc, None
    assert (hyp["status"][B * nbest:] == SENT).all() and (toks[B * nbest * stride:] == SENT).all(), "wrote behind the last entry"
    if want_den:
        assert (den[2 * tot:] == SENT).all() and (cid[tot * cand:] == SENT).all(), "wrote behind the last entry"
    else:
        assert (den == SENT).all() and (cid == SENT).all()
    out, r0 = [], 0
    for b in range(B):
        h = hyp[b * nbest:(b + 1) * nbest]
        rows = toks[b * nbest * stride:(b + 1) * nbest * stride].reshape(nbest, stride)
        hyps = []
        for k in range(nbest):
            n = int(h["n_tokens"][k])
            assert 0 <= n <= T[b] and (rows[k, n:] == SENT).all(), "entries past n_tokens were touched"
            if h["status"][k] == 0:
                hyps.append((tuple(int(v) for v in rows[k, :n]), float(h["score"][k])))
            else:
                assert n == 0 and (np.isnan(h["score"][k]) if h["status"][k] == 2 else h["score"][k] == NINF)
        out.append({"hyps": hyps, "status": h["status"].tolist(), "raw": h.tobytes() + b"".join(rows[k, :int(h["n_tokens"][k])].tobytes() for k in range(nbest)),
                    "den": den[2 * r0:2 * (r0 + T[b])].reshape(-1, 2).copy(), "cand_id": cid[r0 * cand:(r0 + T[b]) * cand].reshape(-1, cand).copy()})
        r0 += T[b]
    return rc, out


def compare(rec, ref, name=""):
    """The issue's rule.  -> True when the case was compared by its sorted scores only (reference margin below 1e-9)."""
    got, want = rec["hyps"], ref["hyps"]
    assert len(got) == len(want), (name, len(got), len(want))
    close = lambda a, b: abs(a - b) <= 1e-9 * max(1.0, abs(b))  # noqa: E731
    if ref["margin"] < 1e-9:
        assert all(close(a, b) for a, b in zip(sorted(s for _, s in got), sorted(s for _, s in want))), name
        return True
    assert [y for y, _ in got] == [y for y, _ in want], (name, got, want)
    assert all(close(a, b) for (_, a), (_, b) in zip(got, want)), (name, got, want)
    return False
