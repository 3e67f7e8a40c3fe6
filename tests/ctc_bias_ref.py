"""Hotword biasing of the CTC prefix beam search (csrc/ctc_bias.hpp, the bias forms of csrc/ctc_beam.hpp) restated in Python from
the definition: the phrase automaton with its state found as the longest suffix that is a node, by search, without fail links
(Naive); the closed form of a finished string's bias, which knows nothing of states (closed_form); the search of
tests/ctc_beam_lm_ref.py with the bias term, with a model or without (search); and the runner and the comparison rule that
tests/test_ctc_beam_bias_cpu.py (ss_ctc_beam_bias_host) and tests/test_ctc_beam_bias_gpu.py (ss_op_ctc_beam_bias) share."""
import ctypes as C

import numpy as np

from tests.ctc_beam_ref import G, NINF, SENT, candidates, frame_values

BHYP = np.dtype([("score", "<f8"), ("ctc_score", "<f8"), ("lm_score", "<f8"), ("bias_score", "<f8"), ("n_tokens", "<i4"),
                 ("status", "<i4")])
MAX_LEN = 32


def occurs_inside(phrases):
    """True when a phrase occurs inside another one at a position other than its start (the set is then refused)."""
    ps = [tuple(p) for p in phrases]
    for p in ps:
        for q in ps:
            if p is not q and any(q[i:i + len(p)] == p for i in range(1, len(q) - len(p) + 1)):
                return True
    return False


def admissible(phrases, V=None, pad=-1, unk=-1):
    ps = [tuple(p) for p in phrases]
    if any(len(p) < 1 or len(p) > MAX_LEN for p in ps) or len(set(ps)) != len(ps) or occurs_inside(ps):
        return False
    return all(t > 0 and t not in (pad, unk) and (V is None or t < V) for p in ps for t in p)


def random_set(rng, labels, n_phrases, max_len, tries=200):
    """An admissible set of up to n_phrases phrases over `labels` with float32 boosts in [-1, 3), by rejection: a phrase that
    would break a rule is drawn again.  Prefix nesting is sought: every third phrase extends an earlier one."""
    ps = []
    for _ in range(tries):
        if len(ps) >= n_phrases:
            break
        if ps and len(ps) % 3 == 2:
            base = ps[int(rng.integers(len(ps)))]
            p = base + tuple(int(rng.choice(labels)) for _ in range(int(rng.integers(1, 3))))
        else:
            p = tuple(int(rng.choice(labels)) for _ in range(int(rng.integers(1, max_len + 1))))
        if len(p) <= MAX_LEN and admissible(ps + [p]):
            ps.append(p)
    boosts = [float(np.float32(rng.uniform(-1.0, 3.0))) for _ in ps]
    return [list(p) for p in ps], boosts


class Naive:
    """The automaton by definition: nodes are the distinct phrase prefixes (tuples), a node's boost the largest of the phrases
    through it, held summed root-down in float64, floor the held of the deepest phrase end on the path; the state of a string is
    its longest suffix that is a node, found by trying the suffixes, the longest first."""

    def __init__(self, phrases, boosts):
        self.phrases = [tuple(p) for p in phrases]
        self.ends = set(self.phrases)
        boost = {}
        for p, b in zip(self.phrases, boosts):
            for k in range(1, len(p) + 1):
                boost[p[:k]] = max(boost.get(p[:k], -np.inf), float(np.float32(b)))
        self.held, self.floor = {(): 0.0}, {(): 0.0}
        for n in sorted(boost, key=len):
            self.held[n] = self.held[n[:-1]] + boost[n]
            self.floor[n] = self.held[n] if n in self.ends else self.floor[n[:-1]]

    def state(self, y):
        y = tuple(y)
        for k in range(min(len(y), MAX_LEN), -1, -1):
            if y[len(y) - k:] in self.held:
                return y[len(y) - k:]
        raise AssertionError

    def step(self, s, c):
        """state s (a node) --c--> (delta, new state)."""
        n = self.state(s + (c,))
        d = self.held[n] - self.held[s]
        if n != s + (c,):
            d = d + self.floor[s]
        return d, n

    def open(self, s):
        return self.held[s] - self.floor[s]

    def walk(self, y, finish=True):
        """-> (deltas, states, sum): the state after token j is the longest suffix of y[:j + 1] that is a node -- of the STRING, not
        of the state before it plus the token."""
        s, ds, ss, acc = (), [], [], 0.0
        for j, c in enumerate(y):
            d, n = self.step(s, int(c))
            assert n == self.state(tuple(int(v) for v in y[:j + 1]))
            ds.append(d); ss.append(n); acc += d
            s = n
        return ds, ss, acc - self.open(s) if finish else acc


def closed_form(phrases, boosts, y):
    """The finished bias of y without any state: the sum of held[p] over the occurrences (p, i) of phrases in y that are not a
    proper prefix of another occurrence starting at the same i."""
    a = Naive(phrases, boosts)
    y = tuple(int(v) for v in y)
    total = 0.0
    for i in range(len(y)):
        here = [p for p in a.ends if y[i:i + len(p)] == p]
        if here:
            total += a.held[max(here, key=len)]                # occurrences at one i are prefixes of each other: the longest
    return total


def search(x, V, pad, unk, beam, cand, nbest, bias, scale, finish=True, lm=None, lm_weight=0.0, word_score=0.0, eos_term=True, den=None):
    """tests/ctc_beam_lm_ref.py:search with the bias term.  bias: a Naive; lm: a tests.ngram_ref.Ref or None.  -> dict(status, hyps
    [(labels, fin, ctc, lm_sum, bias)] best first, margin, cand_id); margin as there, on the fused scores."""
    x = np.asarray(x, np.float32)
    T = x.shape[0]
    cid = [candidates(x[t], V, pad, unk, cand) for t in range(T)]
    bad = bool(np.isnan(x[:, :V]).any()) or (den is not None and bool(np.isnan(np.asarray(den)).any()))
    if bad:
        return {"status": 2, "hyps": [], "margin": np.inf, "cand_id": cid}
    lp = frame_values(x, V, pad, unk, den)
    W = cand + 1
    info = {(): (lm.start() if lm else None, 0.0, 0.0, (), 0.0)}     # labels -> (history, lm_sum, bonus, bias state, bias_sum)

    def fields(q):
        if q not in info:
            hist, s, b, bs, bsum = fields(q[:-1])
            b1 = b
            if lm:
                v, hist = lm.lp(hist, q[-1])
                s = s + v
                b1 = b + ((lm_weight * v) + word_score)
            d, bs2 = bias.step(bs, q[-1])
            info[q] = (hist, s, b1 + (scale * d), bs2, bsum + d)
        return info[q]

    bm = [((), 0.0, NINF)]
    margin = np.inf
    with np.errstate(invalid="ignore"):
        for t in range(T):
            ent, where = [], {}                  # [labels, pb', pnb', place]
            for r, (p, pb, pnb) in enumerate(bm):
                tot = np.logaddexp(pb, pnb)
                where[p] = len(ent)
                ent.append([p, tot + lp[t, 0], pnb + lp[t, p[-1]] if p else NINF, r * W])
            for r, (p, pb, pnb) in enumerate(bm):
                tot = np.logaddexp(pb, pnb)
                for j, c in enumerate(cid[t]):
                    if c < 0:
                        continue
                    term = (pb if (p and c == p[-1]) else tot) + lp[t, c]
                    q = p + (c,)
                    if q in where:
                        e = ent[where[q]]
                        e[2] = np.logaddexp(e[2], term)
                    else:
                        where[q] = len(ent)
                        ent.append([q, NINF, term, r * W + 1 + j])
            live = [(np.logaddexp(e[1], e[2]), e) for e in ent]
            live = [(tot + fields(e[0])[2], e) for tot, e in live if tot > NINF]
            live.sort(key=lambda v: (-v[0], v[1][3]))
            if len(live) > beam:
                margin = min(margin, live[beam - 1][0] - live[beam][0])
            bm = [(e[0], e[1], e[2]) for _, e in live[:beam]]
    fin = []
    for r, (p, pb, pnb) in enumerate(bm):
        tot = float(np.logaddexp(pb, pnb))
        hist, s, b, bs, bsum = fields(p)
        f = tot + b
        if lm and eos_term:
            v, _ = lm.lp(hist, lm.eos)
            f, s = f + (lm_weight * v), s + v
        if finish:
            o = bias.open(bs)
            f, bsum = f - (scale * o), bsum - o
        fin.append((p, f, tot, s, bsum, r))
    fin.sort(key=lambda v: (-v[1], v[5]))
    for a, b in zip(fin[:nbest], fin[1:nbest + 1]):
        margin = min(margin, a[1] - b[1])
    return {"status": 0, "hyps": [h[:5] for h in fin[:nbest]], "margin": float(margin), "cand_id": cid}


def run(lib, xs, V, pad, unk, beam, cand, nbest, bias, scale, finish=True, lm=None, lm_weight=0.0, word_score=0.0, eos_term=True,
        gpu=False, out_stride=None, want_den=True, bias_opts=True, lm_opts=None):
    """tests/ctc_beam_lm_ref.py:run for the bias entry points: bias and lm are the library's handles (c_void_p, or None), ->
    (rc, records); a record is dict(hyps [(labels, score, ctc_score, lm_score, bias_score)], status, raw, den, cand_id).  lm_opts:
    None gives the model its options exactly when there is one; True / False force them.  Guards and sentinels as there."""
    from streamspeech_amd.lib import SSCtcBiasOpts, SSCtcLmOpts
    B = len(xs)
    T = [a.shape[0] for a in xs]
    ld = xs[0].shape[1] if B else V
    x = np.ascontiguousarray(np.concatenate(xs, 0), np.float32) if B else np.zeros((1, ld), np.float32)
    tot = sum(T)
    stride = max(T + [1]) if out_stride is None else out_stride
    nb, nc = max(nbest, 1), max(cand, 1)
    hyp = np.zeros(B * nb + G, BHYP)
    hyp["status"] = SENT
    toks = np.full(B * nb * max(stride, 1) + G, SENT, np.int32)
    den = np.full(2 * tot + G, np.float32(SENT), np.float32)
    cid = np.full(tot * nc + G, SENT, np.int32)
    bufs = [hyp, toks, den, cid]
    use = [True, True, want_den, want_den]
    hT = (C.c_int32 * max(B, 1))(*T)
    with_lo = (lm is not None) if lm_opts is None else lm_opts
    lo = C.byref(SSCtcLmOpts(lm_weight, word_score, int(eos_term))) if with_lo else None
    bo = C.byref(SSCtcBiasOpts(scale, int(finish), 0)) if bias_opts else None
    if gpu:
        import torch
        dx = torch.from_numpy(x).cuda()
        dev = [torch.from_numpy(b.view(np.uint8).copy()).cuda() for b in bufs]
        ptr = [C.c_void_p(d.data_ptr()) if u else None for d, u in zip(dev, use)]
        rc = lib.ss_op_ctc_beam_bias(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(dx.data_ptr()), ld, V, pad, unk, B,
                                     hT, beam, cand, nbest, ptr[0], ptr[1], stride, ptr[2], ptr[3], lm, lo, bias, bo)
        torch.cuda.synchronize()
        bufs = [d.cpu().numpy().view(b.dtype) for d, b in zip(dev, bufs)]
    else:
        ptr = [C.c_void_p(b.ctypes.data) if u else None for b, u in zip(bufs, use)]
        rc = lib.ss_ctc_beam_bias_host(C.c_void_p(x.ctypes.data), ld, V, pad, unk, B, hT, beam, cand, nbest, ptr[0], ptr[1], stride,
                                       ptr[2], ptr[3], lm, lo, bias, bo)
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
                hyps.append((tuple(int(v) for v in rows[k, :n]), float(h["score"][k]), float(h["ctc_score"][k]), float(h["lm_score"][k]),
                             float(h["bias_score"][k])))
            else:
                s = h["score"][k], h["ctc_score"][k]
                assert n == 0 and h["lm_score"][k] == 0 and h["bias_score"][k] == 0
                assert np.isnan(s).all() if h["status"][k] == 2 else (np.asarray(s) == NINF).all()
        out.append({"hyps": hyps, "status": h["status"].tolist(),
                    "raw": h.tobytes() + b"".join(rows[k, :int(h["n_tokens"][k])].tobytes() for k in range(nbest)),
                    "den": den[2 * r0:2 * (r0 + T[b])].reshape(-1, 2).copy(), "cand_id": cid[r0 * cand:(r0 + T[b]) * cand].reshape(-1, cand).copy()})
        r0 += T[b]
    return rc, out


def compare(rec, ref, name=""):
    """tests/ctc_beam_lm_ref.py:compare with the bias score: ids equal and score / ctc_score / lm_score / bias_score within
    1e-9 * max(1, |.|) -> False; a case whose reference margin is below 1e-9 compares its sorted scores only -> True."""
    got, want = rec["hyps"], ref["hyps"]
    assert len(got) == len(want), (name, len(got), len(want))
    close = lambda a, b: abs(a - b) <= 1e-9 * max(1.0, abs(b))  # noqa: E731
    if ref["margin"] < 1e-9:
        assert all(close(a, b) for a, b in zip(sorted(h[1] for h in got), sorted(h[1] for h in want))), name
        return True
    assert [h[0] for h in got] == [h[0] for h in want], (name, got, want)
    assert all(close(a[k], b[k]) for a, b in zip(got, want) for k in (1, 2, 3, 4)), (name, got, want)
    return False
