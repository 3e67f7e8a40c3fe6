"""The resumable CTC prefix beam search (csrc/ctc_stream.hip, ss_ctc_stream_*) for its tests: a node-table restatement of
tests/ctc_beam_ref.py:search -- prefixes are trie nodes and (parent node, token) -> node is a table that lives as long as the
utterance, as in the library -- with an option that FORGETS the table at a frame (the mutant a resumable search becomes when the
child table does not survive a cut), and the runner tests/test_ctc_stream_cpu.py (ss_ctc_stream_advance_host) and
tests/test_ctc_stream_gpu.py (ss_op_ctc_stream_advance) share.  The oracle of every comparison is the one-shot search through
tests/ctc_beam_ref.py:run / tests/ctc_beam_lm_ref.py:run and the `raw` bytes of their records: no tolerance anywhere."""
import ctypes as C

import numpy as np

from tests import ctc_beam_ref as R
from tests.ctc_beam_lm_ref import LMHYP
from tests.ctc_beam_ref import G, HYP, NINF, SENT

PART = np.dtype([("frames", "<i4"), ("n_stable", "<i4"), ("n_alive", "<i4"), ("status", "<i4")])


def search_nodes(x, V, pad, unk, beam, cand, nbest, den=None, forget_at=None):
    """tests/ctc_beam_ref.py:search over a node table -> the same dict.  forget_at = c: the child table is emptied before frame c,
    so a string made before the cut and proposed again after it is a second node (its probability split between the two)."""
    x = np.asarray(x, np.float32)
    T = x.shape[0]
    cid = [R.candidates(x[t], V, pad, unk, cand) for t in range(T)]
    bad = bool(np.isnan(x[:, :V]).any()) or (den is not None and bool(np.isnan(np.asarray(den)).any()))
    if bad:
        return {"status": 2, "hyps": [], "margin": np.inf, "cand_id": cid}
    lp = R.frame_values(x, V, pad, unk, den)
    if np.isnan(lp).any():
        return {"status": 2, "hyps": [], "margin": np.inf, "cand_id": cid}
    W = cand + 1
    par, tok, child = [-1], [-1], {}
    bm = [(0, 0.0, NINF)]                # (node, pb, pnb) in rank order
    margin = np.inf

    def labels(n):
        out = []
        while n > 0:
            out.append(tok[n])
            n = par[n]
        return tuple(out[::-1])

    with np.errstate(invalid="ignore"):
        for t in range(T):
            if forget_at == t:
                child.clear()
            ent, where = [], {}          # [node or None, (parent, token), pb', pnb', place in the frame's order]
            for r, (n, pb, pnb) in enumerate(bm):
                tot = np.logaddexp(pb, pnb)
                where[n] = len(ent)
                ent.append([n, None, tot + lp[t, 0], pnb + lp[t, tok[n]] if n > 0 else NINF, r * W])
            for r, (n, pb, pnb) in enumerate(bm):
                tot = np.logaddexp(pb, pnb)
                for j, c in enumerate(cid[t]):
                    if c < 0:
                        continue
                    term = (pb if (n > 0 and c == tok[n]) else tot) + lp[t, c]
                    q = child.get((n, c))
                    if q is not None and q in where:
                        e = ent[where[q]]
                        e[3] = np.logaddexp(e[3], term)
                    else:
                        ent.append([q, (n, c), NINF, term, r * W + 1 + j])
            live = [(np.logaddexp(e[2], e[3]), e) for e in ent]
            live = [(tot, e) for tot, e in live if tot > NINF]
            live.sort(key=lambda v: (-v[0], v[1][4]))
            if len(live) > beam:
                margin = min(margin, live[beam - 1][0] - live[beam][0])
            nxt = []
            for _, e in live[:beam]:
                if e[0] is None:         # a new string: its node, then its place in the table
                    par.append(e[1][0])
                    tok.append(e[1][1])
                    e[0] = child[e[1]] = len(par) - 1
                nxt.append((e[0], e[2], e[3]))
            bm = nxt
    tots = [float(np.logaddexp(pb, pnb)) for _, pb, pnb in bm]
    for a, b in zip(tots[:nbest], tots[1:nbest + 1]):
        margin = min(margin, a - b)
    return {"status": 0, "hyps": [(labels(n), s) for (n, _, _), s in zip(bm[:nbest], tots)], "margin": float(margin), "cand_id": cid}


def common_prefix(seqs):
    """Length of the longest common prefix of the label tuples (0 for none)."""
    seqs = list(seqs)
    if not seqs:
        return 0
    n = 0
    while all(len(s) > n for s in seqs) and len({s[n] for s in seqs}) == 1:
        n += 1
    return n


class Stream:
    """An ss_ctc_stream of ss_debug_ctc_stream_create: host memory and ss_ctc_stream_advance_host, or (gpu) device memory and
    ss_op_ctc_stream_advance.  lm: the library's handle (c_void_p) or None; opts: (lm_weight, word_score, eos_term) or None."""

    def __init__(self, lib, V, pad, unk, S, max_frames, beam, cand, nbest, lm=None, opts=None, gpu=False):
        from streamspeech_amd.lib import SSCtcLmOpts
        self.lib, self.V, self.nbest, self.gpu, self.lm = lib, V, nbest, gpu, lm is not None
        self.h = C.c_void_p()
        o = C.byref(SSCtcLmOpts(opts[0], opts[1], int(opts[2]))) if opts is not None else None
        self.rc = lib.ss_debug_ctc_stream_create(V, pad, unk, int(gpu), S, max_frames, beam, cand, nbest, lm, o, C.byref(self.h))
        assert (self.rc == 0) == bool(self.h.value)

    def reset(self, slot):
        return self.lib.ss_ctc_stream_reset(self.h, slot)

    def close(self):
        if self.h.value:
            self.lib.ss_ctc_stream_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def advance(self, slots, rows, upto, final, out_stride=None, n=None, null=()):
        """rows: per session its NEW rows [k, ld] float32 (k may be 0) -> (rc, records); a record is dict(hyps, status, raw, part
        (frames, n_stable, n_alive, status), part_raw).  Guards and sentinels as tests/ctc_beam_ref.py:run; `null` names arguments
        passed as NULL (the refusals)."""
        n = len(slots) if n is None else n
        B = len(slots)
        ld = rows[0].shape[1] if rows else self.V
        x = np.ascontiguousarray(np.concatenate(list(rows) + [np.zeros((1, ld), np.float32)], 0), np.float32)
        stride = max(list(upto) + [1]) if out_stride is None else out_stride
        nb = self.nbest
        hyp = np.zeros(max(B, 1) * nb + G, LMHYP if self.lm else HYP)
        hyp["status"] = SENT
        toks = np.full(max(B, 1) * nb * max(stride, 1) + G, SENT, np.int32)
        part = np.full((max(B, 1) + G) * 4, SENT, np.int32).view(PART)
        bufs = [hyp, toks, part]
        ar = lambda v: (C.c_int32 * max(len(v), 1))(*[int(a) for a in v])  # noqa: E731
        hs, hu, hf = ar(slots), ar(upto), ar(final)
        hs, hu, hf = [None if k in null else v for k, v in zip(("slots", "upto", "final"), (hs, hu, hf))]
        if self.gpu:
            import torch
            dx = torch.from_numpy(x).cuda()
            dev = [torch.from_numpy(b.view(np.uint8).copy()).cuda() for b in bufs]
            ptr = [C.c_void_p(d.data_ptr()) for d in dev]
            ptr = [None if k in null else v for k, v in zip(("hyps", "tokens", "part"), ptr)]
            rc = self.lib.ss_op_ctc_stream_advance(C.c_void_p(torch.cuda.current_stream().cuda_stream), self.h, n, hs,
                                                   None if "logits" in null else C.c_void_p(dx.data_ptr()), ld, hu, hf, ptr[0], ptr[1],
                                                   stride, ptr[2])
            torch.cuda.synchronize()
            bufs = [d.cpu().numpy().view(b.dtype) for d, b in zip(dev, bufs)]
        else:
            ptr = [C.c_void_p(b.ctypes.data) for b in bufs]
            ptr = [None if k in null else v for k, v in zip(("hyps", "tokens", "part"), ptr)]
            rc = self.lib.ss_ctc_stream_advance_host(self.h, n, hs, None if "logits" in null else C.c_void_p(x.ctypes.data), ld, hu, hf,
                                                     ptr[0], ptr[1], stride, ptr[2])
        hyp, toks, part = bufs
        if rc != 0:                                                # a refusal writes nothing
            assert (hyp["status"] == SENT).all() and (toks == SENT).all() and (part.view(np.int32) == SENT).all()
            return rc, None
        assert (hyp["status"][B * nb:] == SENT).all() and (toks[B * nb * stride:] == SENT).all(), "wrote behind the last entry"
        assert (part.view(np.int32)[4 * B:] == SENT).all(), "wrote behind the last entry"
        out = []
        for b in range(B):
            h = hyp[b * nb:(b + 1) * nb]
            tr = toks[b * nb * stride:(b + 1) * nb * stride].reshape(nb, stride)
            hyps = []
            for k in range(nb):
                m = int(h["n_tokens"][k])
                assert 0 <= m <= upto[b] and (tr[k, m:] == SENT).all(), "entries past n_tokens were touched"
                lab = tuple(int(v) for v in tr[k, :m])
                if h["status"][k] == 0:
                    hyps.append((lab, float(h["score"][k]), float(h["ctc_score"][k]), float(h["lm_score"][k])) if self.lm
                                else (lab, float(h["score"][k])))
                else:
                    assert m == 0 and (np.isnan(h["score"][k]) if h["status"][k] == 2 else h["score"][k] == NINF)
            p = part[b]
            out.append({"hyps": hyps, "status": h["status"].tolist(),
                        "raw": h.tobytes() + b"".join(tr[k, :int(h["n_tokens"][k])].tobytes() for k in range(nb)),
                        "part": tuple(int(p[k]) for k in PART.names), "part_raw": p.tobytes()})
        return rc, out
