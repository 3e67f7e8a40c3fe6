"""References for the keyword spotter on the CTC heads (the rule: include/streamspeech_hip.h at ss_batch_ctc_spot), in float64 Python
with no torch anywhere, and the ctypes runners the CPU and GPU tests share.

(a) brute(): for a keyword and every (start, end) a Viterbi PINNED to state 0 at `start` and state S - 1 at `end`, summed in frame
    order from 0.0.  A float64 addition is monotone, so the recursion's e_end -- which takes the maximum state by state -- must equal
    max over start of these path maxima EXACTLY, and the start it reports must be one of the maximisers.
(b) spot(): a direct restatement of the recursion with its start frames and of the emission rule, state by state and frame by
    frame; it pins the tie rules (stay > advance > skip, stay > enter, later candidate wins an equal score) and the order."""
import ctypes as C

import numpy as np

HIT = np.dtype([("keyword", "<i4"), ("start", "<i4"), ("end", "<i4"), ("n_labels", "<i4"), ("score", "<f8")])
COUNT = np.dtype([("n_hits", "<i4"), ("status", "<i4"), ("overflow", "<i4"), ("frames", "<i4")])
NEG = float("-inf")


def costs(x):
    """c[t][v] = logit - row max, one float32 subtraction; bad[t]: a NaN in the row, or no finite maximum."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        mx = np.fmax.reduce(x, axis=1)                       # fmax skips a NaN, as fmaxf
        bad = np.isnan(x).any(axis=1) | ~(mx > NEG)
        c = (x - mx[:, None]).astype(np.float32)
    return c, bad


def states(y):
    """The labels of the states [y0, 0, y1, 0, ..., y(L-1)] and, per state, whether it may be entered from s - 2."""
    L = len(y)
    lab = [y[s >> 1] if s % 2 == 0 else 0 for s in range(2 * L - 1)]
    skip = [s % 2 == 0 and s >= 2 and y[s >> 1] != y[(s >> 1) - 1] for s in range(2 * L - 1)]
    return lab, skip


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
def brute(c, y):
    """-> P [T][T] float64: P[start][end] = the best path pinned to state 0 at start and state S - 1 at end (-inf: none)."""
    T = c.shape[0]
    lab, skip = states(y)
    S = len(lab)
    cc = c[:, lab].astype(np.float64)                        # [T][S]
    skip = np.asarray(skip)
    P = np.full((T, T), NEG)
    for st in range(T):
        v = np.full(S, NEG)
        v[0] = 0.0 + cc[st, 0]
        P[st, st] = v[S - 1]
        for t in range(st + 1, T):
            a1 = np.concatenate(([NEG], v[:-1]))
            a2 = np.where(skip, np.concatenate(([NEG, NEG], v[:-2]))[:S], NEG)
            v = np.maximum(np.maximum(v, a1), a2) + cc[t]
            P[st, t] = v[S - 1]
    return P


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
class KeywordState:
    def __init__(self, y, tau):
        self.y, self.L = list(y), len(y)
        self.lab, self.skip = states(y)
        self.S = len(self.lab)
        self.thr = -float(np.float32(tau)) * self.L
        self.a = [NEG] * self.S
        self.b = [-1] * self.S
        self.P = None                                        # (score, start, end)
        self.last_end = -1

    def frame(self, crow, t, k, hits, trace=None):
        a, b = self.a, self.b
        na, nb = [0.0] * self.S, [0] * self.S
        for s in range(self.S):
            x = float(crow[self.lab[s]])
            if s == 0:
                if a[0] >= 0.0:                              # stay beats enter on equality
                    v, st = a[0], b[0]
                else:
                    v, st = 0.0, t
            else:
                v, st = a[s], b[s]                           # stay > advance > skip
                if a[s - 1] > v:
                    v, st = a[s - 1], b[s - 1]
                if self.skip[s] and a[s - 2] > v:
                    v, st = a[s - 2], b[s - 2]
            na[s], nb[s] = v + x, st
        self.a, self.b = na, nb
        e, st = na[-1], nb[-1]
        if trace is not None:
            trace.append((e, st))
        cand = e >= self.thr
        if cand and st <= self.last_end:
            return
        if cand and self.P is not None and st <= self.P[2]:
            if e >= self.P[0]:
                self.P = (e, st, t)
            return
        if self.P is not None:
            hits.append((k, self.P[1], self.P[2], self.L, self.P[0]))
            self.last_end = self.P[2]
        self.P = (e, st, t) if cand else None

    def finish(self, k, hits):
        if self.P is not None:
            hits.append((k, self.P[1], self.P[2], self.L, self.P[0]))
            self.P = None


def order(hits):
    return sorted(hits, key=lambda h: (h[2], h[0], h[1]))


def records(hits):
    out = np.zeros(len(hits), HIT)
    for i, h in enumerate(hits):
        out[i] = h
    return out


def spot(x, phrases, taus, trace=None):
    """One utterance -> (status, hits in the returned order as HIT records).  trace: a dict keyword -> [(e_t, s_t)] to fill."""
    c, bad = costs(x)
    if bad.any():
        return 2, records([])
    hits = []
    ks = [KeywordState(y, t) for y, t in zip(phrases, taus)]
    for t in range(c.shape[0]):
        for k, st in enumerate(ks):
            st.frame(c[t], t, k, hits, None if trace is None else trace.setdefault(k, []))
    for k, st in enumerate(ks):
        st.finish(k, hits)
    return 0, records(order(hits))


# ---- the library ----------------------------------------------------------------------------------------------------------------
def _i32(v):
    return (C.c_int32 * max(len(v), 1))(*[int(x) for x in v])


class KeywordSet:
    """ss_ctc_spot_set over plain lists; .rc is the creation's return code."""

    def __init__(self, lib, phrases, taus, V, pad=-1, unk=-1):
        self.lib, self.h = lib, C.c_void_p()
        tok = np.asarray([t for p in phrases for t in p] or [0], np.int32)
        off = np.cumsum([0] + [len(p) for p in phrases]).astype(np.int32)
        tau = np.asarray(list(taus) or [0.0], np.float32)
        self.rc = lib.ss_ctc_spot_set_create(len(phrases), tok.ctypes.data, off.ctypes.data, tau.ctypes.data, V, pad, unk,
                                             C.byref(self.h))
        self.V = V

    def info(self):
        k, u, g, s, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        assert self.lib.ss_ctc_spot_set_info(self.h, C.byref(k), C.byref(u), C.byref(s), C.byref(g), C.byref(d)) == 0
        return {"keywords": k.value, "labels": u.value, "states": s.value, "workgroups": g.value, "bytes": d.value}

    def close(self):
        if self.h:
            self.lib.ss_ctc_spot_set_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


FILL = 0x5a                                                  # what the outputs hold before a call: a refusal must leave it


def run(lib, kset, xs, max_hits, gpu=False, ld=None, T=None):
    """The one-shot call on a pack of logits arrays -> (rc, hits [B][max_hits], counts [B]), the outputs pre-filled with FILL."""
    B = len(xs)
    V = kset.V
    ld = V if ld is None else ld
    T = [x.shape[0] for x in xs] if T is None else T
    flat = np.zeros((max(sum(x.shape[0] for x in xs), 1), ld), np.float32)
    r = 0
    for x in xs:
        flat[r:r + x.shape[0], :min(x.shape[1], ld)] = x[:, :ld]
        r += x.shape[0]
    nb, nh = max(B, 1), max(max_hits, 1)
    if not gpu:
        hits = np.frombuffer(bytearray([FILL]) * (nb * nh * HIT.itemsize), HIT).reshape(nb, nh).copy()
        counts = np.frombuffer(bytearray([FILL]) * (nb * COUNT.itemsize), COUNT).copy()
        rc = lib.ss_ctc_spot_host(flat.ctypes.data, ld, B, _i32(T), kset.h, max_hits, hits.ctypes.data, counts.ctypes.data)
        return rc, hits, counts
    import torch
    d = torch.from_numpy(flat).cuda()
    dh = torch.full((nb * nh * HIT.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    dc = torch.full((nb * COUNT.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    rc = lib.ss_op_ctc_spot(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(d.data_ptr()), ld, B, _i32(T), kset.h,
                            max_hits, C.c_void_p(dh.data_ptr()), C.c_void_p(dc.data_ptr()))
    torch.cuda.synchronize()
    return rc, dh.cpu().numpy().view(HIT).reshape(nb, nh), dc.cpu().numpy().view(COUNT)


def trace(lib, kset, x):
    """The host twin's e_t and s_t of every keyword on one utterance -> (rc, e [T][K] float64, start [T][K] int32)."""
    x = np.ascontiguousarray(x, np.float32)
    K = kset.info()["keywords"]
    e = np.zeros((x.shape[0], K), np.float64)
    s = np.zeros((x.shape[0], K), np.int32)
    rc = lib.ss_debug_ctc_spot_trace_host(x.ctypes.data, x.shape[1], x.shape[0], kset.h, e.ctypes.data, s.ctypes.data)
    return rc, e, s


def written(hits, counts, b=0):
    """The records a call wrote for utterance b."""
    return hits[b, :min(int(counts["n_hits"][b]), hits.shape[1])]


class Stream:
    """ss_ctc_spot_stream of ss_debug_ctc_spot_stream_create over logits arrays (host twin, or the kernels with gpu)."""

    def __init__(self, lib, kset, max_sessions, gpu=False):
        self.lib, self.kset, self.gpu, self.h = lib, kset, gpu, C.c_void_p()
        self.rc = lib.ss_debug_ctc_spot_stream_create(kset.h, 1 if gpu else 0, max_sessions, C.byref(self.h))

    def reset(self, slot):
        return self.lib.ss_ctc_spot_stream_reset(self.h, slot)

    def advance(self, slots, new_rows, upto, final, max_hits=64):
        """new_rows[i]: the logits rows [f, upto[i]) of session i -> (rc, hits [n][max_hits], counts [n])."""
        n, V = len(slots), self.kset.V
        flat = np.zeros((max(sum(r.shape[0] for r in new_rows), 1), V), np.float32)
        r = 0
        for x in new_rows:
            flat[r:r + x.shape[0]] = x
            r += x.shape[0]
        nn = max(n, 1)
        if not self.gpu:
            hits = np.frombuffer(bytearray([FILL]) * (nn * max_hits * HIT.itemsize), HIT).reshape(nn, max_hits).copy()
            counts = np.frombuffer(bytearray([FILL]) * (nn * COUNT.itemsize), COUNT).copy()
            rc = self.lib.ss_ctc_spot_stream_advance_host(self.h, n, _i32(slots), flat.ctypes.data, V, _i32(upto),
                                                          _i32([1 if f else 0 for f in final]), max_hits, hits.ctypes.data,
                                                          counts.ctypes.data)
            return rc, hits, counts
        import torch
        d = torch.from_numpy(flat).cuda()
        dh = torch.full((nn * max_hits * HIT.itemsize,), FILL, dtype=torch.uint8, device="cuda")
        dc = torch.full((nn * COUNT.itemsize,), FILL, dtype=torch.uint8, device="cuda")
        rc = self.lib.ss_op_ctc_spot_stream_advance(C.c_void_p(torch.cuda.current_stream().cuda_stream), self.h, n, _i32(slots),
                                                    C.c_void_p(d.data_ptr()), V, _i32(upto), _i32([1 if f else 0 for f in final]),
                                                    max_hits, C.c_void_p(dh.data_ptr()), C.c_void_p(dc.data_ptr()))
        torch.cuda.synchronize()
        return rc, dh.cpu().numpy().view(HIT).reshape(nn, max_hits), dc.cpu().numpy().view(COUNT)

    def close(self):
        if self.h:
            self.lib.ss_ctc_spot_stream_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def stream_utterance(st, x, cuts, slot=0, max_hits=64):
    """One utterance through slot `slot` in the calls (cuts ..., T) -> (the hits of all calls concatenated and sorted, the counts
    of each call)."""
    T, f, got, cnts = x.shape[0], 0, [], []
    for t in list(cuts) + [T]:
        rc, hits, counts = st.advance([slot], [x[f:t]], [t], [t == T], max_hits)
        assert rc == 0
        assert counts["overflow"][0] == 0
        got.append(written(hits, counts).copy())
        cnts.append(counts[0].copy())
        f = t
    allh = np.concatenate(got) if got else records([])
    return np.sort(allh, order=["end", "keyword", "start"]), cnts
