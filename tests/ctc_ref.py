"""The scored CTC search restated in NumPy: masked_argmax_lprob_kernel and ctc_collapse_spans_kernel (csrc/ctc_scores.hip) in float64,
the token sum also in sequential float32 (the order the kernel promises), and words_from_ctc (streamspeech_amd/words.py) written
out independently.  tests/test_ctc_ref_cpu.py holds these against torch and the reference's own post-processing rule;
tests/test_ctc_scores_gpu.py holds the kernels against these."""
import math

import numpy as np


def masked_argmax_lprob(x, N, masks=(), ld=None):
    """x [M, ld] float32 -> (ids int32 [M], lprob float64 [M]) over columns [0, N).  ids: masked columns skipped, NaN counts as
    -inf but stays a candidate, the lowest index wins a tie.  lprob = log_softmax over the FULL row (masks after), at ids; NaN if
    the row holds a NaN."""
    x = np.asarray(x, np.float32)[:, :N]
    M = x.shape[0]
    ids, lp = np.zeros(M, np.int32), np.zeros(M, np.float64)
    keep = np.array([n not in masks for n in range(N)])
    for m in range(M):
        r = x[m].astype(np.float64)
        c = np.where(np.isnan(r), -np.inf, r)
        c = np.where(keep, c, np.nan)                      # masked: not a candidate
        cand = np.nonzero(keep)[0]
        best = cand[0]
        for n in cand:                                     # first maximum
            if c[n] > c[best]:
                best = n
        ids[m] = best
        if np.isnan(r).any():
            lp[m] = np.nan
            continue
        mx = r.max()
        with np.errstate(invalid="ignore", divide="ignore"):
            lse = math.log(np.exp(r - mx).sum()) if np.isfinite(mx) else np.nan
            lp[m] = (c[best] - mx) - lse
    return ids, lp


def collapse_spans(raw, lprob, blank, pad):
    """-> (tokens, index, last, tok_lprob float64, tok_lprob sequential float32): drop repeats, then blank and pad
    (agent/ctc_decoder.py:66-88); per kept token the last frame of its run of equal raw ids and the sum of lprob over the run."""
    raw = [int(v) for v in raw]
    lp = np.asarray(lprob, np.float32)
    T = len(raw)
    toks, index, last, s64, s32 = [], [], [], [], []
    i = 0
    while i < T:
        e = i
        while e + 1 < T and raw[e + 1] == raw[i]:
            e += 1
        if raw[i] != blank and raw[i] != pad:
            toks.append(raw[i])
            index.append(i)
            last.append(e)
            s64.append(float(lp[i:e + 1].astype(np.float64).sum()))
            acc = lp[i]
            for k in range(i + 1, e + 1):
                acc = np.float32(acc + lp[k])
            s32.append(acc)
        i = e + 1
    return toks, index, last, np.asarray(s64, np.float64), np.asarray(s32, np.float32)


def collapse_spans_segmented(raw, lprob, segs, blank, pad):
    """The packed form: segs [(start, len)] -> the packed output arrays as the kernel leaves them (untouched entries None)."""
    n = len(raw)
    toks, index, last, s32 = [None] * n, [None] * n, [None] * n, [None] * n
    counts = []
    for st, ln in segs:
        t, i, l, _, s = collapse_spans(raw[st:st + ln], lprob[st:st + ln], blank, pad)
        counts.append(len(t))
        for k in range(len(t)):
            toks[st + k], index[st + k], last[st + k], s32[st + k] = t[k], i[k], l[k], s[k]
    return toks, index, last, s32, counts


def words(tokens, index, last, tok_lprob, symbols, frame_ms=40, n_final=None, finished=False, t0_ms=0):
    """words_from_ctc, independently: [(text, start_ms, end_ms, confidence, stable)]."""
    out, cur = [], None
    for j, t in enumerate(tokens):
        sym = symbols[t]
        if cur is None or sym.startswith("▁"):
            cur = {"text": "", "first": index[j], "last": last[j], "lp": 0.0, "frames": 0}
            out.append(cur)
        cur["text"] += sym.replace("▁", "")
        cur["last"] = last[j]
        cur["lp"] += float(tok_lprob[j])
        cur["frames"] += last[j] - index[j] + 1
    res = []
    for k, w in enumerate(out):
        if finished:
            stable = True
        elif n_final is None:
            stable = None
        else:
            stable = k + 1 < len(out) and out[k + 1]["first"] < n_final
        conf = math.exp(w["lp"] / w["frames"]) if not math.isnan(w["lp"]) else float("nan")
        res.append((w["text"], t0_ms + w["first"] * frame_ms, t0_ms + (w["last"] + 1) * frame_ms, conf, stable))
    return res
