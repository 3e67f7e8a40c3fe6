"""Plain references of the decode glue kernels (csrc/elementwise.hip) and of the beam-search kernels (csrc/beam_kernels.hip): NumPy, float64
where there is arithmetic, one obvious expression or loop per operation, no tiling and no tricks.  tests/test_glue_ref_cpu.py checks
each against the torch expression the kernel's comment cites; tests/test_glue_ops_gpu.py checks the kernels against them.

Shapes and layouts are the kernels' (see the comments of csrc/elementwise.hpp and BeamState in csrc/beam.hpp); ids are Python ints or
int64 arrays, never wrapped.
"""
import numpy as np

NEG = -np.inf
CAND = 64            # row stride of the candidate lists (SS_OP_BEAM_CAND)


# ---- masked argmax ---------------------------------------------------------------------------------------------------------------
def masked_argmax(logits, N, masks=(-1, -1, -1), force=-1, row_max_len=None, step=0, force_id=-1, row_min_len=None, ban_id=-1):
    """ids[m] = the lowest index of the maximum of logits[m, :N] over the columns not in `masks`, NaN counted as -inf; `force` >= 0
    answers `force`; row_max_len / row_min_len are the per-row forms (force_id on rows at their length, ban_id in place of masks[1]
    on rows below their minimum)."""
    x = np.asarray(logits, np.float64)
    ids = np.empty(x.shape[0], np.int64)
    unmasked = {}
    for m in range(x.shape[0]):
        f, mk = force, list(masks)
        if row_max_len is not None and step >= row_max_len[m]:
            f = force_id
        if row_min_len is not None and step < row_min_len[m]:
            mk[1] = ban_id
        if f >= 0:
            ids[m] = f
            continue
        if tuple(mk) not in unmasked:
            unmasked[tuple(mk)] = np.setdiff1d(np.arange(N), mk)     # ascending
        cols = unmasked[tuple(mk)]
        v = x[m, cols]
        v = np.where(np.isnan(v), NEG, v)
        ids[m] = cols[np.argmax(v)]           # np.argmax: the first of equal maxima
    return ids


# ---- CTC collapse ----------------------------------------------------------------------------------------------------------------
def ctc_collapse(raw, blank, pad):
    """(tokens, index): frames that differ from their predecessor and are neither blank nor pad."""
    raw = np.asarray(raw, np.int64)
    prev = np.concatenate([[np.iinfo(np.int64).min], raw[:-1]])
    keep = (raw != prev) & (raw != blank) & (raw != pad)
    idx = np.nonzero(keep)[0]
    return raw[idx], idx


# ---- durations -------------------------------------------------------------------------------------------------------------------
def dur_predict(logdur=None, forced=None):
    """(dur [K], cum [K + 1]): dur = max(round_half_even(exp(x) - 1), 1) or the forced durations; cum = [0, cumsum(dur)]."""
    if forced is not None:
        dur = np.asarray(forced, np.int64)
    else:
        with np.errstate(over="ignore"):
            dur = np.maximum(np.rint(np.exp(np.asarray(logdur, np.float64)) - 1.0), 1.0).astype(np.int64)
    return dur, np.concatenate([[0], np.cumsum(dur)]).astype(np.int64)


def round_margin(logdur):
    """Smallest distance of exp(x) - 1 from a rounding boundary (an integer + 0.5)."""
    y = np.exp(np.asarray(logdur, np.float64)) - 1.0
    return float(np.min(np.abs(y - np.floor(y) - 0.5)))


def repeat_rows(emb, dur):
    """out = emb rows repeated dur times each (torch.repeat_interleave)."""
    return np.repeat(np.asarray(emb), np.asarray(dur, np.int64), axis=0)


# ---- embeddings / row movers -----------------------------------------------------------------------------------------------------
def embed_tokens(tok, emb, pos_table, scale, pos0, pos_stride, pad_id, row_pos=None):
    """out[i] = scale * emb[tok[i]] + pos_table[pos_i]; ids outside the table read row 0; a pad token takes position pad_id;
    pos_i = pos0 + i * pos_stride, or pos0 + row_pos[i] clamped to the last row of the table (per-row form)."""
    emb, pos_table = np.asarray(emb, np.float64), np.asarray(pos_table, np.float64)
    out = np.empty((len(tok), emb.shape[1]), np.float64)
    for i, tk in enumerate(np.asarray(tok, np.int64)):
        if tk < 0 or tk >= emb.shape[0]:
            tk = 0
        if tk == pad_id:
            pos = pad_id
        elif row_pos is None:
            pos = pos0 + i * pos_stride
        else:
            pos = pos0 + int(row_pos[i])
        if row_pos is not None and pos >= pos_table.shape[0]:
            pos = pos_table.shape[0] - 1
        out[i] = scale * emb[tk] + pos_table[pos]
    return out


def upsample_add_pos(src, up, pos_row, pad_value):
    """out[u] = src[u // up] + (pos_row unless src[u // up, 0] == pad_value)."""
    src = np.asarray(src, np.float64)
    rep = np.repeat(src, up, axis=0)
    return rep + np.where(rep[:, :1] != pad_value, np.asarray(pos_row, np.float64)[None, :], 0.0)


def gather_rows(idx, table):
    """out[i] = table[idx[i]], ids outside the table read row 0."""
    idx = np.asarray(idx, np.int64)
    return np.asarray(table)[np.where((idx < 0) | (idx >= len(table)), 0, idx)]


def scatter_rows(dst_row, src, dst, D):
    """dst[dst_row[i], :D] = src[i, :D] on a copy of dst; rows outside dst are dropped."""
    out = np.array(dst, copy=True)
    for i, r in enumerate(np.asarray(dst_row, np.int64)):
        if 0 <= r < out.shape[0]:
            out[r, :D] = np.asarray(src)[i, :D]
    return out


# ---- HiFi-GAN conv_post ----------------------------------------------------------------------------------------------------------
def conv_post_tanh(x, w, bias, slope=0.01):
    """wav[t] = tanh(bias + sum_{j < 7, c} w[j, c] * leaky_relu(x[t + j - 3, c])), zero outside [0, T); x [T, C], w [7, C]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    a = np.where(x > 0, x, x * slope)
    T = a.shape[0]
    ap = np.concatenate([np.zeros((3, a.shape[1])), a, np.zeros((3, a.shape[1]))])
    acc = np.zeros(T)
    for j in range(7):
        acc += ap[j:j + T] @ w[j]
    return np.tanh(acc + float(bias))


# ---- beam search -----------------------------------------------------------------------------------------------------------------
def log_softmax(x):
    """float64 log-softmax of one row; a NaN anywhere makes the whole row NaN, as torch's does."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        m = np.max(x)
        return (x - m) - np.log(np.sum(np.exp(x - m)))


def beam_lprobs(row, step, min_len, max_len, cum, pad, unk, eos, unk_pen):
    """The masked, accumulated candidate scores of one hypothesis row (unity/sequence_generator.py:290-327 + BeamSearch.step)."""
    v = log_softmax(row)
    v = np.where(np.isnan(v), NEG, v)
    if 0 <= pad < len(v):
        v[pad] = NEG
    if 0 <= unk < len(v):                      # a vocabulary without the id: nothing to penalise
        v[unk] -= unk_pen
    if step >= max_len:
        e = v[eos]
        v[:] = NEG
        v[eos] = e
    if step < min_len:
        v[eos] = NEG
    if step > 0:
        v = v + float(cum)
    return v


def order(scores, flat):
    """Positions sorted as torch.topk's result is documented for distinct keys and as the kernels promise for equal ones: score
    descending, then flattened index ascending."""
    return np.lexsort((np.asarray(flat), -np.asarray(scores, np.float64)))


def beam_topk(logits, k, t_step, min_len, max_len, npre, done, cum, pad, unk, eos, unk_pen):
    """{row: (scores, tokens)}, the min(2k, V - 1) best candidates of every row that takes part (utterance not done; only beam 0 at
    lock-step index 0)."""
    out = {}
    R, V = logits.shape
    for r in range(R):
        b, j = divmod(r, k)
        if done[b] or (t_step == 0 and j != 0):
            continue
        v = beam_lprobs(logits[r], t_step + npre[b], min_len, max_len[b], cum[r], pad, unk, eos, unk_pen)
        o = order(v, np.arange(V))[:min(2 * k, V - 1)]
        out[r] = (v[o], o)
    return out


def beam_merge(st, B, k, Lc, V, t_step, c0, eos, normalize):
    """One step of the search on a copy of the state `st` (dict of NumPy arrays shaped as BeamState: tok / cum [t_step + 2][R],
    anc [2][R][Lc], cand_s / cand_t [R][CAND], ignore [R], done / max_len / npre / fin_cnt [B], fin_score / fin_len [B][k],
    fin_tok / fin_pos / fin_anc [B][k][Lc]).  Writes exactly what the step defines; everything else keeps its value.

    Per utterance (unity/sequence_generator.py:329-470, finalize_hypos, is_finished): the global top 2k of the beams' lists in
    (score, beam * V + token) order; </s> candidates among the first k that are finite and not ignored are finalised while the table
    has room; the utterance is done when it finalised something and the table is full or it is at its length limit (or it is past
    the limit); the next hypotheses are the first k of `candidates ordered by (masked, position)`, masked meaning ignored or </s>
    among the first k and </s> among the rest, and a masked one that still gets a slot is ignored at the next step; slot j's
    ancestry is its parent's up to the cache index written at this step, then itself."""
    s = {n: np.array(a, copy=True) for n, a in st.items()}
    R, f32 = B * k, np.float32
    cur, nxt = t_step & 1, (t_step + 1) & 1
    ci = c0 + t_step
    for b in range(B):
        r0 = b * k
        step = t_step + int(st["npre"][b])

        def carry():
            for j in range(k):
                s["anc"][nxt, r0 + j, :ci + 1] = st["anc"][cur, r0 + j, :ci + 1]
                s["anc"][nxt, r0 + j, ci + 1] = r0 + j
            s["tok"][t_step + 1, r0:r0 + k] = eos
            s["cum"][t_step + 1, r0:r0 + k] = 0.0

        if st["done"][b]:
            carry()
            continue
        nl, nc = (1 if t_step == 0 else k), 2 * k
        sc = np.concatenate([st["cand_s"][r0 + l, :nc] for l in range(nl)])
        tk = np.concatenate([st["cand_t"][r0 + l, :nc] for l in range(nl)]).astype(np.int64)
        bm = np.repeat(np.arange(nl), nc)
        o = order(sc, bm * V + tk)[:nc]
        sel_s, sel_t, sel_b = sc[o], tk[o], bm[o]
        ign = st["ignore"][r0:r0 + k] != 0
        eosm = (sel_t == eos) & (sel_s != NEG)
        eosm[:k] &= ~ign
        cnt, fins = int(st["fin_cnt"][b]), []
        for q in range(k):
            if eosm[q] and cnt < k:
                fins.append((q, cnt))
                cnt += 1
        s["fin_cnt"][b] = cnt
        done = (bool(eosm[:k].any()) and (cnt == k or step == st["max_len"][b])) or step >= st["max_len"][b]
        s["done"][b] = int(done)
        for q, e in fins:
            s["fin_score"][b, e] = f32(sel_s[q]) / f32(step + 1) if normalize else f32(sel_s[q])
            s["fin_len"][b, e] = t_step + 1
            a = st["anc"][cur, r0 + sel_b[q]]
            s["fin_anc"][b, e, :ci + 1] = a[:ci + 1]
            for u in range(t_step + 1):
                s["fin_tok"][b, e, u] = st["tok"][u + 1, a[c0 + u + 1]] if u < t_step else eos
                c = f32(st["cum"][u + 1, a[c0 + u + 1]]) if u < t_step else f32(sel_s[q])
                p = f32(st["cum"][u, a[c0 + u]]) if u + st["npre"][b] > 0 else f32(0)
                s["fin_pos"][b, e, u] = c - p if u + st["npre"][b] > 0 else c
        if done:
            carry()
            continue
        masked = eosm.copy()
        masked[:k] |= ign
        act = np.argsort(masked * nc + np.arange(nc), kind="stable")[:k]
        s["ignore"][r0:r0 + k] = masked[act]
        for j, q in enumerate(act):
            s["tok"][t_step + 1, r0 + j] = sel_t[q]
            s["cum"][t_step + 1, r0 + j] = sel_s[q]
            s["anc"][nxt, r0 + j, :ci + 1] = st["anc"][cur, r0 + sel_b[q], :ci + 1]
            s["anc"][nxt, r0 + j, ci + 1] = r0 + j
    return s


def beam_prefix_score(logits, ftok, pad, unk, unk_pen):
    """lp[i] = masked float64 log-softmax of row i at ftok[i]; NaN (= no value) where ftok[i] < 0."""
    lp = np.full(len(ftok), np.nan)
    for i, tk in enumerate(ftok):
        if tk < 0:
            continue
        v = log_softmax(logits[i])[tk]
        v = NEG if np.isnan(v) or tk == pad else v
        lp[i] = v - unk_pen if tk == unk else v
    return lp


def beam_prefix_chain(lp, row0, npre, k, cum0, pos):
    """In-order float32 chain per utterance on copies of cum0 [B * k] / pos: cum_p = lp_p + cum_{p-1}, pos_p = cum_p - cum_{p-1}."""
    cum0, pos = np.array(cum0, np.float32), np.array(pos, np.float32)
    lp = np.asarray(lp, np.float32)
    with np.errstate(invalid="ignore"):        # -inf - -inf is NaN here as it is there
        for b, (r, n) in enumerate(zip(row0, npre)):
            c = np.float32(0)
            for p in range(n):
                nc = lp[r + p] + c if p > 0 else lp[r + p]
                pos[r + p] = nc - c if p > 0 else nc
                c = nc
            if n > 0:
                cum0[b * k] = c
    return cum0, pos


# ---- inputs both test files use --------------------------------------------------------------------------------------------------
DUR_SPECIALS = (0.0, -3.0, -np.inf, float(np.log(301.2)))


def dur_inputs(K, seed):
    """float32 log-durations log(1 + n + f), n in [0, 8], f in [0.05, 0.45] or [0.55, 0.95] (so exp(x) - 1 stays 0.05 away from every
    rounding boundary), with DUR_SPECIALS at the front when there is room."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 9, K)
    f = rng.uniform(0.05, 0.45, K) + 0.5 * rng.integers(0, 2, K)
    x = np.log(1.0 + n + f).astype(np.float32)
    if K >= 64:
        x[:len(DUR_SPECIALS)] = DUR_SPECIALS
    return x


def forced_durs(K, seed):
    """Forced durations 0 .. 5 with zeros at the front, in the middle and at the end."""
    d = np.random.default_rng(seed).integers(0, 6, K)
    if K >= 8:
        d[0] = d[K // 2] = d[K // 2 + 1] = d[K - 1] = d[K - 2] = 0
    return d


def ctc_frames(T, V, seed):
    """Random ids in [0, V) in runs of 1 .. 4 frames."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, V, T)
    return np.repeat(ids, rng.integers(1, 5, T))[:T]
