"""Plain NumPy float64 reference of the ops behind the streaming encoder (ss_encoder_stream_forward, the session pool's batched step
and its CTC path): the chunk-causal strided conv of the subsampler with GLU and a row range, the depthwise conv + BatchNorm(eval) +
SiLU of the Conformer conv module in its ragged, row-range and pooled forms, the pool's row gathers and row stacking, and LayerNorm.

Every op is restated from its definition, one output row at a time, with no regard for tiles: output row m of a conv sees input
position p iff 0 <= p < in_len and, with chunk > 0, p < ((m * stride) // chunk + 1) * chunk -- the end of the chunk output row m's
first sample lies in.  Rows an op is not defined to write come back as NaN (float) / are left alone (caches, which are returned as
copies): tests/test_stream_ops_gpu.py compares bit patterns outside the written rows itself.  tests/test_stream_ref_cpu.py pins all of
it to oracle.streamspeech_oracle.chunk_causal_conv1d and torch.nn.functional in float64.
"""
import numpy as np


def visible_limit(m, stride, chunk, in_len):
    """First input position output row m does not see."""
    return in_len if chunk <= 0 else min(in_len, ((m * stride) // chunk + 1) * chunk)


def chunk_conv(x, w, bias=None, stride=1, pad=0, chunk=0, rows=None, glu=False, out_len=None):
    """x [in_len, Cin], w [N, Cin, taps], bias [N] -> [out_len, N] (glu: [out_len, N / 2]).  out[m] = sum_j x[m stride + j - pad] .
    w[:, :, j]^T over the visible positions.  rows = (m0, m1): only those rows are computed, the others are NaN -- what a row holds
    never depends on where the range starts.  glu: the N output channels are blocks of [16 value | 16 gate] (weights.glu_interleave),
    block b gives output channels 16 b .. 16 b + 15 = value * sigmoid(gate)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    in_len, (N, _, taps) = x.shape[0], w.shape
    if out_len is None:
        out_len = (in_len + 2 * pad - taps) // stride + 1
    m0, m1 = (0, out_len) if rows is None else rows
    acc = np.full((out_len, N), np.nan)
    for m in range(m0, m1):
        lim = visible_limit(m, stride, chunk, in_len)
        v = np.zeros(N) if bias is None else np.asarray(bias, np.float64).copy()
        for j in range(taps):
            p = m * stride + j - pad
            if 0 <= p < lim:
                v = v + w[:, :, j] @ x[p]
        acc[m] = v
    if not glu:
        return acc
    blk = acc.reshape(out_len, N // 32, 2, 16)
    return (blk[:, :, 0] / (1.0 + np.exp(-blk[:, :, 1]))).reshape(out_len, N // 2)


def dwconv(x, w, chunk=0, rows=None):
    """Depthwise conv alone: x [T, C], w [C, K] (K odd), "same" padding K // 2, the visibility rule above at stride 1."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    T, (Cc, K) = x.shape[0], w.shape
    half = K // 2
    t0, t1 = (0, T) if rows is None else rows
    y = np.full((T, Cc), np.nan)
    for t in range(t0, t1):
        lim = visible_limit(t, 1, chunk, T)
        v = np.zeros(Cc)
        for j in range(K):
            p = t + j - half
            if 0 <= p < lim:
                v = v + w[:, j] * x[p]
        y[t] = v
    return y


def bn_silu(y, mean, var, gamma, beta, eps):
    f = lambda a: np.asarray(a, np.float64)
    v = (y - f(mean)) / np.sqrt(f(var) + eps) * f(gamma) + f(beta)
    return v / (1.0 + np.exp(-v))


def dwconv_bn_silu(x, w, mean, var, gamma, beta, eps=1e-5, chunk=0, rows=None):
    """One utterance x [T, C], rows = (t0, t1) or all; rows outside are NaN."""
    return bn_silu(dwconv(x, w, chunk, rows), mean, var, gamma, beta, eps)


def dwconv_bn_silu_ragged(x, segs, w, mean, var, gamma, beta, eps=1e-5, chunk=0, t_begin=0):
    """A pack x [M, C] of utterances segs = [(start, len)]: each convolved alone, rows [t_begin, len) of each; the rest NaN."""
    x = np.asarray(x, np.float64)
    y = np.full((x.shape[0], x.shape[1]), np.nan)
    for s, n in segs:
        if n > t_begin:
            y[s + t_begin:s + n] = dwconv_bn_silu(x[s:s + n], w, mean, var, gamma, beta, eps, chunk, (t_begin, n))[t_begin:]
    return y


def pool_dwconv(gs, cache, sess, w, mean, var, gamma, beta, eps=1e-5):
    """The pooled form.  gs [Ms, C] stacked rows, cache [slots, slot_rows, C], sess = [(q_start, n, r0, T, slot, chunk)] with
    T = r0 + n.  A session's input is its slot's rows [0, r0) followed by its stacked rows gs[q_start : q_start + n]; rows [r0, T) of
    the conv of that utterance go to y[q_start : q_start + n].  Returns (y [Ms, C] with NaN in rows of no session, the cache after
    the call: the stacked rows copied to rows [r0, T) of the slot, in the cache's own dtype, everything else as it was)."""
    gs64 = np.asarray(gs, np.float64)
    y = np.full(gs64.shape, np.nan)
    after = np.array(cache, copy=True)
    for q, n, r0, T, slot, chunk in sess:
        assert T == r0 + n
        x = np.concatenate([np.asarray(cache[slot][:r0], np.float64), gs64[q:q + n]])
        y[q:q + n] = dwconv_bn_silu(x, w, mean, var, gamma, beta, eps, chunk, (r0, T))[r0:]
        after[slot][r0:T] = np.asarray(gs)[q:q + n]
    return y, after


def pool_gather(stk, cache, tab):
    """tab = [(length, k0, nf, slot, s_start)] in call order; stk [Ms, ...] stacked rows, cache [slots, slot_rows, ...].  Row j of a
    session is its slot's row j for j < k0 and stacked row s_start + j - k0 otherwise; rows k0 <= j < nf go to the slot.  Returns
    (the packed output, the cache after the call).  Pure copies: exact in any dtype."""
    out, after = [], np.array(cache, copy=True)
    for length, k0, nf, slot, s0 in tab:
        rows = [cache[slot][j] if j < k0 else stk[s0 + j - k0] for j in range(length)]
        out.extend(rows)
        for j in range(k0, min(nf, length)):
            after[slot][j] = stk[s0 + j - k0]
    return np.array(out, dtype=np.asarray(stk).dtype).reshape((len(out),) + np.asarray(stk).shape[1:]), after


def pool_stack_rows(enc, src, pre):
    """Stacked row r of segment z (pre[z] <= r < pre[z + 1]) = enc[src[z] + r - pre[z]]."""
    out = [enc[src[z] + r - pre[z]] for z in range(len(src)) for r in range(pre[z], pre[z + 1])]
    return np.array(out, dtype=np.asarray(enc).dtype).reshape((len(out),) + np.asarray(enc).shape[1:])


def layernorm(x, gamma, beta, eps=1e-5, dtype=np.float64):
    """Two-pass LayerNorm over the last axis, every step in `dtype` (float64: the reference; float32: the plain chain whose error
    the large-mean bound of the GPU test is measured from)."""
    x, g, b = (np.asarray(a, dtype) for a in (x, gamma, beta))
    D = dtype(x.shape[-1])
    mean = x.sum(-1, keepdims=True, dtype=dtype) / D
    d = x - mean
    var = (d * d).sum(-1, keepdims=True, dtype=dtype) / D
    return d * (dtype(1.0) / np.sqrt(var + dtype(eps))) * g + b
