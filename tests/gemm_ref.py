"""Plain torch float64 reference of the conv-GEMM contract at the top of csrc/gemm.hpp, for one utterance and for a segment table:

    out[m, n] = epi( sum_{j < taps} sum_{c < Cin} act_in(A[m * stride + j * dil - pad, c]) * W[n, j * Cin + c] )

restated from that formula with no regard for tiles, k-splits or kernels: input rows outside [0, in_len) read as zero, with chunk > 0
rows at or beyond ((m * stride) // chunk + 1) * chunk read as zero too; the optional prologue is LayerNorm over the Cin columns
(eps 1e-5, linears only) or a leaky-ReLU on the input; the epilogue runs in the kernels' order -- + bias, activation, * alpha, + R,
R2 + ., / div -- or is the GLU over [16 value | 16 gate] column blocks; the twin is C2 = leaky_relu(C, c2_slope).

W is the launcher's own layout, [N, taps * Cin] tap-major (weights.conv_tap_major of a [N, Cin, taps] conv weight).  Everything is
computed in the dtype the inputs come in: float64 for the reference, float32 for the plain chain a measured bound rests on.
tests/test_gemm_ref_cpu.py pins it to torch.nn.functional, tests/stream_ref.py and tests/slab_ref.py.
"""
import torch

ACT_NONE, ACT_SILU, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3, 4      # enum Act of csrc/common.hpp


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


def layernorm(x, g, b, eps=1e-5):
    """Two-pass LayerNorm over the last axis, every step in x's dtype."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    return d / torch.sqrt(var + eps) * g + b


def activate(v, act, slope=0.1):
    if act == ACT_SILU:
        return v / (1.0 + torch.exp(-v))
    if act == ACT_RELU:
        return torch.clamp(v, min=0.0)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_LRELU:
        return lrelu(v, slope)
    assert act == ACT_NONE
    return v


def out_len_of(in_len, taps, stride, pad, dil=1):
    """Rows of a conv's output as torch counts them, floored at 0 (an utterance shorter than the kernel's reach gives none)."""
    return max(0, (in_len + 2 * pad - dil * (taps - 1) - 1) // stride + 1)


def contract(x, W, M, taps=1, dil=1, stride=1, pad=0, in_len=None, chunk=0):
    """The double sum alone for ONE utterance: x [rows >= in_len, Cin] (already activated), W [N, taps * Cin] -> [M, N]."""
    cin = x.shape[1]
    in_len = x.shape[0] if in_len is None else in_len
    assert W.shape[1] == taps * cin and in_len <= x.shape[0]
    m = torch.arange(M)
    limit = torch.full((M,), in_len, dtype=torch.long)
    if chunk > 0:
        limit = torch.minimum(limit, ((m * stride) // chunk + 1) * chunk)
    acc = x.new_zeros(M, W.shape[0])
    for j in range(taps):
        p = m * stride + j * dil - pad
        ok = (p >= 0) & (p < limit)
        rows = x[p.clamp(0, max(x.shape[0] - 1, 0))] if x.shape[0] else x.new_zeros(M, cin)
        rows = torch.where(ok[:, None], rows, torch.zeros_like(rows))
        acc = acc + rows @ W[:, j * cin:(j + 1) * cin].t()
    return acc


def glu_blocks(v):
    """[M, N] in blocks of [16 value | 16 gate] -> [M, N / 2]: value * sigmoid(gate)."""
    M, N = v.shape
    assert N % 32 == 0
    blk = v.reshape(M, N // 32, 2, 16)
    return (blk[:, :, 0] / (1.0 + torch.exp(-blk[:, :, 1]))).reshape(M, N // 2)


def epilogue(acc, bias=None, act=ACT_NONE, act_slope=0.1, alpha=1.0, R=None, R2=None, div=0.0, glu=False):
    v = acc if bias is None else acc + bias
    if glu:
        assert act == ACT_NONE and alpha == 1.0 and R is None and R2 is None and div == 0.0
        return glu_blocks(v)
    v = activate(v, act, act_slope) * alpha
    if R is not None:
        v = v + R
    if R2 is not None:
        v = R2 + v
    if div > 0:
        v = v / div
    return v


def gemm(A, W, M=None, taps=1, dil=1, stride=1, pad=0, in_len=None, chunk=0, in_slope=None, ln=None, bias=None, act=ACT_NONE,
         act_slope=0.1, alpha=1.0, R=None, R2=None, div=0.0, glu=False, c2_slope=None, segs=None, out_rows=None):
    """The whole launch.  One utterance (segs None): A [rows, Cin], output rows [0, M) (M defaults to the rows of A, in_len too).
    Segment table: segs = [(out_start, out_len, in_start, in_len)], every utterance convolved ALONE from A[in_start : in_start +
    in_len] into rows [out_start, out_start + out_len) of an [out_rows, .] result; rows of no utterance come back as NaN.  R / R2 are
    indexed by output row.  ln = (gamma, beta): LayerNorm of the A rows first (taps == 1).  Returns C, or (C, C2) with c2_slope."""
    if ln is not None:
        assert taps == 1 and in_slope is None
        A = layernorm(A, ln[0], ln[1])
    elif in_slope is not None:
        A = lrelu(A, in_slope)
    kw = dict(taps=taps, dil=dil, stride=stride, pad=pad, chunk=chunk)
    if segs is None:
        M = A.shape[0] if M is None else M
        acc = contract(A, W, M, in_len=in_len, **kw)
    else:
        if out_rows is None:
            out_rows = max([o + n for o, n, _, _ in segs] + [0])
        acc = A.new_full((out_rows, W.shape[0]), float("nan"))
        for o, n, i, ilen in segs:
            if n > 0:
                acc[o:o + n] = contract(A[i:i + ilen], W, n, **kw)
    out = epilogue(acc, bias, act, act_slope, alpha, R, R2, div, glu)
    return out if c2_slope is None else (out, lrelu(out, c2_slope))
