"""Plain torch reference of the packed-batch slab convs (csrc/conv_slab.hip, conv_c16 / c32 / c64.hip, conv_c64w.hip) and of the
fused ResBlock (csrc/resblock.hip), in whatever dtype the inputs come in (float64 for the reference, float32 for the chain whose
error the ResBlock bound rests on).  No conv primitive: a conv is the sum over its taps of one matmul per tap on the zero-padded
utterance, so tests/test_slab_ref_cpu.py can check it against torch.nn.functional.conv1d written another way.  (`upsample` is the one
exception, on purpose: torch's conv_transpose1d per utterance, the independent side of the polyphase identity.)

A pack is a [M, C] tensor of utterances laid end to end; `segs` lists (start, len) per utterance.  Every utterance is convolved
ALONE: rows outside it read as zero whatever lies next to it in the pack.  Rows of the pack no segment covers come back as NaN --
no launch may write them.
"""
import torch
import torch.nn.functional as F


def lrelu(x, slope):
    return torch.where(x > 0, x, x * slope)


def seg_table(lens, start=0):
    """Contiguous (start, len) list of a pack of utterances of these lengths."""
    segs, at = [], start
    for n in lens:
        segs.append((at, int(n)))
        at += int(n)
    return segs


def _conv_one(x, w, taps, dil, pad):
    """x [L, Cin] of ONE utterance, w [N, Cin, taps] -> [L, N]: y[m] = sum_j x[m - pad + j dil] . w[:, :, j]^T, zero outside [0, L).
    Even tap counts at the default pad put the extra padding row on the right."""
    L, cin = x.shape
    right = dil * (taps - 1) - pad
    xp = torch.cat([x.new_zeros(pad, cin), x, x.new_zeros(max(right, 0), cin)])
    y = x.new_zeros(L, w.shape[0])
    for j in range(taps):
        y = y + xp[j * dil: j * dil + L] @ w[:, :, j].t()
    return y


def seg_conv(x, w, segs, dil=1, pad=None, in_slope=None):
    """Segmented "same" conv of the pack x [M, Cin] with w [N, Cin, taps]; in_slope: leaky-ReLU on the input.  No bias."""
    taps = w.shape[2]
    if pad is None:
        pad = dil * (taps - 1) // 2
    xin = x if in_slope is None else lrelu(x, in_slope)
    y = x.new_full((x.shape[0], w.shape[0]), float("nan"))
    for s, n in segs:
        if n > 0:
            y[s:s + n] = _conv_one(xin[s:s + n], w, taps, dil, pad)
    return y


def upsample(x, w, b, segs, stride, in_slope=None):
    """The other way round for the polyphase upsamplers (weights.convT_polyphase): torch's own ConvTranspose1d, w [Cin, Cout, k] with
    padding (k - stride) / 2, on every utterance of the pack x [M, Cin] alone -> [M * stride, Cout]; in_slope: leaky-ReLU on the input.
    Row q of the polyphase conv's [M, stride * Cout] result is rows q * stride .. q * stride + stride - 1 of this."""
    k = w.shape[2]
    xin = x if in_slope is None else lrelu(x, in_slope)
    y = x.new_full((x.shape[0] * stride, w.shape[1]), float("nan"))
    for s, n in segs:
        if n > 0:
            y[s * stride:(s + n) * stride] = F.conv_transpose1d(xin[s:s + n].t()[None], w, b, stride=stride, padding=(k - stride) // 2)[0].t()
    return y


def epilogue(acc, bias=None, act_slope=None, alpha=1.0, R=None, R2=None, div=0.0, c2_slope=None):
    """The GemmArgs epilogue in the kernels' order: + bias, leaky-ReLU(act_slope), * alpha, + R, R2 + ., / div.  Returns C, or
    (C, C2 = leaky_relu(C, c2_slope)) when c2_slope is given."""
    v = acc if bias is None else acc + bias
    if act_slope is not None:
        v = lrelu(v, act_slope)
    v = v * alpha
    if R is not None:
        v = v + R
    if R2 is not None:
        v = R2 + v
    if div > 0:
        v = v / div
    return v if c2_slope is None else (v, lrelu(v, c2_slope))


def conv(x, w, segs, dil=1, pad=None, in_slope=None, **epi):
    return epilogue(seg_conv(x, w, segs, dil, pad, in_slope), **epi)


def pair(x, segs, w1, b1, w2, b2, dil, slope=0.1, R2=None, div=0.0):
    """conv2(lrelu(conv1_dil(lrelu(x)) + b1)) + b2 + x [+ R2] [/ div]  (one (dilated conv, conv, residual) pair of a ResBlock)."""
    mid = seg_conv(x, w1, segs, dil, None, slope) + b1
    y = (seg_conv(mid, w2, segs, 1, None, slope) + b2) + x
    if R2 is not None:
        y = R2 + y
    if div > 0:
        y = y / div
    return y


def resblock(x, segs, W1, B1, W2, B2, dils, slope=0.1, R2=None, div=0.0):
    """for i in 0..2: x = conv2_i(lrelu(conv1_i(lrelu(x)))) + x;  out = [R2 +] x [/ div]  (the recurrence of csrc/resblock.hip)."""
    for i in range(3):
        x = pair(x, segs, W1[i], B1[i], W2[i], B2[i], dils[i], slope)
    if R2 is not None:
        x = R2 + x
    if div > 0:
        x = x / div
    return x
