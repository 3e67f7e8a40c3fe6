"""Plain torch reference of the packed-batch slab convs (csrc/conv_slab.hip, conv_c16 / c32 / c64.hip, conv_c64w.hip) and of the
fused ResBlock (csrc/resblock.hip), in whatever dtype the inputs come in (float64 for the reference, float32 for the chain whose
error the ResBlock bound rests on).  No conv primitive: a conv is the sum over its taps of one matmul per tap on the zero-padded
utterance, so tests/test_slab_ref_cpu.py can check it against torch.nn.functional.conv1d written another way.  (`upsample` is the one
exception, on purpose: torch's conv_transpose1d per utterance, the independent side of the polyphase identity.)

A pack is a [M, C] tensor of utterances laid end to end; `segs` lists (start, len) per utterance.  Every utterance is convolved
ALONE: rows outside it read as zero whatever lies next to it in the pack.  Rows of the pack no segment covers come back as NaN --
no launch may write them.

The second half restates the operand rounding of the reduced-precision routes (csrc/conv_f16.hip, the split-bf16 form of
csrc/conv_sk2.hip), so that their kernels are held to the float64 conv of the operands they really multiply.
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


# ---- the reduced-precision routes: the same conv on operands rounded the way the kernel rounds them ------------------------------
# csrc/conv_f16.hip and the split-bf16 form of csrc/conv_sk2.hip round their operands by a rule that torch restates exactly; every
# product of two rounded operands is exact in float32, so what is left between a kernel and the float64 conv of the ROUNDED operands
# is float32 accumulation alone.  accum=torch.float32 runs the same sums in float32 on the CPU: its distance to the float64 result is
# the figure E the GPU bounds rest on (reference against reference, no kernel involved).
F16_MAX = 65504.0
F16_MIN_NORMAL = 2.0 ** -14


def to_f16_sat(x):
    """FP16 image of x in x's dtype, as to_f16_sat of csrc/conv_f16.hip: clamp to +-65504 (so +-inf lands there, never on inf), round
    to nearest even.  NaN stays NaN."""
    return x.clamp(-F16_MAX, F16_MAX).half().to(x.dtype)


def to_f16_noclamp(x):
    """MUTANT: the conversion without the clamp (65520 and above become inf)."""
    return x.half().to(x.dtype)


def to_f16_rtz(x):
    """MUTANT: clamp, then round TOWARD ZERO instead of to nearest even."""
    c = x.clamp(-F16_MAX, F16_MAX)
    h = c.half()
    away = h.to(c.dtype).abs() > c.abs()                    # rounded away from zero: one FP16 step back (sign-magnitude bits)
    return torch.where(away, (h.view(torch.int16) - 1).view(torch.float16), h).to(x.dtype)


def flush_f16_subnormals(round_fn=to_f16_sat):
    """MUTANT: round_fn followed by a flush of the FP16 subnormals (|h| < 2^-14) to zero."""
    def f(x):
        h = round_fn(x)
        return torch.where(h.abs() < F16_MIN_NORMAL, torch.zeros_like(h), h)
    return f


def split_bf16(x):
    """(hi, lo) of the split-bf16 form, both float32: hi = bf16(x), lo = bf16(x - hi), round to nearest even (x - hi is exact)."""
    xf = x.float()
    hi = xf.bfloat16().float()
    return hi, (xf - hi).bfloat16().float()


def seg_conv_packed(x, w, segs, dil=1, pad=None):
    """seg_conv written another way, for packs of thousands of short utterances: one matmul per tap over the WHOLE pack, on rows
    gathered at m - pad + j dil and zeroed where that row lies outside the utterance of m.  Same taps in the same order."""
    taps = w.shape[2]
    if pad is None:
        pad = dil * (taps - 1) // 2
    M = x.shape[0]
    lo, hi = torch.zeros(M, dtype=torch.long), torch.zeros(M, dtype=torch.long)       # rows of no utterance: the empty range
    for s, n in segs:
        lo[s:s + n], hi[s:s + n] = s, s + n
    y = x.new_zeros(M, w.shape[0])
    for j in range(taps):
        src = torch.arange(M) - pad + j * dil
        ok = (src >= lo) & (src < hi)
        y = y + torch.where(ok[:, None], x[src.clamp(0, M - 1)], x.new_zeros(())) @ w[:, :, j].t()
    y[hi == lo] = float("nan")
    return y


def _in_act_f32(x, in_slope):
    """The kernels' input activation: float32, fmaxf(v, v * slope)."""
    xf = x.float()
    return xf if in_slope is None else torch.maximum(xf, xf * in_slope)


def _epi_as(epi, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in epi.items()}


def conv_f16(x, w, segs, dil, in_slope=None, accum=torch.float64, round_x=to_f16_sat, round_w=to_f16_sat, **epi):
    """conv() as csrc/conv_f16.hip computes it up to accumulation: the input leaky-ReLU in float32, activations and weights through
    to_f16_sat, then seg_conv_packed and the epilogue in `accum` (float64: the reference; float32: the figure E).  round_x / round_w take
    the mutant conversions above."""
    xh, wh = round_x(_in_act_f32(x, in_slope)), round_w(w.float())
    return epilogue(seg_conv_packed(xh.to(accum), wh.to(accum), segs, dil), **_epi_as(epi, accum))


X3_TERMS = {"hh": (0, 0), "hl": (0, 1), "lh": (1, 0), "ll": (1, 1)}        # term -> (half of W, half of A); 0: hi, 1: lo


def x3_parts(x, w, segs, dil, in_slope=None, accum=torch.float64, terms=tuple(X3_TERMS)):
    """{term: seg_conv_packed of that pair of halves in `accum`}: hh = W_hi . A_hi, hl = W_hi . A_lo, lh = W_lo . A_hi, ll = W_lo . A_lo."""
    A, W = split_bf16(_in_act_f32(x, in_slope)), split_bf16(w)
    return {t: seg_conv_packed(A[X3_TERMS[t][1]].to(accum), W[X3_TERMS[t][0]].to(accum), segs, dil) for t in terms}


def conv_x3(x, w, segs, dil, in_slope=None, terms=("hh", "hl", "lh"), accum=torch.float64, parts=None, **epi):
    """conv() as the split-bf16 form of csrc/conv_sk2.hip computes it up to accumulation: the sum of the chosen terms (the kernel's
    three by default) and the epilogue in `accum`.  parts: x3_parts(...) of the same operands, to share the convs between term sets."""
    if parts is None:
        parts = x3_parts(x, w, segs, dil, in_slope, accum, terms)
    acc = parts[terms[0]].to(accum)
    for t in terms[1:]:
        acc = acc + parts[t].to(accum)
    return epilogue(acc, **_epi_as(epi, accum))
