"""Host side of the rounded-operand tests of the reduced-precision convs (tests/test_f16_ops_gpu.py, the split-bf16 part of
tests/test_sk_ops_gpu.py): the packs, their references (tests/slab_ref.py: conv_f16 / conv_x3), the figure E and the mutant
references, all on the CPU, so that tests/test_slab_ref_cpu.py can check on every pack -- without a GPU -- that the bound the GPU
tests use separates the kernel from its mutants.

The bar of a case is 16 E_case, E_case = max |float32-accumulated CPU reference - float64 CPU reference| on the same rounded operands:
reference against reference.  16: the kernels sum in another order (tap-major 32- / 16-wide MFMA steps, stream-K splits) and the
internal accumulation of the f16 / bf16 MFMAs is not documented.  Never above TOL = 2e-4, the f32 routes' bound.
"""
import types

import torch

from tests import slab_ref as R

MARGIN = 16
TOL = 2e-4
KD = [(3, 1), (3, 5), (7, 3), (11, 1), (11, 5)]
F16_BM = {64: 512, 128: 256, 256: 128}          # F16Cfg<CH>::BM of csrc/conv_f16.hip
F16_MAXSEG = 1024                               # segments per conv_f16 launch


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def pack_lens(bm, d, min_rows=0, extra=()):
    """tests/test_slab_ops_gpu.py pack_lens: 1, 2, d - 1, d, d + 1, bm - 1, bm, bm + 1, 2 bm + 3 rows and a long utterance (first)."""
    lens = [3 * bm + 77, 1, bm, 2, bm - 1, d - 1, bm + 1, d, 2 * bm + 3, d + 1] + list(extra) + [1]
    lens[0] += max(0, min_rows - sum(lens))
    return lens


def host_data(Cc, k, d, lens, seed=0, N=None):
    """The draws of tests/test_slab_ops_gpu.py ConvPack, on the host only."""
    N = Cc if N is None else N
    M = sum(lens)
    return types.SimpleNamespace(
        C=Cc, N=N, k=k, d=d, lens=list(lens), segs=R.seg_table(lens), M=M,
        x=rnd(M, Cc, seed=seed + 1), w=rnd(N, Cc, k, seed=seed + 2, scale=(Cc * k) ** -0.5), b=rnd(N, seed=seed + 3, scale=0.1),
        R=rnd(M, N, seed=seed + 4), R2=rnd(M, N, seed=seed + 5))


def err(a, b):
    """max |a - b| in float64 over the rows both cover (rows of no utterance are NaN in every reference)."""
    e = (a.double() - b.double()).abs()
    return e[torch.isfinite(e)].max().item()


# ---- FP16 ------------------------------------------------------------------------------------------
def plant_f16_subnormals(x, spans, seed):
    """Rows [s, s + n) of x, every channel: values of magnitude [2^-15, 2^-14) with random signs -- FP16 subnormals, whole receptive
    fields of them.  On N(0, 1) data one activation in 20 000 is FP16-subnormal and a kernel that flushed them would be off by 1e-6,
    under the accumulation error; over these rows it is off by ~1e-4."""
    g = torch.Generator().manual_seed(seed)
    for s, n in spans:
        mag = (1.0 + torch.rand(n, x.shape[1], generator=g)) * 2.0 ** -15
        sign = torch.randint(0, 2, (n, x.shape[1]), generator=g) * 2 - 1
        x[s:s + n] = mag * sign
    return x


def f16_edge_case(Cc, k, d, seed=0):
    """The ragged edge pack of (C, k, d) at the kernel's block height; 96 rows of the long utterance, across its first block edge,
    hold FP16 subnormals."""
    bm = F16_BM[Cc]
    h = host_data(Cc, k, d, pack_lens(bm, d), seed)
    plant_f16_subnormals(h.x, [(bm - 48, 96)], seed + 6)
    return h


def f16_unsegmented_case(Cc, k=7, d=3, seed=10):
    """One utterance without a segment table, M = 2 BM + 37: not a multiple of the block height."""
    bm = F16_BM[Cc]
    h = host_data(Cc, k, d, [2 * bm + 37], seed)
    plant_f16_subnormals(h.x, [(bm - 48, 96)], seed + 6)
    return h


def short_lens(n):
    return [1 + (7 * i) % 16 for i in range(n)]           # SHORT_256 / SHORT_300 of the f32 tests, extended


SLICE_CASES = [(Cc, k, d, n) for (Cc, k, d) in ((64, 7, 3), (256, 3, 1)) for n in (1024, 1025, 2049)]


def f16_slice_case(Cc, k, d, nseg, seed=20):
    """nseg utterances of 1 .. 16 rows: ceil(nseg / 1024) launches.  Every other 16-row utterance holds FP16 subnormals."""
    h = host_data(Cc, k, d, short_lens(nseg), seed)
    plant_f16_subnormals(h.x, [h.segs[i] for i in range(9, nseg, 32)], seed + 6)
    assert all(n == 16 for _, n in [h.segs[i] for i in range(9, nseg, 32)])
    return h


F16_EPI = {False: {}, True: dict(in_slope=0.1, act_slope=0.1, div=3.0, c2_slope=0.1)}      # what ss_op_conv_f16 exposes, all of it
F16_MUTANTS = {
    "activations toward zero": dict(round_x=R.to_f16_rtz),
    "weights toward zero": dict(round_w=R.to_f16_rtz),
    "subnormal weights flushed": dict(round_w=R.flush_f16_subnormals()),
    "subnormal activations flushed": dict(round_x=R.flush_f16_subnormals()),
}


def f16_refs(h, on, mutants=True):
    """ref / ref2 (float64, the twin), E, bar, {mutant: its float64 reference} of one epilogue setting of an FP16 case."""
    kw = dict(F16_EPI[on])
    if on:
        kw.update(bias=h.b, R=h.R, R2=h.R2)
    run = lambda **m: R.conv_f16(h.x, h.w, h.segs, h.d, **kw, **m)
    first = lambda r: r[0] if on else r
    full = run()
    ref, ref2 = (full if on else (full, None))
    f32 = first(run(accum=torch.float32))
    E = err(f32, ref)
    return types.SimpleNamespace(ref=ref, ref2=ref2, E=E, bar=MARGIN * E, f32=f32,
                                 mutants={n: first(run(**m)) for n, m in F16_MUTANTS.items()} if mutants else {})


# the lattice of the exact-indexing test: FP32 inputs whose FP16 image is known (name, value, image)
_T = 2.0 ** -24
LATTICE = [
    ("1", 1.0, 1.0), ("-1.5", -1.5, -1.5), ("0.333", 0.333251953125, 0.333251953125), ("-3.1416", -3.140625, -3.140625),
    ("1000.5", 1000.5, 1000.5), ("-0.0", -0.0, -0.0), ("0", 0.0, 0.0),
    ("tie 2049 -> 2048", 2049.0, 2048.0), ("tie 2051 -> 2052", 2051.0, 2052.0), ("tie -(1 + 2^-11) -> -1", -(1 + 2.0 ** -11), -1.0),
    ("tie 1 + 3 2^-11 -> 1 + 2^-9", 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -9), ("1 + 2^-11 + 2^-20 -> 1 + 2^-10", 1 + 2.0 ** -11 + 2.0 ** -20, 1 + 2.0 ** -10),
    ("subnormal 2^-24", _T, _T), ("subnormal -2^-24", -_T, -_T), ("subnormal 1023 2^-24", 1023 * _T, 1023 * _T),
    ("subnormal -513 2^-24", -513 * _T, -513 * _T), ("subnormal tie 2^-25 -> 0", _T / 2, 0.0),
    ("subnormal 2^-25 (1 + 2^-10) -> 2^-24", _T / 2 * (1 + 2.0 ** -10), _T), ("subnormal tie 3 2^-25 -> 2^-23", 1.5 * _T, 2 * _T),
    ("subnormal 100.3 2^-24 -> 100 2^-24", 100.3 * _T, 100 * _T), ("2^-26 -> 0", _T / 4, 0.0), ("smallest normal 2^-14", 2.0 ** -14, 2.0 ** -14),
    ("1023.5 2^-24 -> 2^-14", 1023.5 * _T, 2.0 ** -14),
    ("65504", 65504.0, 65504.0), ("-65504", -65504.0, -65504.0), ("65519.9 -> 65504", 65519.9, 65504.0), ("65520 -> 65504", 65520.0, 65504.0),
    ("1e5 -> 65504", 1e5, 65504.0), ("-1e5 -> -65504", -1e5, -65504.0), ("inf -> 65504", float("inf"), 65504.0),
    ("-inf -> -65504", float("-inf"), -65504.0),
]


def lattice_case(Cc, k, d, seed=0, saturated_weights=False):
    """Selection weights and lattice inputs on the edge pack of (C, k, d): output channel n reads ONE (tap j(n), input channel c(n)),
    through a power of two in [2^-4, 2^2] -- c a seeded permutation (every channel once), j a seeded map onto every tap -- so every
    sum has at most one non-zero product, exact in float32, and the output is known to the bit.  saturated_weights: the weights of
    output channels 0 and 1 are 1e6 and -1e6 (FP16: +-65504; 65504 times an FP16 value is still exact in float32).
    h.src [M, C]: the lattice index behind output (m, n), -1 where the tap falls outside the utterance."""
    bm = F16_BM[Cc]
    h = host_data(Cc, k, d, pack_lens(bm, d), seed)
    g = torch.Generator().manual_seed(1000 + seed)
    h.idx = torch.randint(0, len(LATTICE), (h.M, Cc), generator=g)
    h.x = torch.tensor([v for _, v, _ in LATTICE], dtype=torch.float32)[h.idx]
    h.cmap = torch.randperm(Cc, generator=g)
    h.jmap = (torch.randperm(Cc, generator=g) % k)[torch.randperm(Cc, generator=g)]
    assert sorted(h.cmap.tolist()) == list(range(Cc)) and sorted(set(h.jmap.tolist())) == list(range(k))
    h.scale = 2.0 ** torch.randint(-4, 3, (Cc,), generator=g).float()
    if saturated_weights:
        h.scale[0], h.scale[1] = 1e6, -1e6
    h.w = torch.zeros(Cc, Cc, k)
    h.w[torch.arange(Cc), h.cmap, h.jmap] = h.scale
    pad = d * (k - 1) // 2
    h.src = torch.full((h.M, Cc), -1, dtype=torch.long)
    for s, n in h.segs:
        if n == 0:
            continue
        rows = torch.arange(n)[:, None] - pad + h.jmap[None, :] * d                  # [n, C] source row inside the utterance
        ok = (rows >= 0) & (rows < n)
        got = h.idx[s + rows.clamp(0, n - 1), h.cmap[None, :].expand(n, Cc)]
        h.src[s:s + n] = torch.where(ok, got, torch.full_like(got, -1))
    return h


def lattice_expected(h, in_slope=None):
    """The output of lattice_case written down WITHOUT a conv: weight image times input image, from the table's third column (with
    the input leaky-ReLU: the image of fmaxf(v, v * slope), by numpy's float16 conversion)."""
    import numpy as np
    vals = np.array([v for _, v, _ in LATTICE], dtype=np.float32)
    if in_slope is None:
        img = np.array([i for _, _, i in LATTICE], dtype=np.float64)
    else:
        with np.errstate(over="ignore"):
            img = np.clip(np.maximum(vals, vals * np.float32(in_slope)), -65504, 65504).astype(np.float16).astype(np.float64)
    wimg = torch.from_numpy(np.clip(h.scale.numpy(), -65504, 65504).astype(np.float16).astype(np.float64))
    img = torch.cat([torch.from_numpy(img), torch.zeros(1, dtype=torch.float64)])            # index -1: outside the utterance
    out = img[h.src] * wimg[None, :]
    return out + 0.0                                                                         # (-0 products sum to +0 in the kernel)


# ---- split-bf16 ------------------------------------------------------------------------------------
X3_EPI = {False: {}, "up": dict(c2_slope=0.1), True: dict(in_slope=0.1, act_slope=0.2, alpha=0.5, div=3.0, c2_slope=0.3)}
X3_MUTANTS = {"+ll": ("hh", "hl", "lh", "ll"), "-hl": ("hh", "lh"), "-lh": ("hh", "hl")}


def x3_refs(h):
    """{on: ref / ref2 / E / bar / mutants} for ConvPack's three epilogue settings of a split-bf16 case (h: a ConvPack or host_data).
    The term convs are shared: one set without the input activation (on = False, "up"), one with it (on = True)."""
    out, parts = {}, {}
    for on, epi in X3_EPI.items():
        kw = dict(epi)
        if on:
            kw.update(bias=h.b)
        if on is True:
            kw.update(R=h.R, R2=h.R2)
        slope = kw.pop("in_slope", None)
        if slope not in parts:
            parts[slope] = (R.x3_parts(h.x, h.w, h.segs, h.d, slope),
                            R.x3_parts(h.x, h.w, h.segs, h.d, slope, accum=torch.float32, terms=("hh", "hl", "lh")))
        p64, p32 = parts[slope]
        first = lambda r: r[0] if on else r
        full = R.conv_x3(h.x, h.w, h.segs, h.d, parts=p64, **kw)
        ref, ref2 = full if on else (full, None)
        f32 = first(R.conv_x3(h.x, h.w, h.segs, h.d, parts=p32, accum=torch.float32, **kw))
        E = err(f32, ref)
        out[on] = types.SimpleNamespace(ref=ref, ref2=ref2, E=E, bar=MARGIN * E, f32=f32,
                                        mutants={n: first(R.conv_x3(h.x, h.w, h.segs, h.d, terms=t, parts=p64, **kw))
                                                 for n, t in X3_MUTANTS.items()})
    return out


def nearest(out, refs, M):
    """{mutant: (distance to the reference, distance to the mutant reference)} of a result out [>= M rows]."""
    d0 = err(out[:M], refs.ref)
    return {n: (d0, err(out[:M], m)) for n, m in refs.mutants.items()}
