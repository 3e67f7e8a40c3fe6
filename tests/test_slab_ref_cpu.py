"""tests/slab_ref.py against torch.nn.functional.conv1d in float64 -- every utterance cut out of the pack and taken through conv1d on
its own, the epilogue / pair / ResBlock composed step by step here -- plus the ABI check of the entry points
tests/test_slab_ops_gpu.py calls (ss_op_conv_gemm_ex, ss_op_conv_pair, ss_op_resblock_fused, ss_debug_slab).  The last part checks
the rounded-operand references of the FP16 and split-bf16 convs (to_f16_sat, split_bf16, conv_f16, conv_x3) and, on every pack of
tests/rounded_cases.py, that the GPU tests' bound of 16 E separates the reference from its mutants -- without a kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rounded_cases as RC
from tests import slab_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {"ss_op_conv_gemm_ex": 2, "ss_op_conv_pair": 23, "ss_op_resblock_fused": 19, "ss_debug_slab": 2}


def test_abi_symbols_header_and_bindings():
    from streamspeech_amd import lib as L
    lib = L.load()
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, header, re.S)
        assert m, f"{name} has no prototype in the header"
        assert len(m.group(1).split(",")) == nargs, f"{name}: the header declares another argument count"
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header
    # ss_op_conv_args, field for field: the header's struct and the ctypes mirror name the same fields in the same order
    body = re.search(r"typedef struct ss_op_conv_args \{(.*?)\} ss_op_conv_args;", header, re.S).group(1)
    names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s*\*?", "", decl.strip(), count=1).split(",")]
    assert names == [f[0] for f in L.SSOpConvArgs._fields_]
    assert C.sizeof(L.SSOpConvArgs) == 7 * 8 + 22 * 4 + 8 + 3 * 4 + 4      # 7 pointers, 22 scalars, segs, 3 ints, tail padding


def test_fused_entry_points_refuse_without_touching_the_device():
    """The eligibility checks of launch_conv_pair / launch_resblock_fused come before any device call: a CPU-only machine sees them."""
    from streamspeech_amd import lib as L
    lib = L.load()
    arr, dil = (C.c_void_p * 3)(0, 0, 0), (C.c_int32 * 3)(1, 3, 5)
    rb = lambda Cc, k, d=dil, w=arr, nseg=0: lib.ss_op_resblock_fused(None, None, Cc, w, arr, arr, arr, d, None, Cc, None, Cc, 0.0, Cc, k,
                                                                      4096, 0.1, None, nseg)
    assert rb(64, 3) == L.SS_ERR_ARG and rb(32, 5) == L.SS_ERR_ARG and rb(32, 3, w=None) == L.SS_ERR_ARG
    assert rb(32, 11, d=(C.c_int32 * 3)(1, 3, 6)) == L.SS_ERR_ARG and rb(16, 3, nseg=257) == L.SS_ERR_ARG
    pair = lambda Cc, k, d, M=4096, nseg=0: lib.ss_op_conv_pair(None, None, Cc, None, None, None, None, None, Cc, None, Cc, 0.0, None, Cc,
                                                               0.1, Cc, k, d, M, M, 0.1, None, nseg)
    assert pair(16, 4, 1) == L.SS_ERR_ARG and pair(16, 11, 6) == L.SS_ERR_ARG and pair(16, 3, 1, M=2047) == L.SS_ERR_ARG
    assert pair(32, 7, 1) == L.SS_ERR_ARG and pair(16, 3, 1, nseg=257) == L.SS_ERR_ARG
    assert lib.ss_op_conv_gemm_ex(None, None) == L.SS_ERR_ARG


def test_debug_slab_refuses_a_negative_grid():
    from streamspeech_amd import lib as L
    lib = L.load()
    try:
        assert lib.ss_debug_slab(-1, 0) == L.SS_ERR_ARG
        assert lib.ss_debug_slab(-7, -1) == L.SS_ERR_ARG
        assert lib.ss_debug_slab(3, 0) == 0
        assert lib.ss_debug_slab(0, 1 << 40) == 0
    finally:
        assert lib.ss_debug_slab(0, -1) == 0


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).double()


def _conv1d_utt(x, w, b, dil, left, right):
    """One utterance [L, Cin] through F.conv1d with explicit zero padding."""
    return F.conv1d(F.pad(x.t()[None], (left, right)), w, b, dilation=dil)[0].t()


LENS = [1, 2, 4, 5, 6, 37, 1, 130, 3]


@pytest.mark.parametrize("taps,dil", [(1, 1), (2, 1), (3, 1), (3, 5), (4, 3), (7, 3), (11, 1), (11, 5)])
@pytest.mark.parametrize("cin,n", [(16, 16), (8, 24)])
def test_segmented_conv_is_conv1d_per_utterance(taps, dil, cin, n):
    segs = R.seg_table(LENS, start=3)                       # rows 0..2 and the tail belong to no utterance
    M = segs[-1][0] + segs[-1][1] + 2
    x, w, b = rnd(M, cin, seed=1), rnd(n, cin, taps, seed=2, scale=(cin * taps) ** -0.5), rnd(n, seed=3, scale=0.1)
    Rr, R2 = rnd(M, n, seed=4), rnd(M, n, seed=5)
    got, got2 = R.conv(x, w, segs, dil, in_slope=0.1, bias=b, act_slope=0.2, alpha=0.5, R=Rr, R2=R2, div=3.0, c2_slope=0.3)
    plain = R.conv(x, w, segs, dil)
    covered = torch.zeros(M, dtype=torch.bool)
    span = dil * (taps - 1)
    for s, L in segs:
        covered[s:s + L] = True
        xs = x[s:s + L]
        y = _conv1d_utt(F.leaky_relu(xs, 0.1), w, b, dil, span // 2, span - span // 2)     # even taps: the extra row on the right
        y = F.leaky_relu(y, 0.2) * 0.5
        y = (R2[s:s + L] + (y + Rr[s:s + L])) / 3.0
        assert (got[s:s + L] - y).abs().max() < 1e-12
        assert torch.equal(got2[s:s + L], torch.where(got[s:s + L] > 0, got[s:s + L], got[s:s + L] * 0.3))
        assert (plain[s:s + L] - _conv1d_utt(xs, w, None, dil, span // 2, span - span // 2)).abs().max() < 1e-12
    assert torch.isnan(got[~covered]).all() and torch.isnan(plain[~covered]).all() and torch.isfinite(got[covered]).all()


def test_rectangular_conv_with_an_empty_utterance_is_conv1d_per_utterance():
    """N != Cin (conv_pre, the upsamplers: what tests/test_sk_ops_gpu.py launches) on a pack with an utterance of no rows."""
    lens = [5, 1, 0, 9, 2]
    segs = R.seg_table(lens)
    M, cin, n = sum(lens), 32, 80
    for taps, dil in [(7, 1), (3, 1), (11, 5)]:
        x, w, b = rnd(M, cin, seed=41), rnd(n, cin, taps, seed=42, scale=(cin * taps) ** -0.5), rnd(n, seed=43, scale=0.1)
        got, got2 = R.conv(x, w, segs, dil, bias=b, c2_slope=0.1)
        assert got.shape == (M, n) and torch.isfinite(got).all()         # the empty utterance leaves no uncovered row
        h = dil * (taps - 1) // 2
        for s, L in segs:
            if L:
                assert (got[s:s + L] - _conv1d_utt(x[s:s + L], w, b, dil, h, h)).abs().max() < 1e-12
        assert torch.equal(got2, torch.where(got > 0, got, got * 0.1))


@pytest.mark.parametrize("cin,cout,k,stride", [(64, 32, 8, 4), (128, 64, 11, 5), (16, 8, 4, 2)])
def test_polyphase_conv_is_conv_transpose_per_utterance(cin, cout, k, stride):
    """weights.convT_polyphase through seg_conv (3 taps, pad 1, N = stride * Cout) against F.conv_transpose1d utterance by utterance
    (slab_ref.upsample), utterances of 0, 1 and 2 rows included: the identity the vocoder's upsamplers rest on, at every edge."""
    from streamspeech_amd.weights import convT_polyphase
    lens = [5, 1, 0, 9, 2, 33]
    segs = R.seg_table(lens)
    M = sum(lens)
    x, wt, b = rnd(M, cin, seed=51), rnd(cin, cout, k, seed=52, scale=(cin * k / stride) ** -0.5), rnd(cout, seed=53, scale=0.1)
    wp, bp = convT_polyphase(wt.float(), b.float(), stride)
    assert wp.shape == (stride * cout, 3 * cin) and bp.shape == (stride * cout,)
    w3 = wp.double().reshape(stride * cout, 3, cin).permute(0, 2, 1)          # tap-major rows -> [N, Cin, taps]
    got = R.conv(x, w3, segs, 1, pad=1, in_slope=0.1, bias=bp.double())
    ref = R.upsample(x, wt.float().double(), b.float().double(), segs, stride, in_slope=0.1)
    assert ref.shape == (M * stride, cout) and torch.isfinite(ref).all()
    assert (got.reshape(M * stride, cout) - ref).abs().max() < 1e-12
    x2 = x.clone()
    x2[5] += 100.0                                          # the 1-row utterance: nothing of it reaches its neighbours
    ref2 = R.upsample(x2, wt.float().double(), b.float().double(), segs, stride, in_slope=0.1)
    assert torch.equal(ref2[:5 * stride], ref[:5 * stride]) and torch.equal(ref2[6 * stride:], ref[6 * stride:])


def test_segmented_conv_reads_nothing_of_the_neighbours():
    """Changing one utterance changes its own rows only."""
    segs = R.seg_table([5, 1, 40, 2])
    x, w = rnd(48, 16, seed=6), rnd(16, 16, 11, seed=7, scale=0.1)
    a = R.seg_conv(x, w, segs, 5)
    x2 = x.clone()
    x2[5] += 100.0                                          # the 1-row utterance
    b = R.seg_conv(x2, w, segs, 5)
    assert torch.equal(a[:5], b[:5]) and torch.equal(a[6:], b[6:]) and not torch.equal(a[5], b[5])


@pytest.mark.parametrize("taps,dil", [(3, 1), (3, 5), (7, 3), (11, 5)])
@pytest.mark.parametrize("extras", [False, True])
def test_pair_is_two_conv1d_and_a_residual(taps, dil, extras):
    Cc = 16
    segs = R.seg_table(LENS)
    M = sum(LENS)
    x = rnd(M, Cc, seed=11)
    w1, w2 = (rnd(Cc, Cc, taps, seed=12 + i, scale=(Cc * taps) ** -0.5) for i in range(2))
    b1, b2 = rnd(Cc, seed=14, scale=0.1), rnd(Cc, seed=15, scale=0.1)
    R2 = rnd(M, Cc, seed=16) if extras else None
    got = R.pair(x, segs, w1, b1, w2, b2, dil, 0.1, R2, 3.0 if extras else 0.0)
    for s, L in segs:
        xs = x[s:s + L]
        h1, h2 = dil * (taps - 1) // 2, (taps - 1) // 2
        t = _conv1d_utt(F.leaky_relu(xs, 0.1), w1, b1, dil, h1, h1)
        y = _conv1d_utt(F.leaky_relu(t, 0.1), w2, b2, 1, h2, h2) + xs
        if extras:
            y = (R2[s:s + L] + y) / 3.0
        assert (got[s:s + L] - y).abs().max() < 1e-12


@pytest.mark.parametrize("taps,dils", [(3, (1, 3, 5)), (7, (5, 3, 1)), (11, (1, 1, 1)), (11, (1, 3, 5))])
@pytest.mark.parametrize("extras", [False, True])
def test_resblock_is_the_hifigan_recurrence(taps, dils, extras):
    """hifigan.py ResBlock.forward, utterance by utterance: for (c1, c2): xt = c2(lrelu(c1(lrelu(x)))); x = xt + x."""
    Cc = 16
    segs = R.seg_table(LENS)
    M = sum(LENS)
    x = rnd(M, Cc, seed=21)
    W1 = [rnd(Cc, Cc, taps, seed=22 + i, scale=(Cc * taps) ** -0.5) for i in range(3)]
    W2 = [rnd(Cc, Cc, taps, seed=25 + i, scale=(Cc * taps) ** -0.5) for i in range(3)]
    B1 = [rnd(Cc, seed=28 + i, scale=0.1) for i in range(3)]
    B2 = [rnd(Cc, seed=31 + i, scale=0.1) for i in range(3)]
    R2 = rnd(M, Cc, seed=34) if extras else None
    got = R.resblock(x, segs, W1, B1, W2, B2, dils, 0.1, R2, 3.0 if extras else 0.0)
    for s, L in segs:
        u = x[s:s + L].t()[None]                            # [1, C, L] as the module sees it
        for i in range(3):
            xt = F.conv1d(F.leaky_relu(u, 0.1), W1[i], B1[i], dilation=dils[i], padding=dils[i] * (taps - 1) // 2)
            xt = F.conv1d(F.leaky_relu(xt, 0.1), W2[i], B2[i], padding=(taps - 1) // 2)
            u = xt + u
        y = u[0].t()
        if extras:
            y = (R2[s:s + L] + y) / 3.0
        assert (got[s:s + L] - y).abs().max() < 1e-11
    f32 = R.resblock(x.float(), segs, [w.float() for w in W1], [b.float() for b in B1], [w.float() for w in W2],
                     [b.float() for b in B2], dils, 0.1, None if R2 is None else R2.float(), 3.0 if extras else 0.0)
    assert f32.dtype == torch.float32 and (f32.double() - got).abs().max() < 1e-4      # the float32 chain is the same function


# ---- the rounded-operand references of the reduced-precision routes (tests/test_f16_ops_gpu.py, split-bf16 in tests/test_sk_ops_gpu.py) ----
# value -> FP16 image, written down by hand: ties at 2^-25 (to 0) and at 2049 (to 2048), the clamp, the subnormal range
F16_TABLE = [(name, v, img) for name, v, img in RC.LATTICE] + [
    ("largest below the clamp's tie", 65519.996, 65504.0), ("3e38", 3e38, 65504.0), ("-3e38", -3e38, -65504.0),
    ("smallest subnormal", 2.0 ** -24, 2.0 ** -24), ("largest subnormal", 1023 * 2.0 ** -24, 1023 * 2.0 ** -24),
    ("tie at 2^-25", 2.0 ** -25, 0.0), ("tie at 2049", 2049.0, 2048.0), ("-2049", -2049.0, -2048.0),
]


def test_to_f16_sat_on_named_values():
    """Against the hand-written images and against numpy's own float16 conversion after a numpy clip, bit for bit (the sign of zero
    included), from float32 and from float64; the mutants differ from it where they should."""
    names = [n for n, _, _ in F16_TABLE]
    for dtype in (torch.float32, torch.float64):
        v = torch.tensor([x for _, x, _ in F16_TABLE], dtype=dtype)
        img = torch.tensor([i for _, _, i in F16_TABLE], dtype=dtype)
        got = R.to_f16_sat(v)
        assert got.dtype == dtype
        with np.errstate(over="ignore"):
            by_numpy = torch.from_numpy(np.clip(v.numpy(), -65504, 65504).astype(np.float16).astype(v.numpy().dtype))
        for want in (img, by_numpy):
            bad = [names[i] for i in range(len(names)) if got[i] != want[i] or torch.signbit(got[i]) != torch.signbit(want[i])]
            assert not bad, bad
        assert torch.equal(got.half().to(dtype), got)                   # every image is an FP16 value
        free = R.to_f16_noclamp(v)
        assert [n for n, a, b in zip(names, free, got) if a != b] == [n for n, x, _ in F16_TABLE if abs(x) >= 65520.0]
        assert torch.isinf(free[[names.index("65520 -> 65504"), names.index("-inf -> -65504")]]).all()
        rtz = R.to_f16_rtz(v)
        assert (rtz.abs() <= v.abs()).all() and (rtz.abs() <= got.abs()).all() and torch.equal(rtz.half().to(dtype), rtz)
        assert rtz[names.index("tie 2051 -> 2052")] == 2050.0 and rtz[names.index("subnormal 2^-25 (1 + 2^-10) -> 2^-24")] == 0.0
        assert rtz[names.index("-1e5 -> -65504")] == -65504.0 and rtz[names.index("tie -(1 + 2^-11) -> -1")] == -1.0
        flushed = R.flush_f16_subnormals()(v)
        sub = got.abs() < 2.0 ** -14
        assert sub.sum() >= 8 and not flushed[sub].any() and torch.equal(flushed[~sub], got[~sub])
    assert torch.isnan(R.to_f16_sat(torch.tensor([float("nan")]))).all()
    # round toward zero, everywhere: the largest FP16 value not above |x|
    x = torch.cat([rnd(20000, seed=91).float(), rnd(20000, seed=92, scale=1e-4).float(), rnd(2000, seed=93, scale=3e4).float()])
    rtz, rne = R.to_f16_rtz(x), R.to_f16_sat(x)
    up = (rtz.half().view(torch.int16) + 1).view(torch.float16).float()          # one FP16 step away from zero
    inside = x.abs() < 65504.0
    assert (rtz.abs() <= x.abs()).all() and (up.abs() > x.abs())[inside].all() and ((rtz == rne) | (up == rne))[inside].all()
    assert 0.3 < (rtz != rne).float().mean() < 0.7


def test_split_bf16_halves():
    """hi and lo are bf16 values (the low 16 bits of their float32 are zero), |x - hi - lo| <= 2^-16 |x|, hi is the nearest bf16."""
    x = torch.cat([rnd(50000, seed=94).float(), rnd(50000, seed=95, scale=0.02).float(), torch.tensor([0.0, -0.0, 1.0, 3.0e38, 1e-30, 257.0, 259.0])])
    hi, lo = R.split_bf16(x)
    assert hi.dtype == lo.dtype == torch.float32
    assert not (hi.view(torch.int32) & 0xFFFF).any() and not (lo.view(torch.int32) & 0xFFFF).any()
    assert ((x.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * x.double().abs()).all()
    assert ((x - hi).abs() <= 2.0 ** -8 * x.abs()).all() and (lo.abs() <= 2.0 ** -8 * x.abs()).all()
    assert hi[-2] == 256.0 and hi[-1] == 260.0                  # ties at 257 / 259 (bf16 step 2 there): to the even significand
    hi2, lo2 = R.split_bf16(x.double())
    assert torch.equal(hi2, hi) and torch.equal(lo2, lo)


def test_conv_f16_and_conv_x3_are_the_conv_of_the_rounded_operands():
    segs = R.seg_table(LENS)
    x, w = rnd(sum(LENS), 16, seed=96).float(), rnd(16, 16, 7, seed=97, scale=0.1).float()
    x[3] = 1e5
    b, Rr = rnd(16, seed=98).float(), rnd(sum(LENS), 16, seed=99).float()
    act = torch.maximum(x, x * 0.1)
    want = R.conv(R.to_f16_sat(act).double(), R.to_f16_sat(w).double(), segs, 3, bias=b.double(), act_slope=0.1, R=Rr.double(), c2_slope=0.1)
    got = R.conv_f16(x, w, segs, 3, in_slope=0.1, bias=b, act_slope=0.1, R=Rr, c2_slope=0.1)
    same = lambda a_, b_: torch.allclose(a_, b_, rtol=1e-13, atol=1e-13, equal_nan=True)      # (seg_conv_packed: other matmul shapes)
    assert got[0].dtype == torch.float64 and same(got[0], want[0]) and same(got[1], want[1])
    gap = R.seg_table(LENS, start=3)                        # rows 0..2 and the tail belong to no utterance: NaN in both
    xg = rnd(gap[-1][0] + gap[-1][1] + 2, 16, seed=90)
    for taps, dil in [(1, 1), (3, 5), (4, 3), (11, 5)]:
        wg = rnd(8, 16, taps, seed=89)
        a_, b_ = R.seg_conv_packed(xg, wg, gap, dil), R.seg_conv(xg, wg, gap, dil)
        assert same(a_, b_) and torch.equal(torch.isnan(a_), torch.isnan(b_)) and torch.isnan(a_[:3]).all()
    f32 = R.conv_f16(x, w, segs, 3, in_slope=0.1, accum=torch.float32, bias=b, act_slope=0.1, R=Rr, c2_slope=0.1)
    assert f32[0].dtype == torch.float32 and 0 < (f32[0].double() - got[0]).abs().max() < 1e-2       # (a row of 65504: f32 ulps of ~1e3)
    assert not torch.isfinite(R.conv_f16(x, w, segs, 3, round_x=R.to_f16_noclamp)).all()
    (ah, al), (wh, wl) = R.split_bf16(act), R.split_bf16(w)
    c = lambda a_, w_: R.seg_conv(a_.double(), w_.double(), segs, 3)
    assert same(R.conv_x3(x, w, segs, 3, in_slope=0.1), c(ah, wh) + c(al, wh) + c(ah, wl))
    assert same(R.conv_x3(x, w, segs, 3, in_slope=0.1, terms=("hh", "ll")), c(ah, wh) + c(al, wl))
    four = R.conv_x3(x, w, segs, 3, in_slope=0.1, terms=("hh", "hl", "lh", "ll"))
    exact = R.seg_conv(act.double(), w.double(), segs, 3)
    assert (four - exact).abs().max() < 2.0 ** -14 * exact.abs().max()      # hi + lo is x to 2^-16


def separates(refs, what, bar_mutants=None):
    """The condition that keeps a GPU bound of 16 E meaningful, on the references alone: the bar is under TOL and under half the
    distance of every mutant reference, and the float32-accumulated reference itself passes the nearest-reference check."""
    dist = {n: RC.err(m, refs.ref) for n, m in refs.mutants.items()}
    near = RC.nearest(refs.f32, refs, refs.ref.shape[0])
    print(f"{what}: E {refs.E:.3e} bar {refs.bar:.3e} mutants " + " ".join(f"[{n}: {v:.3e}]" for n, v in dist.items()))
    assert 0 < refs.E and refs.bar < RC.TOL, f"{what}: bar {refs.bar}"
    for n in bar_mutants or dist:
        assert refs.bar < 0.5 * dist[n], f"{what}: the bar {refs.bar} does not separate the mutant '{n}' at {dist[n]}"
    for n, (d0, dm) in near.items():
        assert d0 < 0.5 * dm, f"{what}: the float32 reference is at {d0} from the reference, {dm} from the mutant '{n}'"


F16_EDGE = [(Cc, k, d) for Cc in (64, 128, 256) for (k, d) in RC.KD]


@pytest.mark.parametrize("Cc,k,d", F16_EDGE)
def test_f16_bar_separates_the_mutants_on_the_edge_packs(Cc, k, d):
    h = RC.f16_edge_case(Cc, k, d)
    bm = RC.F16_BM[Cc]
    assert h.lens[0] >= bm + 48 + (k - 1) * d and {1, 2, d - 1, d, d + 1, bm - 1, bm, bm + 1, 2 * bm + 3} <= set(h.lens)
    for on in (False, True):
        separates(RC.f16_refs(h, on), f"conv_f16 C={Cc} k={k} d={d} on={on}")


@pytest.mark.parametrize("Cc,k,d,nseg", RC.SLICE_CASES)
def test_f16_bar_separates_the_mutants_on_the_slice_packs(Cc, k, d, nseg):
    h = RC.f16_slice_case(Cc, k, d, nseg)
    assert len(h.segs) == nseg and h.M == sum(RC.short_lens(nseg))
    for on in (False, True):
        separates(RC.f16_refs(h, on), f"conv_f16 C={Cc} k={k} d={d} nseg={nseg} on={on}")


def test_f16_unsegmented_and_lattice_references():
    """The unsegmented launches' reference separates too; the lattice reference is one exact product per sum: R.conv_f16 on it equals,
    bit for bit in float32, the product of the hand-written images -- no conv involved -- with the input activation off and on."""
    for Cc in (64, 128, 256):
        h = RC.f16_unsegmented_case(Cc)
        assert h.M % RC.F16_BM[Cc] and len(h.segs) == 1
        for on in (False, True):
            separates(RC.f16_refs(h, on), f"conv_f16 C={Cc} unsegmented on={on}")
    for Cc, k, d, sat in [(64, 11, 5, False), (128, 3, 1, True), (256, 11, 5, True)]:
        h = RC.lattice_case(Cc, k, d, saturated_weights=sat)
        assert set(h.src.unique().tolist()) == set(range(-1, len(RC.LATTICE)))        # every lattice point reaches an output
        for slope in (None, 0.1):
            ref, want = R.conv_f16(h.x, h.w, h.segs, d, in_slope=slope), RC.lattice_expected(h, slope)
            assert torch.isfinite(ref).all() and torch.equal(ref.float().double(), ref)
            assert torch.equal(ref.float().view(torch.int32), want.float().view(torch.int32))
            assert torch.equal(R.conv_f16(h.x, h.w, h.segs, d, in_slope=slope, accum=torch.float32), ref.float())     # exact in float32


def _x3_packs():
    from test_sk_ops_gpu import SHAPES
    return [(shape, pack) for shape in SHAPES for pack in ("edges", "short256", "short300")] + [((128, 256, 3, 1), "one utterance")]


@pytest.mark.parametrize("shape,pack", _x3_packs(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v.replace(" ", "_"))
def test_x3_bar_separates_the_dropped_terms(shape, pack):
    """Split-bf16: 16 E lies under half the distance of a dropped hl or lh term (~2^-9 of the output).  The ll term (~2^-17, about
    1e-5) is nearer than 32 E: no bound separates it, so the GPU test compares distances instead (nearest reference), which the
    float32-accumulated reference passes here for all three."""
    from test_sk_ops_gpu import ROUTES, lens_of
    cin, n, k, d = shape
    lens = [4301] if pack == "one utterance" else lens_of(pack, ROUTES["conv_sk2_x3"]["bm"], d)
    h = RC.host_data(cin, k, d, lens, 0, N=n)
    for on, refs in RC.x3_refs(h).items():
        separates(refs, f"conv_sk2_x3 {shape} {pack} on={on}", bar_mutants=("-hl", "-lh"))
