"""tests/gemm_ref.py against torch.nn.functional (linear, conv1d, layer_norm, glu) in float64, tests/stream_ref.chunk_conv for the chunk
rule and tests/slab_ref.py for a ragged "same" conv, plus the ABI check of ss_op_ln_linear_ex (what tests/test_gemm_routes_gpu.py
calls) and the refusals of launch_smallm / launch_canon that must leave the launch census alone -- no GPU anywhere here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_ref as G
from tests import slab_ref, stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"ss_op_ln_linear_ex": 19}


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).double()


def tap_major(w):
    from streamspeech_amd.weights import conv_tap_major
    return conv_tap_major(w)


# ---- ABI ----------------------------------------------------------------------------------------------
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
    # ss_op_ln_linear's arguments in its order, ln_out after ln_b and canon at the end
    old = re.search(r"\bint\s+ss_op_ln_linear\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    new = re.search(r"\bint\s+ss_op_ln_linear_ex\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    names = lambda s: [a.split()[-1].lstrip("*") for a in s.split(",")]
    assert names(new) == names(old)[:5] + ["ln_out"] + names(old)[5:] + ["canon"]
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header


def census(lib):
    out = {}
    for c in range(lib.ss_prof_num_classes()):
        n, fl, by = C.c_int64(), C.c_double(), C.c_double()
        assert lib.ss_prof_totals(c, C.byref(fl), C.byref(by), C.byref(n)) == 0
        out[lib.ss_prof_class_name(c).decode()] = (n.value, fl.value, by.value)
    return out


def test_refused_layernorm_linears_leave_the_census_alone():
    """A LayerNorm-prologue linear no kernel takes (K > 512 on the small-M kernel, by shape or through CANON_SMALLM; ln_out on a shape
    that is not the GEMV's; CANON_SEQ at K != 256) is SS_ERR_ARG and books nothing: the census counts launches, and bench.py's dispatch
    table and the took_since assertions of the op tests read it.  Nothing is launched, so the pointers are never dereferenced."""
    from streamspeech_amd import lib as L
    lib = L.load()
    p = C.c_void_p(0x1000)          # never read
    for M, N, K in [(16, 512, 1024), (3, 512, 4096), (192, 512, 768)]:
        before = census(lib)
        rc = lib.ss_op_ln_linear(None, p, K, p, p, p, p, None, 0, p, N, M, N, K, 0, 1.0, 0)
        assert rc == L.SS_ERR_ARG, f"({M}, {N}, {K}): rc {rc}"
        assert census(lib) == before, f"({M}, {N}, {K}): a refused call was booked as a launch"
    ex = lambda M, N, K, ln_out, canon, ln=True: lib.ss_op_ln_linear_ex(None, p, K, p if ln else None, p if ln else None, ln_out, p, p,
                                                                         None, 0, p, N, M, N, K, 0, 1.0, 0, canon)
    for what, call in [("CANON_SMALLM, ln_g at K = 1024", lambda: ex(40, 512, 1024, None, 2)),
                       ("CANON_SMALLM, 1025 rows", lambda: ex(1025, 32, 64, None, 2, ln=False)),
                       ("the shapes above through the new entry", lambda: ex(16, 512, 1024, None, 0)),
                       ("ln_out at M = 5", lambda: ex(5, 512, 512, p, 0)),
                       ("ln_out at K = 320", lambda: ex(3, 512, 320, p, 0)),
                       ("ln_out under CANON_SMALLM", lambda: ex(3, 512, 512, p, 2)),
                       ("CANON_SEQ with ln_g at K = 320", lambda: ex(50, 64, 320, None, 1)),
                       ("ln_out without LayerNorm", lambda: ex(3, 512, 512, p, 0, ln=False)),
                       ("canon = 3", lambda: ex(3, 512, 512, None, 3))]:
        before = census(lib)
        assert call() == L.SS_ERR_ARG, what
        assert census(lib) == before, f"{what}: a refused call was booked as a launch"
    before = census(lib)
    assert lib.ss_op_ln_linear_ex(None, p, 64, None, p, None, p, p, None, 0, p, 64, 8, 64, 64, 0, 1.0, 0, 0) == L.SS_ERR_ARG    # ln_b alone
    assert census(lib) == before


# ---- the reference against torch.nn.functional -------------------------------------------------------------
@pytest.mark.parametrize("act,ref_act", [(G.ACT_NONE, lambda v: v), (G.ACT_SILU, F.silu), (G.ACT_RELU, F.relu), (G.ACT_TANH, torch.tanh),
                                         (G.ACT_LRELU, lambda v: F.leaky_relu(v, 0.3))])
def test_linear_and_epilogue_order(act, ref_act):
    M, N, K = 13, 21, 40
    x, w, b, R, R2 = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4), rnd(M, N, seed=5)
    got, got2 = G.gemm(x, w, bias=b, act=act, act_slope=0.3, alpha=0.5, R=R, R2=R2, div=3.0, c2_slope=0.2)
    ref = (R2 + (ref_act(F.linear(x, w, b)) * 0.5 + R)) / 3.0
    assert (got - ref).abs().max() < 1e-13
    assert torch.equal(got2, F.leaky_relu(got, 0.2))
    assert (G.gemm(x, w) - F.linear(x, w)).abs().max() < 1e-13
    assert (G.gemm(x, w, M=9) - F.linear(x, w)[:9]).abs().max() < 1e-13


@pytest.mark.parametrize("K", [64, 320])
def test_layernorm_prologue_and_glu(K):
    M, N = 7, 96
    x, g, b = rnd(M, K, seed=11) * 3.0 + 5.0, 1.0 + rnd(K, seed=12, scale=0.1), rnd(K, seed=13, scale=0.1)
    w, bias = rnd(N, K, seed=14, scale=K ** -0.5), rnd(N, seed=15, scale=0.1)
    ln = F.layer_norm(x, (K,), g, b, 1e-5)
    assert (G.layernorm(x, g, b) - ln).abs().max() < 1e-13
    assert (G.gemm(x, w, ln=(g, b), bias=bias, act=G.ACT_SILU) - F.silu(F.linear(ln, w, bias))).abs().max() < 1e-13
    # GLU: blocks of [16 value | 16 gate] are F.glu of [all values | all gates]
    y = F.linear(ln, w, bias).reshape(M, N // 32, 2, 16)
    ref = F.glu(torch.cat([y[:, :, 0].reshape(M, -1), y[:, :, 1].reshape(M, -1)], dim=1), dim=1)
    assert (G.gemm(x, w, ln=(g, b), bias=bias, glu=True) - ref).abs().max() < 1e-13
    f32 = G.layernorm(x.float(), g.float(), b.float())
    assert f32.dtype == torch.float32 and (f32.double() - ln).abs().max() < 1e-4


@pytest.mark.parametrize("taps,dil,stride,pad", [(1, 1, 1, 0), (3, 1, 1, 1), (5, 1, 2, 2), (7, 3, 1, 9), (4, 2, 3, 1), (3, 1, 2, 0),
                                                 (11, 5, 1, 25), (2, 1, 1, 0)])
@pytest.mark.parametrize("in_len", [1, 2, 5, 64, 131])
def test_conv_is_conv1d(taps, dil, stride, pad, in_len):
    cin, n = 8, 12
    x, w, b = rnd(in_len, cin, seed=21), rnd(n, cin, taps, seed=22, scale=(cin * taps) ** -0.5), rnd(n, seed=23, scale=0.1)
    M = G.out_len_of(in_len, taps, stride, pad, dil)
    if M == 0:
        assert in_len + 2 * pad < dil * (taps - 1) + 1
        return
    ref = F.conv1d(x.t()[None], w, b, stride=stride, padding=pad, dilation=dil)[0].t()
    assert ref.shape == (M, n)
    got = G.gemm(x, tap_major(w), M=M, taps=taps, dil=dil, stride=stride, pad=pad, bias=b)
    assert (got - ref).abs().max() < 1e-13
    # the input leaky-ReLU is applied before the zero padding (leaky_relu(0) = 0 either way)
    got = G.gemm(x, tap_major(w), M=M, taps=taps, dil=dil, stride=stride, pad=pad, in_slope=0.1)
    ref = F.conv1d(F.leaky_relu(x, 0.1).t()[None], w, None, stride=stride, padding=pad, dilation=dil)[0].t()
    assert (got - ref).abs().max() < 1e-13


def test_rows_past_in_len_read_as_zero():
    """M != in_len: what the kernel reads beyond in_len is zero whatever the buffer holds there."""
    cin, n, taps = 8, 12, 3
    x, w = rnd(70, cin, seed=31), rnd(n, cin, taps, seed=32)
    got = G.gemm(x, tap_major(w), M=70, taps=taps, pad=1, in_len=50)
    xz = x.clone()
    xz[50:] = 0
    ref = F.conv1d(xz.t()[None], w, None, padding=1)[0].t()
    assert (got - ref).abs().max() < 1e-13 and got[51:].abs().max() == 0 and got[50].abs().max() > 0


@pytest.mark.parametrize("chunk", [0, 8, 16, 5])
@pytest.mark.parametrize("T", [5, 83])
def test_chunk_rule_is_stream_ref(chunk, T):
    cin, n = 16, 64
    x, w, b = rnd(T, cin, seed=41), rnd(n, cin, 5, seed=42, scale=(cin * 5) ** -0.5), rnd(n, seed=43, scale=0.1)
    for glu in (False, True):
        ref = stream_ref.chunk_conv(x.numpy(), w.numpy(), b.numpy(), stride=2, pad=2, chunk=chunk, glu=glu)
        got = G.gemm(x, tap_major(w), M=ref.shape[0], taps=5, stride=2, pad=2, chunk=chunk, bias=b, glu=glu)
        assert got.shape == ref.shape and np.abs(got.numpy() - ref).max() < 1e-13
    ref = stream_ref.chunk_conv(x.numpy(), w[:, :, :3].numpy(), None, stride=1, pad=1, chunk=chunk)
    got = G.gemm(x, tap_major(w[:, :, :3].contiguous()), taps=3, pad=1, chunk=chunk)
    assert np.abs(got.numpy() - ref).max() < 1e-13


def test_ragged_same_conv_is_slab_ref():
    lens = [5, 1, 0, 37, 2, 130]
    segs = slab_ref.seg_table(lens, start=2)                  # rows 0, 1 and the tail belong to no utterance
    rows = segs[-1][0] + segs[-1][1] + 3
    cin, n = 16, 24
    for taps, dil in [(3, 1), (7, 3), (11, 5), (4, 1)]:
        x, w, b = rnd(rows, cin, seed=51), rnd(n, cin, taps, seed=52, scale=(cin * taps) ** -0.5), rnd(n, seed=53, scale=0.1)
        Rr, R2 = rnd(rows, n, seed=54), rnd(rows, n, seed=55)
        ref, ref2 = slab_ref.conv(x, w, segs, dil, in_slope=0.1, bias=b, act_slope=0.2, alpha=0.5, R=Rr, R2=R2, div=3.0, c2_slope=0.3)
        got, got2 = G.gemm(x, tap_major(w), taps=taps, dil=dil, pad=dil * (taps - 1) // 2, in_slope=0.1, bias=b, act=G.ACT_LRELU,
                           act_slope=0.2, alpha=0.5, R=Rr, R2=R2, div=3.0, c2_slope=0.3, segs=[(s, L, s, L) for s, L in segs],
                           out_rows=rows)
        covered = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), covered) and covered.any() and not covered.all()
        assert (got[covered] - ref[covered]).abs().max() < 1e-12 and (got2[covered] - ref2[covered]).abs().max() < 1e-12


def test_ragged_strided_pack_convolves_every_utterance_alone():
    """out_start != in_start: a stride-2 conv over a pack, utterance by utterance through F.conv1d."""
    cin, n, taps, stride, pad = 8, 32, 5, 2, 2
    lens = [1, 2, 5, 64, 0, 65, 131]
    outs = [G.out_len_of(L, taps, stride, pad) for L in lens]
    assert outs == [1, 1, 3, 32, 0, 33, 66]
    segs, o, i = [], 0, 0
    for L, n_out in zip(lens, outs):
        segs.append((o, n_out, i, L))
        o, i = o + n_out, i + L
    x, w, b = rnd(i, cin, seed=61), rnd(n, cin, taps, seed=62), rnd(n, seed=63)
    for chunk in (0, 8):
        got = G.gemm(x, tap_major(w), taps=taps, stride=stride, pad=pad, chunk=chunk, bias=b, segs=segs)
        assert got.shape == (o, n) and torch.isfinite(got).all()
        for (os_, n_out, is_, L) in segs:
            if n_out:
                ref = stream_ref.chunk_conv(x[is_:is_ + L].numpy(), w.numpy(), b.numpy(), stride=stride, pad=pad, chunk=chunk)
                assert np.abs(got[os_:os_ + n_out].numpy() - ref).max() < 1e-13
                if chunk == 0:
                    ref = F.conv1d(x[is_:is_ + L].t()[None], w, b, stride=stride, padding=pad)[0].t()
                    assert (got[os_:os_ + n_out] - ref).abs().max() < 1e-13
