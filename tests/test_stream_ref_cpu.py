"""tests/stream_ref.py against oracle.streamspeech_oracle.chunk_causal_conv1d and torch.nn.functional in float64 (error bar 1e-12),
plus the ABI check of the entry points tests/test_stream_ops_gpu.py calls and the launchers' refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import stream_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-12

NEW = {"ss_op_conv_gemm_rows": 6, "ss_op_dwconv_bn_silu_ex": 18, "ss_op_pool_dwconv": 16, "ss_op_pool_gather_rows": 10,
       "ss_op_pool_gather_ids": 9, "ss_op_pool_stack_rows": 8}


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


def test_launchers_refuse_without_touching_the_device():
    """Every refusal of the new launchers comes before any device call: a CPU-only machine sees them."""
    from streamspeech_amd import lib as L
    lib = L.load()
    dw = lambda K, nsess=1: lib.ss_op_pool_dwconv(None, None, None, 96, None, None, K, None, None, None, None, 1e-5, 256, None, nsess, 8)
    assert dw(30) == L.SS_ERR_ARG and dw(33) == L.SS_ERR_ARG and dw(0) == L.SS_ERR_ARG and dw(31, 0) == L.SS_ERR_ARG
    assert dw(31, -1) == L.SS_ERR_ARG
    rows = lambda W, nsess: lib.ss_op_pool_gather_rows(None, None, None, None, 96, W, None, None, nsess, 8)
    assert rows(256, 0) == L.SS_ERR_ARG and rows(128, 1) == L.SS_ERR_ARG and rows(256, -3) == L.SS_ERR_ARG
    assert lib.ss_op_pool_gather_ids(None, None, None, None, 96, None, None, 0, 8) == L.SS_ERR_ARG
    stack = lambda W, nsess=1: lib.ss_op_pool_stack_rows(None, None, None, W, None, None, nsess, 8)
    assert stack(254) == L.SS_ERR_ARG and stack(1028) == L.SS_ERR_ARG and stack(2048) == L.SS_ERR_ARG and stack(0) == L.SS_ERR_ARG
    assert stack(256, 0) == L.SS_ERR_ARG
    ex = lambda K, t_begin=0: lib.ss_op_dwconv_bn_silu_ex(None, None, 256, None, 256, None, K, None, None, None, None, 1e-5, 48, 256, 0,
                                                          None, 0, t_begin)
    assert ex(30) == L.SS_ERR_ARG and ex(33) == L.SS_ERR_ARG and ex(31, -1) == L.SS_ERR_ARG
    assert lib.ss_op_conv_gemm_rows(None, None, 0, None, None, 0) == L.SS_ERR_ARG
    a = L.SSOpConvArgs()
    assert lib.ss_op_conv_gemm_rows(None, C.byref(a), 0, None, None, 3) == L.SS_ERR_ARG


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).double()


def err(got, ref):
    return float(np.abs(np.asarray(got) - ref.numpy()).max())


# ---- the strided conv ------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 8, 16])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("T", [1, 5, 20, 43])
def test_chunk_conv_is_the_oracles_closed_form(chunk, stride, T):
    from oracle import streamspeech_oracle as O
    cin, n, k = 8, 64, 5
    x, w, b = rnd(T, cin, seed=1), rnd(n, cin, k, seed=2, scale=0.2), rnd(n, seed=3, scale=0.1)
    ref = O.chunk_causal_conv1d(x.t().contiguous(), w, b, stride, chunk if chunk else 999999).t()
    got = R.chunk_conv(x, w, b, stride=stride, pad=k // 2, chunk=chunk)
    assert got.shape == tuple(ref.shape) and err(got, ref) < BAR
    if chunk == 0:          # the unchunked case is the ordinary padded conv
        assert err(got, F.conv1d(x.t()[None], w, b, stride=stride, padding=k // 2)[0].t()) < BAR


@pytest.mark.parametrize("chunk", [0, 8, 16])
def test_chunk_conv_glu_is_glu_of_the_interleaved_weights(chunk):
    """GLU over [16 value | 16 gate] blocks of weights.glu_interleave == F.glu over [value ; gate] halves."""
    from oracle import streamspeech_oracle as O
    from streamspeech_amd.weights import glu_interleave
    T, cin, n, k = 37, 8, 96, 5
    x, w, b = rnd(T, cin, seed=4), rnd(n, cin, k, seed=5, scale=0.2), rnd(n, seed=6, scale=0.1)
    ref = F.glu(O.chunk_causal_conv1d(x.t().contiguous(), w, b, 2, chunk if chunk else 999999), dim=0).t()
    got = R.chunk_conv(x, glu_interleave(w), glu_interleave(b), stride=2, pad=2, chunk=chunk, glu=True)
    assert got.shape == (19, n // 2) and err(got, ref) < BAR


@pytest.mark.parametrize("m0", [0, 1, 7, 8, 9, 18])
def test_chunk_conv_row_range_is_the_same_rows(m0):
    T, cin, n, k = 37, 8, 32, 5
    x, w, b = rnd(T, cin, seed=7), rnd(n, cin, k, seed=8, scale=0.2), rnd(n, seed=9, scale=0.1)
    full = R.chunk_conv(x, w, b, stride=2, pad=2, chunk=8)
    part = R.chunk_conv(x, w, b, stride=2, pad=2, chunk=8, rows=(m0, 19))
    assert np.array_equal(part[m0:], full[m0:]) and np.isnan(part[:m0]).all() and np.isfinite(full).all()


# ---- the depthwise conv module -----------------------------------------------------------------------
def _dw_torch(x, w, chunk, mean, var, g, b, eps=1e-5):
    from oracle import streamspeech_oracle as O
    y = O.chunk_causal_conv1d(x.t().contiguous(), w[:, None, :], None, 1, chunk if chunk else 999999, groups=x.shape[1]).t()
    return F.silu((y - mean) / torch.sqrt(var + eps) * g + b)


def _bn(Cc, seed):
    return (rnd(Cc, seed=seed) * 0.1, torch.rand(Cc, generator=torch.Generator().manual_seed(seed + 1)).double() + 0.5,
            rnd(Cc, seed=seed + 2) * 0.1 + 1, rnd(Cc, seed=seed + 3) * 0.1)


@pytest.mark.parametrize("chunk", [0, 8, 16])
@pytest.mark.parametrize("K", [3, 15, 31])
@pytest.mark.parametrize("T", [1, 14, 33])
def test_dwconv_bn_silu_is_the_oracles_depthwise_conv(chunk, K, T):
    Cc = 6
    x, w, bn = rnd(T, Cc, seed=10), rnd(Cc, K, seed=11, scale=K ** -0.5), _bn(Cc, 12)
    got = R.dwconv_bn_silu(x, w, *bn, chunk=chunk)
    assert err(got, _dw_torch(x, w, chunk, *bn)) < BAR
    if chunk == 0:
        y = F.conv1d(x.t()[None], w[:, None, :], None, padding=K // 2, groups=Cc)[0].t()
        assert err(R.dwconv(x, w), y) < BAR
        assert err(got, F.silu(F.batch_norm(y, bn[0], bn[1], bn[2], bn[3], False, 0.0, 1e-5))) < BAR


def test_ragged_and_row_range_forms_are_each_utterance_alone():
    Cc, K = 6, 15
    lens = [1, 14, 33, 16]
    segs, at = [], 2
    for n in lens:
        segs.append((at, n))
        at += n
    x, w, bn = rnd(at + 3, Cc, seed=20), rnd(Cc, K, seed=21, scale=K ** -0.5), _bn(Cc, 22)
    for t_begin in (0, 1, 15):
        got = R.dwconv_bn_silu_ragged(x, segs, w, *bn, chunk=8, t_begin=t_begin)
        covered = np.zeros(x.shape[0], bool)
        for s, n in segs:
            if n > t_begin:
                covered[s + t_begin:s + n] = True
                assert err(got[s + t_begin:s + n], _dw_torch(x[s:s + n], w, 8, *bn)[t_begin:]) < BAR
        assert np.isnan(got[~covered]).all() and np.isfinite(got[covered]).all()


def test_pooled_form_is_the_conv_of_cache_rows_then_stacked_rows():
    Cc, K, slots, R_ = 6, 15, 4, 40
    cache = rnd(slots, R_, Cc, seed=30).numpy()
    gs = rnd(50, Cc, seed=31).numpy()
    w, bn = rnd(Cc, K, seed=32, scale=K ** -0.5), _bn(Cc, 33)
    sess = [(0, 9, 7, 16, 3, 8), (9, 33, 0, 33, 0, 0), (42, 1, 15, 16, 2, 16)]          # (q_start, n, r0, T, slot, chunk)
    y, after = R.pool_dwconv(gs, cache, sess, w, *bn)
    touched = np.zeros((slots, R_), bool)
    for q, n, r0, T, slot, chunk in sess:
        full = torch.from_numpy(np.concatenate([cache[slot][:r0], gs[q:q + n]]))
        assert err(y[q:q + n], _dw_torch(full, w, chunk, *bn)[r0:]) < BAR
        assert np.array_equal(after[slot][r0:T], gs[q:q + n])
        touched[slot, r0:T] = True
    assert np.array_equal(after[~touched], cache[~touched]) and np.isnan(y[43:]).all()


# ---- copies and LayerNorm ------------------------------------------------------------------------------
def test_gather_and_stack_are_exact_copies():
    cache = np.arange(3 * 6 * 2, dtype=np.int32).reshape(3, 6, 2)
    stk = -np.arange(1, 21, dtype=np.int32).reshape(10, 2)
    tab = [(5, 2, 4, 2, 0), (1, 1, 1, 0, 3), (4, 0, 4, 1, 3)]          # (len, k0, nf, slot, s_start)
    out, after = R.pool_gather(stk, cache, tab)
    assert out.dtype == np.int32 and out.shape == (10, 2)
    assert np.array_equal(out[:5], np.concatenate([cache[2][:2], stk[0:3]]))
    assert np.array_equal(out[5:6], cache[0][:1]) and np.array_equal(out[6:], stk[3:7])
    want = cache.copy()
    want[2][2:4] = stk[0:2]
    want[1][0:4] = stk[3:7]
    assert np.array_equal(after, want)
    enc = np.arange(40, dtype=np.float32).reshape(10, 4)
    got = R.pool_stack_rows(enc, [2, 9, 4], [0, 3, 4, 6])
    assert np.array_equal(got, enc[[2, 3, 4, 9, 4, 5]])


@pytest.mark.parametrize("D", [64, 96, 1024])
def test_layernorm_is_torch_layer_norm(D):
    x, g, b = rnd(7, D, seed=40) * 3 + 1, rnd(D, seed=41) * 0.1 + 1, rnd(D, seed=42) * 0.1
    assert err(R.layernorm(x, g, b), F.layer_norm(x, (D,), g, b, 1e-5)) < BAR
    x32 = R.layernorm(x.float(), g.float(), b.float(), dtype=np.float32)
    assert x32.dtype == np.float32 and err(x32.astype(np.float64), F.layer_norm(x, (D,), g, b, 1e-5)) < 1e-4
