"""The references of tests/glue_ref.py against the torch expressions the kernels' comments cite (and the reference tree's
BeamSearch.step where that tree is present), plus the ABI check of the ss_op_* entry points tests/test_glue_ops_gpu.py calls."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import streamspeech_oracle as O
from tests import glue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["ss_op_masked_argmax", "ss_op_ctc_collapse", "ss_op_dur_predict", "ss_op_repeat_rows", "ss_op_embed_tokens",
       "ss_op_embed_tokens_rows", "ss_op_upsample_add_pos", "ss_op_gather_rows", "ss_op_scatter_rows", "ss_op_conv_post_tanh",
       "ss_op_conv_post_tanh_crop", "ss_op_beam_topk", "ss_op_beam_merge", "ss_op_beam_prefix_score", "ss_op_beam_prefix_chain"]


def test_abi_symbols_header_and_bindings():
    import ctypes as C
    from streamspeech_amd import lib as L
    lib = L.load()
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} has no prototype in the header"
        assert name in L.SIGNATURES
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header
    assert C.sizeof(L.SSOpBeamState) == 15 * C.sizeof(C.c_void_p)
    assert L.SS_OP_BEAM_CAND == R.CAND and "#define SS_OP_BEAM_CAND 64" in header


def test_masked_argmax_is_torch_max():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(40, 300, generator=g)
    x[0, 5] = x[0, 69] = 9.0                     # equal maxima: the lower index
    x[1] = 2.0                                   # all equal
    x[2, ::7] = float("nan")
    x[3] = float("nan")
    x[4] = float("-inf")
    x[5, 200] = x[5, 299] = float("inf")
    x[6, 17] = 50.0                              # the maximum under a mask
    masks = (17, 0, 123)
    y = x.clone()
    y[y != y] = float("-inf")
    y[:, list(masks)] = float("-inf")
    # torch.max over a row whose best value is -inf may answer a masked column; the kernels' rule there is the first unmasked one
    want = y.max(-1).indices.tolist()
    want[3] = want[4] = 1
    assert R.masked_argmax(x.numpy(), 300, masks).tolist() == want
    assert R.masked_argmax(x.numpy(), 300).tolist()[:3] == [5, 0, x[2].nan_to_num(float("-inf")).argmax().item()]
    assert R.masked_argmax(x.numpy(), 300, masks, force=7).tolist() == [7] * 40
    rml = np.array([2, 3, 4] * 14)[:40]
    got = R.masked_argmax(x.numpy(), 300, masks, row_max_len=rml, step=3, force_id=2)
    assert got.tolist() == [2 if rml[m] <= 3 else want[m] for m in range(40)]
    y2 = y.clone()
    y2[:, 0] = x[:, 0].nan_to_num(float("-inf"))     # ban_id replaces mask1 (column 0) on rows below their minimum
    y2[:, 6] = float("-inf")
    w2 = y2.max(-1).indices.tolist()
    got = R.masked_argmax(x.numpy(), 300, masks, row_min_len=rml, step=3, ban_id=6).tolist()
    assert [got[m] for m in range(5, 40)] == [w2[m] if rml[m] > 3 else want[m] for m in range(5, 40)]


@pytest.mark.parametrize("T", [1, 2, 64, 1025])
def test_ctc_collapse_is_the_oracles(T):
    for blank in (0, 9):
        ids = R.ctc_frames(T, 10, T + blank)
        tok, idx = R.ctc_collapse(ids, blank, 1)
        wt, wi = O.ctc_collapse(ids.tolist(), blank, 1)
        assert tok.tolist() == wt and idx.tolist() == wi
    assert R.ctc_collapse(np.zeros(T, int), 0, 1)[0].size == 0 and R.ctc_collapse(np.ones(T, int), 0, 1)[0].size == 0


@pytest.mark.parametrize("K", [1, 64, 65, 1024, 1025, 2500])
def test_dur_predict_is_clamp_round_exp_and_cumsum(K):
    x = R.dur_inputs(K, K)
    assert R.round_margin(x) >= 0.05 - 1e-4       # float32 expf (a few ulp of <= 302) cannot move a value across a boundary
    dur, cum = R.dur_predict(x)
    t = torch.from_numpy(x).double()
    want = torch.clamp(torch.round(torch.exp(t) - 1), min=1).long()
    assert dur.tolist() == want.tolist()
    assert cum.tolist() == [0] + torch.cumsum(want, 0).tolist()
    if K >= 64:
        assert dur[:4].tolist() == [1, 1, 1, 300]
    f = R.forced_durs(K, K)
    dur, cum = R.dur_predict(forced=f)
    assert dur.tolist() == f.tolist() and cum.tolist() == [0] + np.cumsum(f).tolist()


def test_repeat_rows_is_repeat_interleave_and_largest_k():
    for K in (1, 9, 65):
        d = R.forced_durs(K, K + 1)
        emb = np.random.default_rng(K).standard_normal((K, 3)).astype(np.float32)
        got = R.repeat_rows(emb, d)
        want = torch.repeat_interleave(torch.from_numpy(emb), torch.from_numpy(d), dim=0).numpy()
        assert np.array_equal(got, want)
        cum = R.dur_predict(forced=d)[1]
        for f in range(int(cum[-1])):              # the kernel's rule: the largest k < K with cum[k] <= f
            k = max(i for i in range(K) if cum[i] <= f)
            assert np.array_equal(got[f], emb[k])


def test_row_movers_are_torch_indexing():
    rng = np.random.default_rng(5)
    emb = torch.from_numpy(rng.integers(-1024, 1025, (50, 8)) / 256.0)
    pos = torch.from_numpy(rng.integers(-1024, 1025, (40, 8)) / 256.0)
    tok = np.array([4, 1, 7, -3, 50, 49, 1, 0])
    tk = torch.from_numpy(np.where((tok < 0) | (tok >= 50), 0, tok))
    for stride in (0, 1):
        p = torch.where(tk == 1, torch.tensor(1), 2 + stride * torch.arange(8))
        assert np.array_equal(R.embed_tokens(tok, emb, pos, 16.0, 2, stride, 1), (16.0 * emb[tk] + pos[p]).numpy())
    rp = np.array([0, 3, 37, 38, 90, 5, 6, 7])
    p = torch.where(tk == 1, torch.tensor(1), torch.clamp(2 + torch.from_numpy(rp), max=39))
    assert np.array_equal(R.embed_tokens(tok, emb, pos, 16.0, 2, 0, 1, row_pos=rp), (16.0 * emb[tk] + pos[p]).numpy())
    src = emb[:6].clone()
    src[2, 0] = 1.0
    want = src.repeat_interleave(3, 0) + torch.where(src.repeat_interleave(3, 0)[:, :1] != 1.0, pos[3][None], torch.tensor(0.0))
    assert np.array_equal(R.upsample_add_pos(src, 3, pos[3], 1.0), want.numpy())
    assert np.array_equal(R.gather_rows(tok, emb.numpy()), emb[tk].numpy())
    dst = np.full((6, 10), np.nan)
    rows = np.array([5, -1, 2, 6, 0])
    got = R.scatter_rows(rows, emb.numpy(), dst, 8)
    want = torch.full((6, 10), float("nan"), dtype=torch.float64)
    want[torch.tensor([5, 2, 0]), :8] = emb[torch.tensor([0, 2, 4])]
    assert np.array_equal(got, want.numpy(), equal_nan=True)


@pytest.mark.parametrize("T,C", [(1, 16), (5, 32), (300, 16)])
def test_conv_post_tanh_is_torch_conv1d(T, C):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, C, generator=g, dtype=torch.float64)
    w = torch.randn(7, C, generator=g, dtype=torch.float64) * (7 * C) ** -0.5
    a = torch.nn.functional.leaky_relu(x, 0.01).t()[None]
    want = torch.tanh(torch.nn.functional.conv1d(a, w.t()[None], torch.tensor([0.1], dtype=torch.float64), padding=3))[0, 0]
    assert np.max(np.abs(R.conv_post_tanh(x, w, 0.1) - want.numpy())) < 1e-14


def _beam_case(V, k, seed):
    rng = np.random.default_rng(seed)
    logits = (rng.integers(-32, 33, (3 * k, V)) / 8.0).astype(np.float32)
    cum = (rng.integers(-40, 1, 3 * k) / 8.0).astype(np.float32)
    return logits, cum


@pytest.mark.parametrize("V,k,step", [(11, 5, 0), (300, 2, 0), (300, 5, 3), (300, 5, 9), (65, 32, 2)])
def test_beam_topk_is_log_softmax_masks_topk(V, k, step):
    """The per-row lists merged (glue_ref.beam_merge's order) are torch.topk over the flattened beam x vocabulary of the masked
    log-softmax + cumulative score, and BeamSearch.step of the reference tree where it is present."""
    pad, unk, eos, pen, min_len, max_len = 1, 3, 2, 0.5625, 2, 9
    logits, cum = _beam_case(V, k, V + k + step)
    logits[0, 7] = np.nan
    B = 3
    lists = R.beam_topk(logits, k, step, min_len, [max_len] * B, [0] * B, [0] * B, cum, pad, unk, eos, pen)
    lp = torch.log_softmax(torch.from_numpy(logits).double(), -1)
    lp[lp != lp] = float("-inf")
    lp[:, pad] = float("-inf")
    lp[:, unk] -= pen
    if step >= max_len:
        lp[:, :eos] = float("-inf")
        lp[:, eos + 1:] = float("-inf")
    if step < min_len:
        lp[:, eos] = float("-inf")
    lp = lp.view(B, k, V)
    scores = torch.zeros(B, k, max(step, 1), dtype=torch.float64)
    scores[:, :, step - 1] = torch.from_numpy(cum).double().view(B, k)
    flat = (lp[:, :1] if step == 0 else lp + scores[:, :, step - 1].unsqueeze(-1)).reshape(B, -1)
    n = min(2 * k, flat.size(1) - 1)
    top = torch.topk(flat, n)
    step_ref = None
    try:
        from oracle import ref_loader
        if ref_loader.available():
            ref_loader._mod("fairseq.token_generation_constraints")
            step_ref = ref_loader._load_file("fairseq.search", "fairseq/fairseq/search.py").BeamSearch.step
    except Exception:          # the tree is optional: without it the torch expression above is the whole check
        step_ref = None
    for b in range(B):
        nl = 1 if step == 0 else k
        sc = np.concatenate([lists[b * k + l][0] for l in range(nl)])
        tk = np.concatenate([lists[b * k + l][1] for l in range(nl)])
        bm = np.repeat(np.arange(nl), len(lists[b * k][0]))
        o = R.order(sc, bm * V + tk)[:n]
        assert np.allclose(sc[o], top.values[b].numpy(), rtol=0, atol=1e-12)   # float64 both; -inf equals -inf
        fin = np.isfinite(sc[o])
        # ids: wherever the score is held by one candidate only (torch.topk leaves the order of equal scores open)
        uniq = np.array([fin[i] and np.sum(np.abs(flat[b].numpy() - sc[o][i]) < 1e-9) == 1 for i in range(n)])
        assert np.array_equal((bm[o] * V + tk[o])[uniq], top.indices[b].numpy()[uniq])
        assert np.allclose(flat[b].numpy()[bm[o] * V + tk[o]], sc[o], rtol=0, atol=1e-12)   # every id holds the score listed with it
        key = list(zip(-sc[o], bm[o] * V + tk[o]))
        assert key == sorted(key)
    if step_ref is not None:
        class Dummy:
            pass
        s_buf, i_buf, b_buf = step_ref(Dummy(), step, lp, scores if step > 0 else None)
        assert np.array_equal(s_buf.numpy(), top.values.numpy())
        assert np.array_equal((b_buf * V + i_buf).long().numpy(), top.indices.numpy())


def test_beam_prefix_refs():
    logits, _ = _beam_case(300, 2, 3)
    logits[4, 9] = np.nan
    ftok = np.array([5, -1, 1, 3, 8, 299])
    lp = R.beam_prefix_score(logits, ftok, 1, 3, 0.5)
    t = torch.log_softmax(torch.from_numpy(logits).double(), -1)
    assert lp[0] == t[0, 5].item() and np.isnan(lp[1]) and lp[2] == -np.inf and lp[3] == t[3, 3].item() - 0.5
    assert lp[4] == -np.inf and lp[5] == t[5, 299].item()
    lp32 = np.array([-1.25, -0.1, -2.3, -0.7, -3.9, -0.01], np.float32)
    cum0, pos = R.beam_prefix_chain(lp32, [0, 1, 1], [1, 0, 4], 2, np.full(6, np.nan), np.full(6, np.nan))
    c = torch.cumsum(torch.from_numpy(lp32[1:5]), 0)                          # float32, in order
    assert cum0[0] == lp32[0] and np.isnan(cum0[1:4]).all() and cum0[4] == c[3].item() and np.isnan(cum0[5])
    assert pos[0] == lp32[0] and pos[1] == lp32[1] and np.isnan(pos[5])
    assert np.array_equal(pos[2:5], (c[1:] - c[:-1]).numpy())


def test_beam_merge_ref_on_a_hand_worked_step():
    """k = 2, one utterance, lock-step index 1: the lists merge to (7 | </s> from beam 0 | </s> from beam 1 | 3); the first </s> is
    finalised, the second one (past the first k) is only skipped, the hypotheses go on with 7 and 3."""
    k, Lc, V, eos = 2, 4, 10, 2
    nan = np.float32("nan")
    st = dict(
        tok=np.array([[2, 2], [5, 6], [-7, -7]]), cum=np.array([[0, 0], [-1, -2], [nan, nan]], np.float32),
        anc=np.array([[[-7] * 4] * 2, [[0, 0, -7, -7], [0, 1, -7, -7]]]),
        cand_s=np.full((2, R.CAND), nan, np.float32), cand_t=np.full((2, R.CAND), -7),
        ignore=np.zeros(2, int), done=np.zeros(1, int), max_len=np.array([9]), npre=np.zeros(1, int), fin_cnt=np.zeros(1, int),
        fin_score=np.full((1, 2), nan, np.float32), fin_len=np.full((1, 2), -7), fin_tok=np.full((1, 2, Lc), -7),
        fin_pos=np.full((1, 2, Lc), nan, np.float32), fin_anc=np.full((1, 2, Lc), -7))
    st["cand_s"][0, :4], st["cand_t"][0, :4] = [-1.5, -2.0, -2.5, -3.0], [7, 2, 4, 8]
    st["cand_s"][1, :4], st["cand_t"][1, :4] = [-2.0, -2.25, -3.5, -4.0], [2, 3, 9, 5]
    for normalize, score in ((0, -2.0), (1, -1.0)):
        s = R.beam_merge(st, 1, k, Lc, V, 1, 0, eos, normalize)
        assert s["tok"][2].tolist() == [7, 3] and s["cum"][2].tolist() == [-1.5, -2.25]
        assert s["anc"][0].tolist() == [[0, 0, 0, -7], [0, 1, 1, -7]] and np.array_equal(s["anc"][1], st["anc"][1])
        assert s["ignore"].tolist() == [0, 0] and s["done"].tolist() == [0] and s["fin_cnt"].tolist() == [1]
        assert s["fin_score"][0, 0] == score and np.isnan(s["fin_score"][0, 1]) and s["fin_len"][0].tolist() == [2, -7]
        assert s["fin_tok"][0].tolist() == [[5, 2, -7, -7], [-7] * 4] and s["fin_anc"][0].tolist() == [[0, 0, -7, -7], [-7] * 4]
        assert s["fin_pos"][0, 0, :2].tolist() == [-1.0, -1.0] and np.isnan(s["fin_pos"][0, 0, 2:]).all()
    st["fin_cnt"][0] = 1                     # one entry short of full: the step fills the table and ends the utterance
    s = R.beam_merge(st, 1, k, Lc, V, 1, 0, eos, 0)
    assert s["done"].tolist() == [1] and s["fin_cnt"].tolist() == [2] and s["fin_len"][0].tolist() == [-7, 2]
    assert s["tok"][2].tolist() == [eos, eos] and s["cum"][2].tolist() == [0, 0]
    assert s["anc"][0].tolist() == [[0, 0, 0, -7], [0, 1, 1, -7]]
