"""CTC forced alignment on the GPU (csrc/ctc_align.hip): the two kernels through ss_op_ctc_align against tests/ctc_align_ref.py on the
cases the host twin passes in tests/test_ctc_align_cpu.py, then ss_batch_ctc_align on the seeded synthetic checkpoint.

Bounds (tests/ctc_align_ref.py: check): the per-frame values are within TOL = 2e-5 of the float64 log-softmax of the same float32
logits (the bound and the arithmetic of tests/test_ctc_scores_gpu.py), the state is float64, so
  |score - ref| <= T * 2e-5 + 1e-9 * max(1, |ref|);
  the path collapses to the labels and its float64 score is >= the reference's best - 2 * T * 2e-5 (ties and near-ties pass by score);
  |viterbi - that path's float64 score| <= T * 2e-5;
  tok_lprob is bit-equal to the sequential float32 sum of the kernel's own per-frame values along its path;
  an utterance alone, in a pack and in the reversed pack: memcmp-equal outputs."""
import numpy as np
import pytest
import torch

from tests import ctc_align_ref as R
from tests.test_ctc_align_cpu import PAD, _ragged, _run_checked, refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the two kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ld", [(64, 64), (257, 260), (6000, 6000)])
def test_op_small_cases(lib, V, ld):
    """(T, L) = (1, 0), (1, 1), (2, 2), (2, [a, a]) infeasible, (3, [a, a]) with its one path, T = L = 17, and 37 / 9 with repeats."""
    refs, recs = _run_checked(lib, R.small_cases(V, ld), V, gpu=True)
    assert [r["status"] for r in refs] == [0, 0, 0, 1, 0, 0, 0]
    assert recs[0]["path"].tolist() == [0] and recs[0]["score"] == recs[0]["viterbi"]
    assert recs[4]["path"].tolist() == [5, 0, 5]
    assert (recs[5]["path"] != 0).all()


def test_op_states_across_the_block(lib):
    """S = 255 / 257 / 259 and 601 states at T = 320: one, two and three passes of the 256-thread block; V = 64 / 257 (ld 260) / 6000."""
    for case in R.block_cases():
        V = 6000 if "6000" in case[0] else 257 if "257" in case[0] else 64
        _run_checked(lib, [case], V, gpu=True)


def test_op_ragged_pack_and_its_invariance(lib):
    """A pack of eight with an empty and an infeasible row in the middle; each utterance alone and the pack reversed: the same bits."""
    pack = _ragged()
    refs, recs = _run_checked(lib, pack, 64, gpu=True)
    assert [r["status"] for r in refs] == [0, 0, 0, 0, 1, 0, 0, 0]
    rc, rev = R.run(lib, [c[1:] for c in pack[::-1]], 64, pad=PAD, gpu=True)
    assert rc == 0
    for k, case in enumerate(pack):
        alone = R.run(lib, [case[1:]], 64, pad=PAD, gpu=True)[1][0]
        assert R.same_bits(alone, recs[k]) and R.same_bits(alone, rev[len(pack) - 1 - k]), case[0]


def test_op_nan_row_and_dead_label(lib):
    V = 64
    x = R.logits(50, 30, V)
    y = [7, 9, 9, 12]
    bad = x.copy()
    bad[11, 40] = np.nan
    dead = x.copy()
    dead[:, 9] = -np.inf
    refs, recs = _run_checked(lib, [("before", x, y), ("nan_row", bad, y), ("dead_label", dead, y), ("after", x, y)], V, gpu=True)
    assert [r["status"] for r in refs] == [0, 2, 1, 0]
    assert R.same_bits(recs[0], recs[3])


def test_op_follows_a_constructed_labelling(lib):
    x, y, frames = R.constructed()
    _, (rec,) = _run_checked(lib, [("constructed", x, y)], 64, gpu=True)
    assert rec["path"].tolist() == frames.tolist()
    runs = [t for t, v in enumerate(frames) if v != 0 and (t == 0 or frames[t - 1] != v)]
    ends = [t for t, v in enumerate(frames) if v != 0 and (t + 1 == len(frames) or frames[t + 1] != v)]
    assert rec["first"].tolist() == runs and rec["last"].tolist() == ends


def test_op_refusals_and_optional_outputs(lib):
    from streamspeech_amd import lib as L
    for cases, pad in refusals():
        if cases:
            assert R.run(lib, cases, 64, pad=pad, gpu=True)[0] == L.SS_ERR_ARG          # (run checks that nothing was written)
    x, y = R.logits(51, 12, 64), [4, 8]
    full = R.run(lib, [(x, y)], 64, pad=PAD, gpu=True)[1][0]
    rc, recs = R.run(lib, [(x, y)], 64, pad=PAD, gpu=True, want_path=False, want_frame=False)
    assert rc == 0 and recs[0]["first"].tolist() == full["first"].tolist() and recs[0]["tok_lprob"].tobytes() == full["tok_lprob"].tobytes()


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


@pytest.fixture(scope="module")
def encs(model):
    from streamspeech_amd import synth
    return [model.encoder_forward(torch.from_numpy(synth.synth_fbank(60 + k, T)).to(model.device), 16, 16)
            for k, T in enumerate((40, 133, 330))]


@pytest.fixture(scope="module")
def greedy(model, encs):
    """Per head the scored greedy search of the three utterances, one at a time."""
    return [[model.batch_ctc_greedy(hd, e.contiguous(), [e.shape[0]], return_raw=True, return_scores=True)[0] for e in encs]
            for hd in (0, 1)]


def _gemm_launches(lib):
    """GEMM-family launches of the process so far (the library's always-on census)."""
    import ctypes as C
    tot = 0
    for c in range(lib.ss_prof_num_classes()):
        n = C.c_int64(0)
        lib.ss_prof_totals(c, None, None, C.byref(n))
        tot += n.value
    return tot


def _same(a, b):
    return (np.array([a.score, a.viterbi_score]).tobytes() == np.array([b.score, b.viterbi_score]).tobytes() and a.status == b.status
            and a.path == b.path and a.first == b.first and a.last == b.last and np.array_equal(bits(a.tok_lprob), bits(b.tok_lprob)))


def test_model_aligns_the_greedy_tokens_onto_the_greedy_path(model, encs, greedy):
    """The labels are the greedy search's own collapsed tokens: its frame path is optimal for them (no path can use a larger
    per-frame value), so viterbi_score is the sum of the scored search's positional_scores within 2 * T' * 2e-5 (both sides hold
    the per-frame bound), and score >= viterbi_score."""
    cfg = model.cfg
    for hd in (0, 1):
        for enc, g in zip(encs, greedy[hd]):
            toks, lp, Tp = g[0], g[4], enc.shape[0]
            assert cfg.unk not in toks and cfg.pad not in toks    # the search masks both
            a = model.ctc_align(hd, enc, toks)
            assert a.status == 0 and len(a.path) == Tp and R.collapse(a.path) == toks
            want = float(np.asarray(lp, np.float64).sum())
            err = abs(a.viterbi_score - want)
            print(f"ss_batch_ctc_align head {hd} Tp {Tp} L {len(toks)}: |viterbi - greedy sum| = {err:.3e}  score - viterbi = "
                  f"{a.score - a.viterbi_score:.3e}")
            assert err <= 2 * Tp * R.TOL and a.score >= a.viterbi_score
            assert all(0 <= f <= l < Tp for f, l in zip(a.first, a.last)) and a.first == sorted(a.first)
            assert np.isfinite(a.tok_lprob).all() and (a.tok_lprob <= 0).all()


def test_model_pack_equals_the_single_calls(model, encs, greedy):
    Tp = [e.shape[0] for e in encs]
    for hd in (0, 1):
        labels = [g[0] for g in greedy[hd]]
        alone = [model.ctc_align(hd, e, y) for e, y in zip(encs, labels)]
        for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
            packed = torch.cat([encs[k] for k in order], 0).contiguous()
            got = model.batch_ctc_align(hd, packed, [Tp[k] for k in order], [labels[k] for k in order])
            for j, k in enumerate(order):
                assert _same(got[j], alone[k]), (hd, order, j)
        nop = model.batch_ctc_align(hd, encs[1].contiguous(), [Tp[1]], [labels[1]], want_path=False)[0]
        assert nop.path is None and nop.first == alone[1].first and np.array_equal(bits(nop.tok_lprob), bits(alone[1].tok_lprob))


def test_model_dropped_token_too_many_tokens_and_refusals(model, encs, greedy):
    from streamspeech_amd import lib as L
    enc, toks = encs[1], greedy[0][1][0]
    Tp, V = enc.shape[0], model.cfg.src_vocab
    assert len(toks) >= 2
    a = model.ctc_align(0, enc, toks[:1] + toks[2:])             # one token dropped: still aligns
    assert a.status == 0 and R.collapse(a.path) == toks[:1] + toks[2:]
    many = [5 + (j % 2) for j in range(Tp + 1)]                  # T' + 1 labels: infeasible
    b = model.ctc_align(0, enc, many)
    assert b.status == 1 and b.score == -np.inf and b.viterbi_score == -np.inf and set(b.path) == {-1} and set(b.first) == {-1}
    assert np.isnan(b.tok_lprob).all()
    e = model.ctc_align(0, enc, [])                              # no label: the all-blank path
    assert e.status == 0 and set(e.path) == {0} and e.score == e.viterbi_score and e.first == []
    g0 = _gemm_launches(model.lib)                               # the head GEMM is the call's first launch: the census sees it
    model.ctc_align(0, enc, toks)
    g1 = _gemm_launches(model.lib)
    assert g1 > g0
    for bad in ([0], [model.cfg.pad], [-1], [V], [5] * (L.CTC_ALIGN_MAX_LABELS + 1)):
        with pytest.raises(L.StreamSpeechHipError) as err:
            model.ctc_align(0, enc, bad)
        assert err.value.code == L.SS_ERR_ARG
    with pytest.raises(L.StreamSpeechHipError) as err:
        model.batch_ctc_align(2, enc.contiguous(), [Tp], [toks])
    assert err.value.code == L.SS_ERR_ARG
    with pytest.raises(L.StreamSpeechHipError) as err:
        model.batch_ctc_align(0, enc.contiguous(), [0], [[]])
    assert err.value.code == L.SS_ERR_ARG
    assert _gemm_launches(model.lib) == g1, "a refused call launched its head GEMM"
    again = model.ctc_align(0, enc, toks[:1] + toks[2:])         # the context is as usable as before
    assert _same(a, again)
