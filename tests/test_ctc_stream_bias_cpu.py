"""The resumable CTC prefix beam search with a hotword set, without a device: the host twin (ss_ctc_stream_advance_host on an
object of ss_debug_ctc_stream_create_bias) against the ONE-SHOT twin (ss_ctc_beam_bias_host, which tests/test_ctc_beam_bias_cpu.py
pins to the Python reference and to brute force), byte for byte: however an utterance's frames are cut into calls, the last
call's records are the one-shot search's on all frames with the finish (and eos) term, and every other call's are the one-shot
search's on the frames so far without them; the stable prefix never shrinks and is a prefix of every later best hypothesis.  Plus
slot reuse and the refusals.  BiasStream and the check_* functions run again on the kernels in tests/test_ctc_stream_bias_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from tests import ctc_beam_ref as R
from tests import ctc_bias_ref as RB
from tests.ctc_beam_ref import G, SENT
from tests.ctc_stream_ref import PART, common_prefix
from tests.test_ctc_beam_bias_cpu import BIAS_SCALES, LM_W, small_set
from tests.test_ctc_beam_cpu import PAD, SHAPES, UNK, small_case
from tests.test_ctc_beam_lm_cpu import small_lm


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


@pytest.fixture(scope="module")
def objs():
    """Per V of the small shapes: (hotword set, model)."""
    from streamspeech_amd.hotwords import CtcBias
    from streamspeech_amd.ngram import NgramLM
    out = {V: (CtcBias(*small_set(V), V, PAD, UNK), NgramLM(small_lm(V)[0])) for V in sorted({s[1] for s in SHAPES})}
    yield out
    for b, lm in out.values():
        b.close()
        lm.close()


class BiasStream:
    """An ss_ctc_stream of ss_debug_ctc_stream_create_bias: host memory and ss_ctc_stream_advance_host, or (gpu) device memory
    and ss_op_ctc_stream_advance.  bias / lm: the library's handles or None; bopts: (scale, finish) or None; lopts: (lm_weight,
    word_score, eos_term) or None."""

    def __init__(self, lib, V, pad, unk, S, max_frames, beam, cand, nbest, bias, bopts, lm=None, lopts=None, gpu=False):
        from streamspeech_amd.lib import SSCtcBiasOpts, SSCtcLmOpts
        self.lib, self.V, self.nbest, self.gpu = lib, V, nbest, gpu
        self.h = C.c_void_p()
        lo = C.byref(SSCtcLmOpts(lopts[0], lopts[1], int(lopts[2]))) if lopts is not None else None
        bo = C.byref(SSCtcBiasOpts(bopts[0], int(bopts[1]), 0)) if bopts is not None else None
        self.rc = lib.ss_debug_ctc_stream_create_bias(V, pad, unk, int(gpu), S, max_frames, beam, cand, nbest, lm, lo, bias, bo,
                                                      C.byref(self.h))
        assert (self.rc == 0) == bool(self.h.value)

    def reset(self, slot):
        return self.lib.ss_ctc_stream_reset(self.h, slot)

    def close(self):
        if self.h.value:
            self.lib.ss_ctc_stream_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def advance(self, slots, rows, upto, final, out_stride=None):
        """rows: per session its NEW rows [k, ld] float32 (k may be 0) -> (rc, records); a record is dict(labels [tuple] of its
        status-0 slots, status, raw, part (frames, n_stable, n_alive, status), part_raw).  Guards and sentinels as
        tests/ctc_beam_ref.py:run."""
        B = len(slots)
        ld = rows[0].shape[1] if rows else self.V
        x = np.ascontiguousarray(np.concatenate(list(rows) + [np.zeros((1, ld), np.float32)], 0), np.float32)
        stride = max(list(upto) + [1]) if out_stride is None else out_stride
        nb = self.nbest
        hyp = np.zeros(max(B, 1) * nb + G, RB.BHYP)
        hyp["status"] = SENT
        toks = np.full(max(B, 1) * nb * max(stride, 1) + G, SENT, np.int32)
        part = np.full((max(B, 1) + G) * 4, SENT, np.int32).view(PART)
        bufs = [hyp, toks, part]
        ar = lambda v: (C.c_int32 * max(len(v), 1))(*[int(a) for a in v])  # noqa: E731
        if self.gpu:
            import torch
            dx = torch.from_numpy(x).cuda()
            dev = [torch.from_numpy(b.view(np.uint8).copy()).cuda() for b in bufs]
            ptr = [C.c_void_p(d.data_ptr()) for d in dev]
            rc = self.lib.ss_op_ctc_stream_advance(C.c_void_p(torch.cuda.current_stream().cuda_stream), self.h, B, ar(slots),
                                                   C.c_void_p(dx.data_ptr()), ld, ar(upto), ar(final), ptr[0], ptr[1], stride, ptr[2])
            torch.cuda.synchronize()
            bufs = [d.cpu().numpy().view(b.dtype) for d, b in zip(dev, bufs)]
        else:
            ptr = [C.c_void_p(b.ctypes.data) for b in bufs]
            rc = self.lib.ss_ctc_stream_advance_host(self.h, B, ar(slots), C.c_void_p(x.ctypes.data), ld, ar(upto), ar(final), ptr[0],
                                                     ptr[1], stride, ptr[2])
        hyp, toks, part = bufs
        if rc != 0:                                                # a refusal writes nothing
            assert (hyp["status"] == SENT).all() and (toks == SENT).all() and (part.view(np.int32) == SENT).all()
            return rc, None
        assert (hyp["status"][B * nb:] == SENT).all() and (toks[B * nb * stride:] == SENT).all(), "wrote behind the last entry"
        assert (part.view(np.int32)[4 * B:] == SENT).all(), "wrote behind the last entry"
        out = []
        for b in range(B):
            h = hyp[b * nb:(b + 1) * nb]
            tr = toks[b * nb * stride:(b + 1) * nb * stride].reshape(nb, stride)
            for k in range(nb):
                m = int(h["n_tokens"][k])
                assert 0 <= m <= upto[b] and (tr[k, m:] == SENT).all(), "entries past n_tokens were touched"
            p = part[b]
            out.append({"labels": [tuple(int(v) for v in tr[k, :int(h["n_tokens"][k])]) for k in range(nb) if h["status"][k] == 0],
                        "status": h["status"].tolist(),
                        "raw": h.tobytes() + b"".join(tr[k, :int(h["n_tokens"][k])].tobytes() for k in range(nb)),
                        "part": tuple(int(p[k]) for k in PART.names), "part_raw": p.tobytes()})
        return rc, out


def one_shot(lib, x, V, beam, cand, nbest, bias, scale, lm, final, gpu=False):
    """The oracle: the one-shot search on these frames, the finish and eos terms only where the call is the utterance's last."""
    rc, recs = RB.run(lib, [x], V, PAD, UNK, beam, cand, nbest, bias.h, scale, final, None if lm is None else lm.h, *LM_W, final,
                      gpu=gpu, want_den=False)
    assert rc == 0
    return recs[0]


def check_stream(lib, x, V, beam, cand, cuts, bias, scale, lm=None, gpu=False, cache=None, nbest=None):
    """One utterance through a one-slot object in the calls (cuts ..., T): every property of the module docstring."""
    T = x.shape[0]
    nbest = beam if nbest is None else nbest
    cache = {} if cache is None else cache
    lh, lo = (None, None) if lm is None else (lm.h, (LM_W[0], LM_W[1], 1))
    with BiasStream(lib, V, PAD, UNK, 1, T, beam, cand, nbest, bias.h, (scale, 1), lh, lo, gpu=gpu) as st:
        assert st.rc == 0
        f, stable, stable_tokens = 0, 0, ()
        for t in list(cuts) + [T]:
            final = t == T
            rc, recs = st.advance([0], [x[f:t]], [t], [final])
            assert rc == 0
            rec = recs[0]
            frames, n_stable, n_alive, status = rec["part"]
            assert (frames, status) == (t, 0)
            if t == 0:                                         # nothing consumed: the empty string alone
                assert rec["labels"] == [()] and (n_stable, n_alive) == (0, 1)
                continue
            if (t, final) not in cache:
                cache[(t, final)] = one_shot(lib, x[:t], V, beam, cand, nbest, bias, scale, lm, final, gpu=gpu)
            want = cache[(t, final)]
            assert rec["raw"] == want["raw"], (t, final, rec["labels"], want["hyps"])
            if nbest == beam:                                  # the records show the whole beam
                assert n_alive == len(want["hyps"]) and n_stable == common_prefix(h[0] for h in want["hyps"]), (t, rec["part"])
            assert n_stable >= stable, "n_stable went down"
            assert all(y[:stable] == stable_tokens for y in rec["labels"]), "a stable token changed"
            stable = n_stable
            stable_tokens = rec["labels"][0][:stable] if rec["labels"] else stable_tokens
            f = t
        rc, again = st.advance([0], [x], [T], [1])             # the final call reset the slot: the utterance again, the same bytes
        assert rc == 0 and again[0]["raw"] == rec["raw"] and again[0]["part_raw"] == rec["part_raw"]


def check_every_split(lib, objs, gpu=False, seeds=range(6)):
    """The (12, 6, 4, 3) cases at logit scale 2, both bias scales, bias alone and with the model: every single cut, and three
    double cuts with a call without rows."""
    shape = SHAPES[0]
    T, V, beam, cand = shape
    bias, lm = objs[V]
    n = 0
    for seed in seeds:
        x = small_case(shape, 2, seed)
        for scale in BIAS_SCALES:
            for m in (None, lm):
                cache = {}
                for cuts in [[c] for c in range(1, T)] + [[0, 5], [3, 3, 4], [6, 11]]:
                    check_stream(lib, x, V, beam, cand, cuts, bias, scale, m, gpu, cache)
                    n += 1
    return n


def test_host_every_split_is_the_one_shot_twin(lib, objs):
    n = check_every_split(lib, objs)
    print(f"ctc_stream bias: {n} streams, every call memcmp-equal to the one-shot twin")


def test_host_finish_term_only_in_the_last_call(lib):
    """Forced logits that stand inside the phrase 4 5 6 after three frames and complete it in the fifth: the non-final call reports
    the credit still lent (bias_score 4), the final call of the same frames takes it off, and the completed phrase keeps all 6."""
    from streamspeech_amd.hotwords import CtcBias
    from tests.test_ctc_beam_bias_cpu import forced
    V = 8
    x = forced(V, [4, 0, 5, 0, 6])
    with CtcBias([[4, 5, 6]], [2.0], V, PAD, UNK) as bias:
        for final3, want3 in ((0, 4.0), (1, 0.0)):
            with BiasStream(lib, V, PAD, UNK, 1, 5, 4, 3, 4, bias.h, (0.5, 1)) as st:
                rc, recs = st.advance([0], [x[:3]], [3], [final3])
                assert rc == 0 and recs[0]["labels"][0] == (4, 5)
                assert np.frombuffer(recs[0]["raw"][:40], RB.BHYP)["bias_score"][0] == want3
                if not final3:
                    rc, recs = st.advance([0], [x[3:]], [5], [1])
                    assert rc == 0 and recs[0]["labels"][0] == (4, 5, 6)
                    assert np.frombuffer(recs[0]["raw"][:40], RB.BHYP)["bias_score"][0] == 6.0


def check_slot_reuse(lib, objs, with_lm, gpu=False):
    """A slot after a final call, and after a reset in the middle of an utterance, gives a fresh object's bytes."""
    shape = SHAPES[2]
    T, V, beam, cand = shape
    bias, lm = objs[V]
    lh, lo = (lm.h, (LM_W[0], LM_W[1], 1)) if with_lm else (None, None)
    a, b = small_case(shape, 6, 40), small_case(shape, 2, 41)
    mk = lambda: BiasStream(lib, V, PAD, UNK, 2, T, beam, cand, beam, bias.h, (1.0, 1), lh, lo, gpu=gpu)  # noqa: E731

    def utter(st, slot, x, cuts=(13, 14)):
        out, f = [], 0
        for t in list(cuts) + [T]:
            rc, recs = st.advance([slot], [x[f:t]], [t], [t == T])
            assert rc == 0
            out.append(recs[0]["raw"] + recs[0]["part_raw"])
            f = t
        return out

    with mk() as fresh:
        want = utter(fresh, 1, b)
    with mk() as st:
        utter(st, 1, a)                                        # T = max_frames frames, then the final call's reset
        assert utter(st, 1, b) == want
        rc, _ = st.advance([1], [a[:25]], [25], [0])           # an utterance abandoned after 25 frames
        assert rc == 0 and st.reset(1) == 0
        assert utter(st, 1, b) == want
        assert st.reset(2) != 0 and st.reset(-1) != 0
    assert want[-1].startswith(one_shot(lib, b, V, beam, cand, beam, bias, 1.0, lm if with_lm else None, True, gpu=gpu)["raw"])


def test_host_slot_reuse(lib, objs):
    check_slot_reuse(lib, objs, False)
    check_slot_reuse(lib, objs, True)


def check_sessions_in_one_call(lib, objs, with_lm, gpu=False):
    """Three sessions with different splits in every call, on other slots than their order: each call's bytes of a session are
    the one-shot twin's on its frames so far."""
    shape = SHAPES[2]
    T, V, beam, cand = shape
    bias, lm = objs[V]
    lh, lo = (lm.h, (LM_W[0], LM_W[1], 1)) if with_lm else (None, None)
    xs = [small_case(shape, 6, 50), small_case(shape, 2, 51)[:23], small_case(shape, 6, 52)[:1]]
    upto = [[9, 9, 40], [1, 20, 23], [1, 1, 1]]
    with BiasStream(lib, V, PAD, UNK, 4, T, beam, cand, 5, bias.h, (1.0, 1), lh, lo, gpu=gpu) as st:
        f = [0, 0, 0]
        for j in range(3):
            rc, recs = st.advance([3, 0, 2], [xs[k][f[k]:upto[k][j]] for k in range(3)], [upto[k][j] for k in range(3)], [j == 2] * 3)
            assert rc == 0
            for k, rec in enumerate(recs):
                want = one_shot(lib, xs[k][:upto[k][j]], V, beam, cand, 5, bias, 1.0, lm if with_lm else None, j == 2, gpu=gpu)
                assert rec["raw"] == want["raw"] and rec["part"][0] == upto[k][j], (k, j)
                f[k] = upto[k][j]


def test_host_sessions_in_one_call(lib, objs):
    check_sessions_in_one_call(lib, objs, False)
    check_sessions_in_one_call(lib, objs, True)


def test_host_create_refusals(lib, objs):
    """The plain object's refusals, and the set's: a NULL set or options, a set of another V / pad / unk, a non-finite scale, a
    model without options or options without a model; an object without a set still writes its own records."""
    from streamspeech_amd import lib as L
    bias, lm = objs[64]
    mk = lambda V=64, pad=PAD, unk=UNK, b=bias.h, bo=(1.0, 1), lh=None, lo=None, **kw: BiasStream(  # noqa: E731
        lib, V, pad, unk, kw.get("S", 2), kw.get("max_frames", 40), kw.get("beam", 4), kw.get("cand", 4), kw.get("nbest", 2), b, bo, lh, lo)
    for kw in (dict(S=0), dict(max_frames=0), dict(max_frames=L.CTC_BEAM_MAX_FRAMES + 1), dict(beam=0), dict(beam=33), dict(cand=0),
               dict(cand=33), dict(nbest=0), dict(nbest=5)):
        assert mk(**kw).rc == L.SS_ERR_ARG, kw
    assert mk(b=None).rc == L.SS_ERR_ARG and mk(bo=None).rc == L.SS_ERR_ARG
    assert mk(V=63).rc == L.SS_ERR_ARG and mk(pad=5).rc == L.SS_ERR_ARG and mk(unk=-1).rc == L.SS_ERR_ARG
    for s in (np.nan, np.inf):
        assert mk(bo=(s, 1)).rc == L.SS_ERR_ARG
    assert mk(lh=lm.h).rc == L.SS_ERR_ARG and mk(lo=(0.5, 0.0, 1)).rc == L.SS_ERR_ARG
    assert mk(lh=lm.h, lo=(np.nan, 0.0, 1)).rc == L.SS_ERR_ARG
    assert lib.ss_debug_ctc_stream_create_bias(64, PAD, UNK, 0, 2, 40, 4, 4, 2, None, None, bias.h, None, None) == L.SS_ERR_ARG
    for st in (mk(), mk(lh=lm.h, lo=(0.5, 0.0, 1))):
        with st:
            assert st.rc == 0
            x = R.scaled_logits(3, 6, 64, 6)
            assert st.advance([0, 0], [x[:3], x[:3]], [3, 3], [0, 0])[0] == L.SS_ERR_ARG     # a slot twice
            assert st.advance([0], [x], [6], [0], out_stride=5)[0] == L.SS_ERR_ARG           # out_stride below upto
            assert st.advance([0], [x[:, :63].copy()], [6], [0])[0] == L.SS_ERR_ARG          # ld < V
            assert st.advance([0], [x], [6], [1])[0] == 0
