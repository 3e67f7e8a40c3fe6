"""The resumable CTC prefix beam search without a device: the host twin (ss_ctc_stream_advance_host on an object of
ss_debug_ctc_stream_create) against the ONE-SHOT twins (ss_ctc_beam_host / ss_ctc_beam_lm_host, which tests/test_ctc_beam_cpu.py and
tests/test_ctc_beam_lm_cpu.py pin to the Python reference and to brute force), byte for byte: however an utterance's frames are cut
into calls, the last call's records are the one-shot search's on all frames and every other call's are the one-shot search's on the
frames so far; n_stable is the common prefix of that search's beam, never shrinks, and what it covers never changes.  Plus a mutant
that forgets the child table across a cut, slots (packs, reuse), every refusal, and the Python layers that need no device.  The
check_* functions run again on the kernels in tests/test_ctc_stream_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import ctc_beam_lm_ref as RL
from tests import ctc_beam_ref as R
from tests import ctc_stream_ref as S
from tests.test_ctc_beam_cpu import PAD, SCALES, SHAPES, UNK, ragged_pack, small_case
from tests.test_ctc_beam_lm_cpu import small_lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHTS = ((0.5, 0.0), (1.0, -0.5))
FORGET_CASE = ((12, 6, 4, 3), 2, 0, 1)                        # (shape, logit scale, seed, cut): where forgetting the table shows


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


@pytest.fixture(scope="module")
def lms():
    from streamspeech_amd.ngram import NgramLM
    out = {V: NgramLM(small_lm(V)[0]) for V in sorted({s[1] for s in SHAPES})}
    yield out
    for lm in out.values():
        lm.close()


# ---- the oracle: the one-shot search on the first t frames -------------------------------------------------------------------------
def one_shot(lib, x, V, beam, cand, nbest, lm=None, w=None, eos=True, gpu=False):
    if lm is None:
        rc, recs = R.run(lib, [x], V, PAD, UNK, beam, cand, nbest, gpu=gpu, want_den=False)
    else:
        rc, recs = RL.run(lib, [x], V, PAD, UNK, beam, cand, nbest, lm.h, w[0], w[1], eos, gpu=gpu, want_den=False)
    assert rc == 0
    return recs[0]


def splits_of(T, seed):
    """Cut points of a seeded multi-cut split of T frames: four distinct cuts, one of them followed by a one-frame call and one
    repeated (a call with no rows), and a one-frame call at the start for odd seeds."""
    rng = np.random.default_rng(1000 + seed)
    cuts = sorted(int(c) for c in rng.choice(np.arange(2, T - 1), 4, replace=False))
    cuts += [cuts[1] + 1, cuts[2]] + ([1] if seed & 1 else [])
    return sorted(cuts)


def check_stream(lib, x, V, beam, cand, cuts, lm=None, w=None, gpu=False, cache=None, nbest=None, max_frames=None):
    """One utterance through a one-slot object in the calls (cuts ..., T): every property of the module docstring.  cache: the
    one-shot records per (t, final) of this utterance and form."""
    T = x.shape[0]
    nbest = beam if nbest is None else nbest
    cache = {} if cache is None else cache
    opts = None if lm is None else (w[0], w[1], 1)

    def oracle(t, final):
        if (t, final) not in cache:
            cache[(t, final)] = one_shot(lib, x[:t], V, beam, cand, nbest, lm, w, eos=final, gpu=gpu)
        return cache[(t, final)]

    with S.Stream(lib, V, PAD, UNK, 1, max_frames or T, beam, cand, nbest, None if lm is None else lm.h, opts, gpu=gpu) as st:
        assert st.rc == 0
        f, stable, stable_tokens = 0, 0, ()
        for t in list(cuts) + [T]:
            final = t == T
            rc, recs = st.advance([0], [x[f:t]], [t], [final])
            assert rc == 0
            rec = recs[0]
            frames, n_stable, n_alive, status = rec["part"]
            assert (frames, status) == (t, 0)
            if t == 0:
                assert [h[0] for h in rec["hyps"]] == [()] and rec["hyps"][0][1] == 0.0 and (n_stable, n_alive) == (0, 1)
            else:
                want = oracle(t, final)
                assert rec["raw"] == want["raw"], (t, final, rec["hyps"], want["hyps"])
                if nbest == beam:                              # the records show the whole beam
                    assert n_alive == len(want["hyps"]) and n_stable == S.common_prefix(h[0] for h in want["hyps"]), (t, rec["part"])
            assert n_stable >= stable, "n_stable went down"
            assert all(h[0][:stable] == stable_tokens for h in rec["hyps"]), "a stable token changed"
            stable = n_stable
            stable_tokens = rec["hyps"][0][0][:stable] if rec["hyps"] else stable_tokens
            f = t
        # the final call reset the slot: the same utterance again gives the same bytes
        rc, again = st.advance([0], [x], [T], [1])
        assert rc == 0 and again[0]["raw"] == rec["raw"] and again[0]["part_raw"] == rec["part_raw"]


def forms(lms, V):
    return [(None, None)] + [(lms[V], w) for w in WEIGHTS]


def check_split_invariance(lib, lms, shape, scale, gpu=False, seeds=range(10)):
    T, V, beam, cand = shape
    n = 0
    for seed in seeds:
        x = small_case(shape, scale, seed)
        for lm, w in forms(lms, V):
            cache = {}
            if T <= 12:
                for c in range(1, T):
                    check_stream(lib, x, V, beam, cand, [c], lm, w, gpu, cache)
                    n += 1
            else:
                for k in range(8):
                    check_stream(lib, x, V, beam, cand, splits_of(T, 8 * seed + k), lm, w, gpu, cache)
                    n += 1
    return n


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_stream_entry_points_are_declared_and_bound(lib):
    from streamspeech_amd import lib as L
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in (("ss_ctc_stream_create", 10), ("ss_ctc_stream_destroy", 1), ("ss_ctc_stream_reset", 2),
                        ("ss_ctc_stream_advance", 13), ("ss_ctc_stream_advance_host", 11), ("ss_debug_ctc_stream_create", 12),
                        ("ss_op_ctc_stream_advance", 12)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"
    assert lib.ss_abi_version() == 2
    assert C.sizeof(L.SSCtcStreamPart) == S.PART.itemsize == 16
    assert [f[0] for f in L.SSCtcStreamPart._fields_] == list(S.PART.names)


# ---- split invariance, partials, the stable prefix ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("shape", SHAPES)
def test_host_split_invariance_and_partials(lib, lms, shape, scale):
    """Seeds 0-9, plain and with the small model at both weight pairs: every single cut of the T = 12 shapes, eight seeded multi-cut
    splits of T = 40 (a call without rows and one-frame calls among them)."""
    n = check_split_invariance(lib, lms, shape, scale)
    print(f"ctc_stream {shape} scale {scale}: {n} streams, every call memcmp-equal to the one-shot twin")


def test_host_final_nbest_below_the_beam(lib, lms):
    """nbest < beam: the LM form's eos term can lift a prefix from behind the first nbest -- the last call ranks the whole beam."""
    shape = SHAPES[2]
    T, V, beam, cand = shape
    for seed in range(4):
        x = small_case(shape, 2, seed)
        for lm, w in forms(lms, V):
            check_stream(lib, x, V, beam, cand, splits_of(T, seed), lm, w, nbest=3)


# ---- the mutant ---------------------------------------------------------------------------------------------------------------------
def test_node_table_reference_is_the_reference():
    for shape in SHAPES:
        T, V, beam, cand = shape
        for scale in SCALES:
            for seed in range(10):
                x = small_case(shape, scale, seed)
                a, b = S.search_nodes(x, V, PAD, UNK, beam, cand, beam), R.search(x, V, PAD, UNK, beam, cand, beam)
                assert a["hyps"] == b["hyps"] and a["margin"] == b["margin"] and a["cand_id"] == b["cand_id"], (shape, scale, seed)


def test_mutant_that_forgets_the_child_table_fails(lib):
    """The reference that empties its child table before frame 1 of the committed case: its n-best differ from the true
    reference's; the twin, cut at that very frame, gives the one-shot bytes."""
    shape, scale, seed, cut = FORGET_CASE
    T, V, beam, cand = shape
    x = small_case(shape, scale, seed)
    ref = R.search(x, V, PAD, UNK, beam, cand, beam)
    mut = S.search_nodes(x, V, PAD, UNK, beam, cand, beam, forget_at=cut)
    with pytest.raises(AssertionError):
        R.compare(mut, ref)
    check_stream(lib, x, V, beam, cand, [cut])
    rec = one_shot(lib, x, V, beam, cand, beam)
    with pytest.raises(AssertionError):
        R.compare(rec, mut)


# ---- slots --------------------------------------------------------------------------------------------------------------------------
def pack_calls(xs, n_calls=3):
    """Per session the frame count after each of n_calls calls: ragged thirds; the T = 1 session has no new rows after the first."""
    return [[min(x.shape[0], -(-x.shape[0] * (j + 1) // n_calls) + (k % 2 if j + 1 < n_calls else 0)) for j in range(n_calls)]
            for k, x in enumerate(xs)]


def check_pack(lib, lm=None, w=None, gpu=False):
    """Eight slots on ragged splits, a NaN session (frame 17 of session 3), a T = 1 session and sessions without new rows in a
    call: every call's bytes of a session are the same alone, in the pack and in the reversed pack on other slots."""
    V, beam, cand, nbest = 64, 8, 8, 5
    xs = ragged_pack(V)
    upto = pack_calls(xs)
    assert upto[4] == [1, 1, 1] and upto[3][0] < 18 <= upto[3][1]
    opts = None if lm is None else (w[0], w[1], 1)
    h = None if lm is None else lm.h
    n, maxT = len(xs), max(x.shape[0] for x in xs)

    def run(order, slots, S_):
        out = {}
        with S.Stream(lib, V, PAD, UNK, S_, maxT, beam, cand, nbest, h, opts, gpu=gpu) as st:
            f = {k: 0 for k in order}
            for j in range(3):
                rc, recs = st.advance(slots, [xs[k][f[k]:upto[k][j]] for k in order], [upto[k][j] for k in order], [j == 2] * len(order))
                assert rc == 0
                for k, rec in zip(order, recs):
                    out[(k, j)] = rec["raw"] + rec["part_raw"]
                    if k == 3:
                        assert rec["part"] == (upto[3][j], 0, 0, 2) if j else rec["part"][3] == 0
                        assert (rec["status"] == [2] * nbest) == (j > 0)
                    f[k] = upto[k][j]
        return out

    pack = run(list(range(n)), list(range(n)), n)
    rev = run(list(range(n))[::-1], [(3 * k + 1) % n for k in range(n)], n)
    for k in range(n):
        alone = run([k], [0], 1)
        for j in range(3):
            assert alone[(k, j)] == pack[(k, j)] == rev[(k, j)], (k, j)
    for k, x in enumerate(xs):                                 # and the last call is the one-shot search
        want = one_shot(lib, x, V, beam, cand, nbest, lm, w, gpu=gpu)
        assert pack[(k, 2)].startswith(want["raw"]), k


def test_host_pack_nan_session_and_invariance(lib, lms):
    check_pack(lib)
    check_pack(lib, lms[64], WEIGHTS[0])


def check_slot_reuse(lib, lm=None, w=None, gpu=False):
    """A slot after a final call, and after a reset in the middle of an utterance, gives a fresh object's bytes; the utterance
    before filled the trie to max_frames."""
    shape = SHAPES[2]
    T, V, beam, cand = shape
    a, b = small_case(shape, 6, 40), small_case(shape, 2, 41)
    opts = None if lm is None else (w[0], w[1], 1)
    h = None if lm is None else lm.h

    def utter(st, slot, x, cuts=(13, 14)):
        out, f = [], 0
        for t in list(cuts) + [T]:
            rc, recs = st.advance([slot], [x[f:t]], [t], [t == T])
            assert rc == 0
            out.append(recs[0]["raw"] + recs[0]["part_raw"])
            f = t
        return out

    with S.Stream(lib, V, PAD, UNK, 2, T, beam, cand, beam, h, opts, gpu=gpu) as fresh:
        want = utter(fresh, 1, b)
    with S.Stream(lib, V, PAD, UNK, 2, T, beam, cand, beam, h, opts, gpu=gpu) as st:
        utter(st, 1, a)                                        # T = max_frames frames, then the final call's reset
        assert utter(st, 1, b) == want
        rc, _ = st.advance([1], [a[:25]], [25], [0])           # an utterance abandoned after 25 frames
        assert rc == 0 and st.reset(1) == 0
        assert utter(st, 1, b) == want
        assert st.reset(2) != 0 and st.reset(-1) != 0


def test_host_slot_reuse(lib, lms):
    check_slot_reuse(lib)
    check_slot_reuse(lib, lms[64], WEIGHTS[1])


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def check_create_refusals(lib, lm, gpu=False):
    from streamspeech_amd import lib as L
    from streamspeech_amd.ngram import NgramLM
    ok = dict(S=2, max_frames=40, beam=4, cand=4, nbest=2)
    bad = [dict(S=0), dict(max_frames=0), dict(max_frames=L.CTC_BEAM_MAX_FRAMES + 1), dict(beam=0), dict(beam=L.CTC_BEAM_MAX_BEAM + 1),
           dict(cand=0), dict(cand=L.CTC_BEAM_MAX_CAND + 1), dict(nbest=0), dict(nbest=5)]
    mk = lambda V, lm, opts, **kw: S.Stream(lib, V, PAD, UNK, kw["S"], kw["max_frames"], kw["beam"], kw["cand"], kw["nbest"], lm, opts,  # noqa: E731
                                            gpu=gpu)
    for b in bad:
        for h, o in ((None, None), (lm.h, (0.5, 0.0, 1))):
            assert mk(64, h, o, **dict(ok, **b)).rc == L.SS_ERR_ARG, b
    assert mk(0, None, None, **ok).rc == L.SS_ERR_ARG
    assert mk(64, lm.h, None, **ok).rc == L.SS_ERR_ARG            # a model without options, options without a model
    assert mk(64, None, (0.5, 0.0, 1), **ok).rc == L.SS_ERR_ARG
    assert mk(63, lm.h, (0.5, 0.0, 1), **ok).rc == L.SS_ERR_ARG   # a model of another V
    for w, ws in ((np.nan, 0.0), (np.inf, 0.0), (0.5, np.nan), (0.5, -np.inf)):
        assert mk(64, lm.h, (w, ws, 1), **ok).rc == L.SS_ERR_ARG
    a, _ = small_lm(64)
    with NgramLM(dict(a, eos=-1)) as no_eos:
        assert mk(64, no_eos.h, (0.5, 0.0, 1), **ok).rc == L.SS_ERR_ARG
        with mk(64, no_eos.h, (0.5, 0.0, 0), **ok) as st:
            assert st.rc == 0
    assert lib.ss_debug_ctc_stream_create(64, PAD, UNK, int(gpu), 2, 40, 4, 4, 2, None, None, None) == L.SS_ERR_ARG
    for st in (mk(64, None, None, **ok), mk(64, lm.h, (0.5, 0.0, 1), **ok)):
        with st:
            assert st.rc == 0


def check_advance_refusals(lib, lm=None, gpu=False):
    """Every refusal of an advance: SS_ERR_ARG, the sentinel-filled outputs untouched (the runner checks), and the slots' next
    legal calls return what they return in an object that never saw the refused ones."""
    from streamspeech_amd import lib as L
    V, T = 64, 20
    xs = [R.scaled_logits(90, T, V, 6), R.scaled_logits(91, T, V, 6)]
    opts = None if lm is None else (0.5, 0.0, 1)
    h = None if lm is None else lm.h
    mk = lambda: S.Stream(lib, V, PAD, UNK, 2, T, 4, 4, 2, h, opts, gpu=gpu)  # noqa: E731

    def legal(st, tried):
        out = []
        for f, t in ((0, 7), (7, 7), (7, T)):
            rc, recs = st.advance([0, 1], [xs[0][f:t], xs[1][f:t]], [t, t], [t == T] * 2)
            assert rc == 0
            out.append([r["raw"] + r["part_raw"] for r in recs])
            if t == 7 and f == 0:
                tried(st)
        return out

    def refused(st):                                           # both slots stand at 7 frames
        E = L.SS_ERR_ARG
        two = [xs[0][7:9], xs[1][7:9]]
        assert st.advance([0, 2], two, [9, 9], [0, 0])[0] == E                  # a slot outside the object
        assert st.advance([-1, 1], two, [9, 9], [0, 0])[0] == E
        assert st.advance([1, 1], two, [9, 9], [0, 0])[0] == E                  # a slot twice
        assert st.advance([0, 1], [xs[0][7:9], xs[1][6:6]], [9, 6], [0, 0])[0] == E     # upto below the frames consumed
        assert st.advance([0], [np.zeros((T - 6, V), np.float32)], [T + 1], [0])[0] == E    # upto above max_frames
        assert st.advance([0, 1], two, [9, 9], [0, 0], out_stride=8)[0] == E    # out_stride below the largest upto
        assert st.advance([0, 1], two, [9, 9], [0, 0], n=0)[0] == E
        assert st.advance([0, 1], two, [9, 9], [0, 0], n=-1)[0] == E
        assert st.advance([0, 1, 0], two + [xs[0][7:9]], [9, 9, 9], [0, 0, 0])[0] == E      # more sessions than slots
        for name in ("slots", "upto", "final", "logits", "hyps", "tokens", "part"):
            assert st.advance([0, 1], two, [9, 9], [0, 0], null=(name,))[0] == E, name
        x63 = [np.ascontiguousarray(a[:, :63]) for a in two]
        assert st.advance([0, 1], x63, [9, 9], [0, 0])[0] == E                  # ld < V

    with mk() as st:
        want = legal(st, lambda s: None)
    with mk() as st:
        assert legal(st, refused) == want
    # the object kinds do not serve each other's calls
    with S.Stream(lib, V, PAD, UNK, 1, T, 4, 4, 2, h, opts, gpu=gpu) as st:
        hyp, tok, part = np.zeros(4, RL.LMHYP), np.zeros(64, np.int32), np.zeros(1, S.PART)
        P = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        one = (C.c_int32 * 1)
        if gpu:
            assert lib.ss_ctc_stream_advance_host(st.h, 1, one(0), P(xs[0]), V, one(5), one(0), P(hyp), P(tok), 8, P(part)) == L.SS_ERR_ARG
            assert not hyp["status"].any() and not tok.any() and not part["frames"].any()
        assert lib.ss_ctc_stream_advance_host(None, 1, one(0), P(xs[0]), V, one(5), one(0), P(hyp), P(tok), 8, P(part)) == L.SS_ERR_ARG
        assert lib.ss_ctc_stream_reset(None, 0) == L.SS_ERR_ARG
    lib.ss_ctc_stream_destroy(None)


def test_host_refusals(lib, lms):
    check_create_refusals(lib, lms[64])
    check_advance_refusals(lib)
    check_advance_refusals(lib, lms[64])


# ---- the Python layers --------------------------------------------------------------------------------------------------------------
def test_asr_beam_emit():
    from streamspeech_amd.text_policy import asr_beam_emit
    sym = ["a", "bc", "d", "e"]
    assert asr_beam_emit("", sym, 0, False) == ("", "")
    assert asr_beam_emit("", sym, 2, False) == ("a bc", "a bc")
    assert asr_beam_emit("a bc", sym, 2, False) == ("", "a bc")
    assert asr_beam_emit("a bc", sym, 3, False) == (" d", "a bc d")
    assert asr_beam_emit("a bc", sym, 1, True) == (" d e", "a bc d e")         # finished: everything, whatever n_stable says
    assert asr_beam_emit("", [], 0, True) == ("", "")
    text, writes = "", []
    for n, fin in ((0, False), (1, False), (1, False), (3, False), (3, True)):
        new, text = asr_beam_emit(text, sym, n, fin)
        writes.append(new)
    assert "".join(writes) == " ".join(sym) == text
    for prev, s, n in (("a bc", ["a", "x"], 2), ("a bc", ["a", "bcd"], 2), ("a bc", sym, 1), ("a b", ["a", "bc"], 2)):
        with pytest.raises(ValueError):                         # what was written would have to change: cannot happen, and is checked
            asr_beam_emit(prev, s, n, False)
    with pytest.raises(ValueError):
        asr_beam_emit("", sym, 5, False)


def test_ctc_beam_options_validation():
    from streamspeech_amd import lib as L
    from streamspeech_amd import text_policy as P
    assert P.CTC_BEAM_MAX == L.CTC_BEAM_MAX_BEAM == L.CTC_BEAM_MAX_CAND
    o = P.CtcBeamOptions(8)
    assert (o.beam, o.cand, o.nbest, o.lm, o.lm_weight, o.word_score) == (8, None, None, None, 0.5, 0.0)
    assert o.stream_kwargs() == dict(beam=8, cand=None, nbest=None)
    lm = object()
    assert P.CtcBeamOptions(4, 6, 2, lm, 0.3, -0.1).stream_kwargs() == dict(beam=4, cand=6, nbest=2, lm=lm, lm_weight=0.3, word_score=-0.1)
    for kw in (dict(beam=0), dict(beam=33), dict(beam=4, cand=0), dict(beam=4, cand=33), dict(beam=4, nbest=0), dict(beam=4, nbest=5),
               dict(beam=4, lm_weight=float("nan")), dict(beam=4, word_score=float("inf"))):
        with pytest.raises(ValueError):
            P.CtcBeamOptions(**kw)


def test_agent_ctc_beam_flags_parse_and_refusals(tmp_path):
    """The five flags parse on every streaming agent (default off); they are the ASR agent's alone, not with --word-details, and
    the dependent flags need --ctc-beam: ValueError at construction, before anything is loaded."""
    import argparse
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    from streamspeech_amd.text_policy import ctc_beam_flags
    req = ["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0"]

    def parse(cls, *extra):
        p = argparse.ArgumentParser()
        cls.add_args(p)
        return p.parse_args(req + list(extra))

    a = parse(StreamSpeechASRAgent)
    assert (a.ctc_beam, a.ctc_beam_cand, a.ctc_lm, a.ctc_lm_weight, a.ctc_word_score) == (0, None, None, 0.5, 0.0)
    assert ctc_beam_flags(a) is None
    a = parse(StreamSpeechASRAgent, "--ctc-beam", "4", "--ctc-beam-cand", "6", "--ctc-lm", "x.arpa", "--ctc-lm-weight", "0.7",
              "--ctc-word-score", "-0.2")
    o = ctc_beam_flags(a)
    assert (o.beam, o.cand, o.nbest, o.lm, o.lm_weight, o.word_score) == (4, 6, None, None, 0.7, -0.2)
    for cls in (StreamSpeechS2STAgent, StreamSpeechS2TTAgent):
        assert parse(cls).ctc_beam == 0
        with pytest.raises(ValueError, match="ctc-beam"):
            cls(parse(cls, "--ctc-beam", "4"))
    for extra in (("--ctc-beam", "4", "--word-details"), ("--ctc-beam-cand", "4"), ("--ctc-lm", "x.arpa"), ("--ctc-lm-weight", "0.3"),
                  ("--ctc-word-score", "0.1"), ("--ctc-beam", "33"), ("--ctc-beam", "4", "--ctc-beam-cand", "40"),
                  ("--ctc-beam", "4", "--ctc-lm-weight", "0.3")):
        with pytest.raises(ValueError, match="ctc"):
            StreamSpeechASRAgent(parse(StreamSpeechASRAgent, *extra))
