"""The hotword set's device step (csrc/ctc_bias.hip: the score kernel behind ss_op_ctc_bias_score, the step the biased search runs
inside its frame loop) against the plain-C++ scorer that tests/test_ctc_bias_cpu.py pins to the definition: bit for bit, on a
4000-phrase set whose child table many lookups probe past a collision."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_ctc_bias_cpu import score_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def big_set(n=4000, V=6000, seed=5):
    """n distinct phrases of 1 .. 6 tokens over V = 6000: a phrase's first token comes from [4, 3000) and the others from
    [3000, V), so none occurs inside another past its start; every fourth extends an earlier phrase (prefix nesting)."""
    rng = np.random.default_rng(seed)
    seen, phrases = set(), []
    while len(phrases) < n:
        if phrases and len(phrases) % 4 == 3:
            p = tuple(phrases[int(rng.integers(len(phrases)))]) + (int(rng.integers(3000, V)),)
        else:
            p = (int(rng.integers(4, 3000)),) + tuple(int(v) for v in rng.integers(3000, V, int(rng.integers(0, 6))))
        if len(p) <= 32 and p not in seen:
            seen.add(p)
            phrases.append(list(p))
    boosts = rng.uniform(-1.0, 4.0, n).astype(np.float32).tolist()
    return phrases, boosts


def test_op_score_is_the_host_scorer_bit_for_bit(lib):
    """256 sequences of 0 .. 80 tokens glued from whole phrases, cut phrases and stray tokens, finish on and off: delta, state
    and sum of ss_op_ctc_bias_score are the bytes of ss_ctc_bias_score_host; CtcBias.score returns the sums; buffers guarded."""
    from streamspeech_amd.hotwords import CtcBias
    phrases, boosts = big_set()
    rng = np.random.default_rng(11)
    seqs = [[]]
    while len(seqs) < 256:
        y = []
        for _ in range(int(rng.integers(1, 14))):
            p = phrases[int(rng.integers(len(phrases)))]
            r = rng.random()
            y += p if r < 0.5 else p[:int(rng.integers(1, len(p) + 1))] if r < 0.8 else [int(rng.integers(4, 6000))]
        seqs.append(y[:80])
    n = [len(s) for s in seqs]
    total = sum(n)
    with CtcBias(phrases, boosts, 6000, 1, 3) as bias:
        assert bias.n_phrases == 4000 and bias.states > 4000 and bias.device_bytes == 12 * bias.slots + 32 * bias.states
        for finish in (True, False):
            want = score_host(lib, bias, seqs, finish)
            tok = torch.tensor([t for s in seqs for t in s], dtype=torch.int32, device="cuda")
            delta = torch.full((total + 3,), -7.0, dtype=torch.float64, device="cuda")
            state = torch.full((total + 3,), -7, dtype=torch.int32, device="cuda")
            sums = torch.full((len(seqs) + 3,), -7.0, dtype=torch.float64, device="cuda")
            rc = lib.ss_op_ctc_bias_score(C.c_void_p(torch.cuda.current_stream().cuda_stream), bias.h, len(seqs), C.c_void_p(tok.data_ptr()),
                                          (C.c_int32 * len(seqs))(*n), int(finish), C.c_void_p(delta.data_ptr()),
                                          C.c_void_p(state.data_ptr()), C.c_void_p(sums.data_ptr()))
            torch.cuda.synchronize()
            assert rc == 0
            d, s, t = delta.cpu().numpy(), state.cpu().numpy(), sums.cpu().numpy()
            assert (d[total:] == -7.0).all() and (s[total:] == -7).all() and (t[len(seqs):] == -7.0).all(), "wrote behind the last entry"
            assert d[:total].tobytes() == np.asarray([v for w in want for v in w[0]], np.float64).tobytes()
            assert s[:total].tolist() == [v for w in want for v in w[1]]
            assert t[:len(seqs)].tobytes() == np.asarray([w[2] for w in want], np.float64).tobytes()
            assert bias.score(seqs, finish) == [w[2] for w in want]
        assert np.count_nonzero(np.asarray([w[2] for w in want])) > 200
        from streamspeech_amd import lib as L
        assert lib.ss_op_ctc_bias_score(None, None, 1, None, (C.c_int32 * 1)(0), 1, None, None, C.c_void_p(sums.data_ptr())) == L.SS_ERR_ARG
        assert lib.ss_op_ctc_bias_score(None, bias.h, 1, None, (C.c_int32 * 1)(2), 1, None, None, C.c_void_p(sums.data_ptr())) == L.SS_ERR_ARG
