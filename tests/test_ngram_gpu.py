"""The n-gram model's device lookup (csrc/ngram_lm.hip: ss_op_ngram_score, one wave per sequence over the table the fused search
reads) bit-equal to the host twin (ss_ngram_score_host) on the cases of tests/test_ngram_cpu.py, which holds the twin to the ARPA
definition -- plus B = 1 and B = 37 sequences in one call on a model of about 50 000 entries, where probing runs past collisions."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_ngram_cpu import V, check_against_ref, host_score, model, sequences

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def dev_score(lib, lm, seqs, eos, want_state=True):
    n = [len(s) for s in seqs]
    tot = sum(n) + (len(seqs) if eos else 0)
    tok = torch.tensor([t for s in seqs for t in s] or [0], dtype=torch.int32, device="cuda")
    lp = torch.full((tot + 3,), -7.0, dtype=torch.float64, device="cuda")
    st = torch.full((tot + 3,), -7, dtype=torch.int32, device="cuda")
    rc = lib.ss_op_ngram_score(C.c_void_p(torch.cuda.current_stream().cuda_stream), lm.h, len(seqs), C.c_void_p(tok.data_ptr()),
                               (C.c_int32 * len(seqs))(*n), int(eos), C.c_void_p(lp.data_ptr()),
                               C.c_void_p(st.data_ptr()) if want_state else None)
    torch.cuda.synchronize()
    lp, st = lp.cpu().numpy(), st.cpu().numpy()
    assert rc == 0 and (lp[tot:] == -7.0).all() and (st[tot:] == -7).all(), "wrote behind the last entry"
    assert want_state or (st == -7).all()
    return lp[:tot], st[:tot]


def both(lib, lm, a, seqs):
    """The device against the twin bit for bit, and (through tests/test_ngram_cpu.py's check) against the reference."""
    for eos in (True, False):
        hl, hs = host_score(lib, lm, seqs, eos)
        dl, ds = dev_score(lib, lm, seqs, eos)
        assert dl.tobytes() == hl.tobytes() and ds.tobytes() == hs.tobytes(), (a["order"], eos)
    check_against_ref(lambda s, e: dev_score(lib, lm, s, e), a, seqs)


@pytest.mark.parametrize("order", [1, 2, 3, 5])
@pytest.mark.parametrize("unk", [False, True])
def test_op_scores_equal_the_twin(lib, order, unk):
    from streamspeech_amd.ngram import NgramLM
    a, _ = model(order, [0, 60, 80, 60, 40][:order], 11 + order, unk=unk, skip_unigrams=("4", "5"))
    with NgramLM(a) as lm:
        both(lib, lm, a, sequences(order) + [[4, 5, 4, 9, 5]])


def test_op_dropped_suffix_small_tables_and_the_python_handle(lib):
    from streamspeech_amd.ngram import NgramLM
    a, removed = model(3, [0, 150, 200], 5, drop_suffix=True)
    assert removed
    with NgramLM(a) as lm:
        both(lib, lm, a, sequences(3))
        got = lm.score([[7, 8, 9], [], [5]], eos=True)            # NgramLM.score is this op
        hl, _ = host_score(lib, lm, [[7, 8, 9], [], [5]], True)
        assert [len(g) for g in got] == [4, 1, 2] and np.concatenate(got).tobytes() == hl.tobytes()
        assert np.concatenate(lm.score([[7, 8, 9]], eos=False)).tobytes() == host_score(lib, lm, [[7, 8, 9]], False)[0].tobytes()
        dl, _ = dev_score(lib, lm, [[7, 8, 9]], True, want_state=False)
        assert dl.tobytes() == hl[:4].tobytes()
    empty = {"order": 1, "counts": [0], "tokens": np.zeros(0, np.int32), "logp": np.zeros(0, np.float32), "backoff": np.zeros(0, np.float32),
             "V": V, "bos": 0, "eos": 2, "unk": 3, "oov_logp": -3.5}
    with NgramLM(empty) as lm:
        both(lib, lm, empty, [[5, 6, 7], []])
    for extra in (0, 1):
        a, _ = model(2, [0, 63 - (V - 2) + extra], 9)
        with NgramLM(a) as lm:
            both(lib, lm, a, sequences(2))


@pytest.mark.parametrize("B", [1, 37])
def test_op_large_table_many_sequences(lib, B):
    """About 50 000 entries over 2 000 symbols, order 3: 131 072 slots at load 0.38, so many lookups probe past a collision; B
    sequences of ragged lengths (an empty one among them) in one call."""
    from streamspeech_amd.ngram import NgramLM
    a, _ = model(3, [0, 24000, 24000], 17, V=2000, unk=True)
    with NgramLM(a) as lm:
        assert 45000 <= lm.entries <= 52000 and lm.slots == 131072
        rng = np.random.default_rng(B)
        seqs = [rng.integers(2, 2000, n).tolist() for n in ([40] if B == 1 else [0, 1, 2, 3] + rng.integers(1, 60, B - 4).tolist())]
        # sequences that follow the model's own trigrams, so that the high-order entries are hit and not only backed off from
        tri = a["tokens"][a["counts"][0] + 2 * a["counts"][1]:].reshape(-1, 3)
        seqs[-1] = tri[rng.integers(0, len(tri), 12)].reshape(-1).tolist()
        both(lib, lm, a, seqs)


def test_op_refusals(lib):
    from streamspeech_amd import lib as L
    from streamspeech_amd.ngram import NgramLM
    a, _ = model(2, [0, 20], 3)
    tok = torch.tensor([5, 6], dtype=torch.int32, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n = (C.c_int32 * 1)(2)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with NgramLM(dict(a, eos=-1)) as lm:
        assert lib.ss_op_ngram_score(s, None, 1, P(tok), n, 0, P(out), None) == L.SS_ERR_ARG
        assert lib.ss_op_ngram_score(s, lm.h, 0, P(tok), n, 0, P(out), None) == L.SS_ERR_ARG
        assert lib.ss_op_ngram_score(s, lm.h, 1, P(tok), n, 1, P(out), None) == L.SS_ERR_ARG      # no eos id
        assert lib.ss_op_ngram_score(s, lm.h, 1, None, n, 0, P(out), None) == L.SS_ERR_ARG
        assert lib.ss_op_ngram_score(s, lm.h, 1, P(tok), n, 0, None, None) == L.SS_ERR_ARG
        assert lib.ss_op_ngram_score(s, lm.h, 1, P(tok), (C.c_int32 * 1)(-1), 0, P(out), None) == L.SS_ERR_ARG
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any()
