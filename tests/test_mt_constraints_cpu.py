"""Lexically constrained beam search without a device: the restatement of the rule (tests/constraint_ref.py) against hand-made
tables and against the reference's own per-step selections recorded in tests/golden/mt_constraints.json; the library's host twin
(ss_mt_cons_select_host) against the restatement on seeded random steps; the refusals (ss_mt_cons_table_host); the packed-tensor
and glossary-file parsers of the Python layers."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import constraint_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "mt_constraints.json")
EOS, PAD = 2, 1
SS_ERR_ARG = 2


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


def i32(a):
    a = np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound(lib):
    from streamspeech_amd import lib as L
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in (("ss_batch_mt_beam_cons", 21), ("ss_mt_cons_select_host", 14), ("ss_op_beam_cons_select", 14),
                        ("ss_mt_cons_table_host", 9)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(lib, name), f"{name} is not exported"
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"
    assert lib.ss_abi_version() == 2
    assert "#define SS_MT_CONS_MAX_TOKENS %d" % L.MT_CONS_MAX_TOKENS in header
    assert L.MT_CONS_TABLE_LD == L.MT_CONS_MAX_TOKENS + 4


# ---- advance and next_tokens against tables made by hand ----------------------------------------------------------------------------
TOKS = (5, 6, 7, 9)
# phrases -> {state: new state for each of TOKS}
ADVANCE = [
    ([[5]], {-1: (0, -1, -1, -1), 0: (0, 0, 0, 0)}),
    # the first token recurs inside the phrase: 5 6 5 7
    ([[5, 6, 5, 7]], {-1: (0, -1, -1, -1), 0: (0, 1, -1, -1), 1: (2, -1, -1, -1), 2: (0, -1, 3, -1), 3: (3, 3, 3, 3)}),
    # two phrases 5 6 | 7: anything may stand between them (state 1), nothing inside the first (state 0)
    ([[5, 6], [7]], {-1: (0, -1, -1, -1), 0: (0, 1, -1, -1), 1: (1, 1, 2, 1), 2: (2, 2, 2, 2)}),
    # no phrase: the only state is finished
    ([], {-1: (-1, -1, -1, -1)}),
]
NEXT = [([[5]], {-1: [5], 0: []}),
        ([[5, 6, 5, 7]], {-1: [5], 0: [6], 1: [5], 2: [5, 7], 3: [5]}),
        ([[5, 6], [7]], {-1: [5], 0: [6], 1: [5, 7], 2: [5]}),
        ([[7, 6], [5]], {1: [5, 7]}),
        ([], {-1: []})]


@pytest.mark.parametrize("phrases,table", ADVANCE)
def test_advance_against_table(phrases, table):
    cons = CR.Constraints(phrases)
    assert sorted(table) == list(range(-1, cons.C)), "the table covers every state"
    for state, want in table.items():
        assert tuple(cons.advance(state, t) for t in TOKS) == want, f"state {state}"


def test_advance_at_the_root_reads_the_last_end_marker():
    """state == -1: the reference indexes endpoints[-1], the last element, which is always set, so a token that does not open the
    first phrase leaves the hypothesis at the root -- through case 3, not through the restart cases."""
    cons = CR.Constraints([[5, 6]])
    assert cons.end == [False, True] and cons.end[-1]
    assert cons.advance(-1, 9) == -1 and cons.advance(-1, 6) == -1 and cons.advance(-1, 5) == 0
    assert cons.advance(0, 9) == -1 and cons.advance(0, 5) == 0        # inside the phrase the restart cases do apply


@pytest.mark.parametrize("phrases,table", NEXT)
def test_next_tokens_against_table(phrases, table):
    cons = CR.Constraints(phrases)
    for state, want in table.items():
        assert cons.next_tokens(state) == want
        assert cons.next_tokens(state, descending=True) == want[::-1]


def test_distinct_token_count():
    assert CR.Constraints([[5, 6, 5, 7]]).U == 3 and CR.Constraints([[5, 6, 5, 7]]).C == 4
    assert CR.Constraints([]).U == 0


# ---- the selection stage against the reference's recorded steps ---------------------------------------------------------------------
def _fix():
    return json.load(open(FIX, encoding="utf-8"))


def _f32(bits):
    return np.asarray(bits, np.int32).view(np.float32)


def test_selection_equals_recorded_reference_steps():
    n = 0
    for name, grp in _fix()["groups"].items():
        k = grp["beam"]
        traced = [r for r in grp["hypotheses"].values() if "trace" in r]
        assert len(traced) >= 2, name
        for rec in traced:
            cons = CR.Constraints(rec["phrases"])
            for st in rec["trace"]:
                cands = list(zip(_f32(st["cand_score_bits"]), st["cand_tok"], st["cand_beam"]))
                got = CR.select_from(cons, cands, st["states"], k)
                assert [int(np.float32(s).view(np.int32)) for s, _, _, _ in got] == st["out_score_bits"], (name, st["step"])
                assert [t for _, t, _, _ in got] == st["out_tok"], (name, st["step"])
                assert [b for _, _, b, _ in got] == st["out_beam"], (name, st["step"])
                assert [s for _, _, _, s in got] == st["out_state"], (name, st["step"])
                n += 1
    assert n >= 40


def test_every_golden_hypothesis_contains_its_phrases_in_order():
    for name, grp in _fix()["groups"].items():
        pinned = [r for r in grp["hypotheses"].values() if r["margin"] > r["tau"]]
        assert len(pinned) >= 6, name
        for rec in grp["hypotheses"].values():
            for h in rec.get("nbest", ()):
                assert None not in CR.contains_in_order(h["tokens"], rec["phrases"])


# ---- the host twin against the restatement ------------------------------------------------------------------------------------------
def _random_step(rng, k, V, C_, step, ties, neg_inf):
    """Phrases of 1 - 4 tokens summing to C_ (ids may recur where V is small), random states, random rows."""
    toks = [int(t) for t in rng.choice([t for t in range(V) if t not in (EOS,)], C_, replace=C_ > V - 1)] if C_ else []
    phrases, o = [], 0
    while o < C_:
        n = int(min(C_ - o, rng.integers(1, 5)))
        phrases.append(toks[o:o + n])
        o += n
    cons = CR.Constraints(phrases)
    states = [-1] * k if step == 0 else [int(s) for s in rng.integers(-1, C_, k)]
    lp = (-rng.random((k, V)) * 8).astype(np.float32)
    if ties:
        lp = np.round(lp * 2) / 2
    if neg_inf:
        lp[rng.random((k, V)) < (0.9 if neg_inf > 1 else 0.2)] = -np.inf
    cum = (np.round(-rng.random(k) * 12) if ties else -rng.random(k) * 12).astype(np.float32)
    return cons, phrases, states, lp.astype(np.float32), cum


def _host_select(lib, lp, cum, k, V, step, states, phrases):
    toks = [t for p in phrases for t in p]
    ends = [int(i == len(p) - 1) for p in phrases for i in range(len(p))]
    ta, tp = i32(toks or [0])
    ea, ep = i32(ends or [0])
    sa, sp = i32(states)
    lp = np.ascontiguousarray(lp, np.float32)
    cum = np.ascontiguousarray(cum, np.float32)
    os_ = np.full(2 * k, np.nan, np.float32)
    ot, ob, ost = (np.full(2 * k, -7, np.int32) for _ in range(3))
    rc = lib.ss_mt_cons_select_host(lp.ctypes.data, cum.ctypes.data, k, V, step, EOS, sa.ctypes.data, ta.ctypes.data, len(toks),
                                    ea.ctypes.data, os_.ctypes.data, ot.ctypes.data, ob.ctypes.data, ost.ctypes.data)
    return rc, os_, ot, ob, ost


SIZES = [(k, V, C_) for k in (1, 2, 5, 32) for V in (37, 300) for C_ in (0, 1, 3, 7, 64)]


@pytest.mark.parametrize("k,V,C_", SIZES)
def test_host_twin_equals_restatement(lib, k, V, C_):
    rng = np.random.default_rng(1000 * k + V + C_)
    if V < 2 * k + 1:                               # the search's own limit (the top-2k list needs 2k real candidates)
        cons, phrases, states, lp, cum = _random_step(rng, k, V, C_, 1, False, 0)
        assert _host_select(lib, lp, cum, k, V, 1, states, phrases)[0] == SS_ERR_ARG
        return
    for step in (0, 1, 4):
        for ties, neg_inf in ((False, 0), (True, 0), (False, 1), (True, 2)):
            cons, phrases, states, lp, cum = _random_step(rng, k, V, C_, step, ties, neg_inf)
            rc, s, t, b, st = _host_select(lib, lp, cum, k, V, step, states, phrases)
            assert rc == 0
            want = CR.select(cons, lp, cum, states, k, step, EOS)
            what = f"k {k} V {V} C {C_} step {step} ties {ties} -inf {neg_inf}"
            assert s.view(np.int32).tolist() == [int(np.float32(x[0]).view(np.int32)) for x in want], what
            assert t.tolist() == [x[1] for x in want], what
            assert b.tolist() == [x[2] for x in want], what
            assert st.tolist() == [x[3] for x in want], what
            assert want == CR.select(cons, lp, cum, states, k, step, EOS, descending=True), "the order of a row's next tokens shows"


def test_no_phrases_is_the_plain_top_2k(lib):
    """C = 0: the selection is the global top 2k in the plain search's order, whatever the rows' bests add."""
    rng = np.random.default_rng(5)
    k, V = 5, 300
    for ties in (False, True):
        cons, phrases, states, lp, cum = _random_step(rng, k, V, 0, 2, ties, 0)
        rc, s, t, b, st = _host_select(lib, lp, cum, k, V, 2, states, phrases)
        assert rc == 0
        rows = lp + cum[:, None]
        order = sorted(range(k * V), key=lambda i: (-float(rows.reshape(-1)[i]), i))[:2 * k]
        assert (t.tolist(), b.tolist()) == ([i % V for i in order], [i // V for i in order])
        assert s.view(np.int32).tolist() == rows.reshape(-1)[order].view(np.int32).tolist()
        assert st.tolist() == [-1] * (2 * k)


def test_host_twin_refuses_a_state_outside_the_phrases_and_bad_phrases(lib):
    rng = np.random.default_rng(9)
    cons, phrases, states, lp, cum = _random_step(rng, 2, 37, 3, 1, False, 0)
    assert _host_select(lib, lp, cum, 2, 37, 1, states, phrases)[0] == 0
    for bad in ([3, -1], [-2, 0]):
        rc, s, t, b, st = _host_select(lib, lp, cum, 2, 37, 1, bad, phrases)
        assert rc == SS_ERR_ARG and np.isnan(s).all() and (t == -7).all()
    assert _host_select(lib, lp, cum, 2, 37, 1, [-1, -1], [[5, EOS]])[0] == SS_ERR_ARG
    assert _host_select(lib, lp, cum, 2, 37, 1, [-1, -1], [[5, 37]])[0] == SS_ERR_ARG


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _table(lib, phrases_per_utt, V=50, max_len=None, ends=None, off=None):
    toks = [t for ph in phrases_per_utt for p in ph for t in p]
    e = ends if ends is not None else [int(i == len(p) - 1) for ph in phrases_per_utt for p in ph for i in range(len(p))]
    o = off if off is not None else np.concatenate([[0], np.cumsum([sum(len(p) for p in ph) for ph in phrases_per_utt])])
    B = len(phrases_per_utt)
    ta, tp = i32(toks or [0])
    ea, ep = i32(e or [0])
    oa, op = i32(o)
    ml = i32(max_len)[1] if max_len is not None else None
    from streamspeech_amd.lib import MT_CONS_TABLE_LD
    tab = np.full(B * MT_CONS_TABLE_LD, -9, np.int32)
    rc = lib.ss_mt_cons_table_host(B, tp, op, ep, V, PAD, EOS, ml, tab.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, tab.reshape(B, MT_CONS_TABLE_LD)


def test_table_layout(lib):
    rc, tab = _table(lib, [[[5, 6, 5, 7]], [], [[9], [8, 9]]])
    assert rc == 0
    assert tab[0, :4].tolist() == [5, 6, 5, 7] and tab[0, 64:].tolist() == [4, 3, 0b1000, 0]
    assert tab[1, 64:].tolist() == [0, 0, 0, 0]
    assert tab[2, :3].tolist() == [9, 8, 9] and tab[2, 64:].tolist() == [3, 2, 0b101, 0]
    rc, tab = _table(lib, [[[4 + i % 40 for i in range(64)]]])
    assert rc == 0 and tab[0, 64:].tolist() == [64, 40, 0, -2 ** 31]


@pytest.mark.parametrize("what,kw", [
    ("more than 64 tokens", dict(phrases_per_utt=[[[4 + i % 40 for i in range(65)]]])),
    ("a token at V", dict(phrases_per_utt=[[[5, 50]]])),
    ("a negative token", dict(phrases_per_utt=[[[-1]]])),
    ("pad in a phrase", dict(phrases_per_utt=[[[5, PAD]]])),
    ("</s> in a phrase", dict(phrases_per_utt=[[[EOS]]])),
    ("an open last phrase", dict(phrases_per_utt=[[[5, 6]]], ends=[0, 0])),
    ("C above max_len", dict(phrases_per_utt=[[[5]], [[5, 6, 7]]], max_len=[4, 2])),
    ("offsets that decrease", dict(phrases_per_utt=[[[5]], [[6]]], off=[0, 2, 1])),
])
def test_refusals(lib, what, kw):
    rc, tab = _table(lib, **kw)
    assert rc == SS_ERR_ARG, what
    assert (tab == -9).all(), "nothing is written after a refusal"


def test_packing_refuses_an_empty_phrase_and_a_wrong_count():
    from streamspeech_amd.lib import pack_constraints
    toks, off, ends = pack_constraints([[[5, 6], [7]], None, [[8]]], 3)
    assert toks.tolist() == [5, 6, 7, 8] and off.tolist() == [0, 3, 3, 4] and ends.tolist() == [0, 1, 1, 1]
    with pytest.raises(ValueError, match="empty"):
        pack_constraints([[[5], []]], 1)
    with pytest.raises(ValueError):
        pack_constraints([[[5]]], 2)


# ---- the Python layers --------------------------------------------------------------------------------------------------------------
def test_packed_tensor_parsing():
    """fairseq's pack_constraints layout, its own docstring's example among them."""
    from streamspeech_amd.generators import unpack_constraints
    packed = torch.tensor([[3, 3, 1, 2, 0, 3, 0, 4, 5, 6, 7, 0], [0] * 12, [1, 1, 8, 9, 10, 1, 4, 11, 12, 0, 0, 0]])
    want = [[[3, 1, 2], [3], [4, 5, 6, 7]], [], [[1, 8, 9, 10, 1, 4, 11, 12]]]
    assert unpack_constraints(packed, 3) == want
    assert [CR.parse_packed(r) for r in packed.tolist()] == want
    assert unpack_constraints(packed[2], 1) == want[2:]
    assert unpack_constraints(want, 3) == want
    with pytest.raises(ValueError):
        unpack_constraints(packed, 2)
    with pytest.raises(ValueError, match="closing"):
        unpack_constraints(torch.tensor([[1, 5, 6]]), 1)


def test_generator_refuses_constraints_when_sampling_and_behind_a_prefix():
    from types import SimpleNamespace
    from oracle.ref_agent import make_dicts
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.generators import SequenceGenerator
    cfg = ModelConfig()
    eng = SimpleNamespace(cfg=cfg)
    d = make_dicts(cfg)["target_unigram"]
    enc = [{"encoder_out": [torch.zeros(7, 1, cfg.encoder_embed_dim if hasattr(cfg, "encoder_embed_dim") else 8)]}]
    gen = SequenceGenerator(eng, d, beam_size=2, sampling=True)
    with pytest.raises(NotImplementedError, match="Target-side constraints were provided, but search method doesn't support them"):
        gen.generate_decoder(enc, torch.zeros(1, 30, 80), None, constraints=[[[5]]])
    gen = SequenceGenerator(eng, d, beam_size=2)
    with pytest.raises(ValueError, match="prefix"):
        gen.generate_decoder(enc, torch.zeros(1, 30, 80), None, prefix_tokens=torch.tensor([[7]]), constraints=[[[5]]])


def test_constraints_file_parser():
    from oracle.ref_agent import make_dicts
    from streamspeech_amd import offline
    from streamspeech_amd.config import ModelConfig
    d = make_dicts(ModelConfig())["target_unigram"]
    a, b, c = d[10], d[11], d[200]
    got = offline.parse_constraints_file([f"3\t{a} {b}\t{c}\n", "\n", f"7\t{c}\r\n", f"3\t{b}\n"], d)
    assert got == {3: [[10, 11], [200], [11]], 7: [[200]]}
    with pytest.raises(ValueError, match="id 5.*not in the target dictionary"):
        offline.parse_constraints_file([f"5\t{a} no-such-piece-anywhere\n"], d)
    with pytest.raises(ValueError, match="id 5.*empty"):
        offline.parse_constraints_file([f"5\t{a}\t\t{b}\n"], d)
    with pytest.raises(ValueError, match="not a sample id"):
        offline.parse_constraints_file([f"x\t{a}\n"], d)
    assert offline.phrase_positions([9, 5, 6, 7, 5, 6, 2], [[5, 6], [5, 6]]) == [1, 4]
    assert offline.phrase_positions([9, 5, 6, 7, 2], [[7], [5, 6]]) == [3, None]


def test_driver_flags(capsys):
    from streamspeech_amd import offline
    ap = offline.build_parser()
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", "x"]
    assert ap.parse_args(base).constraints is None
    assert ap.parse_args(base + ["--constraints", "--constraints-file", "g.tsv"]).constraints == "ordered"
    assert ap.parse_args(base + ["--constraints", "ordered"]).constraints == "ordered"
    for argv, msg in ((["--constraints", "unordered", "--constraints-file", "g.tsv"], "unordered is not implemented"),
                      (["--constraints"], "go together"), (["--constraints-file", "g.tsv"], "go together"),
                      (["--constraints", "--constraints-file", "g.tsv", "--sampling"], "cannot be combined")):
        with pytest.raises(SystemExit):
            offline.main(base + argv)
        assert msg in capsys.readouterr().err
