"""Unit spans without a device: tests/spans_ref.py against a direct restatement (the host CTC collapse, units_from_tokens, a walk over
the kept units), the library's host twin (ss_unit_spans_host: the kernel's definitions and refusals) against that reference on every
op case tests/test_unit_spans_gpu.py runs, every refusal, the tiling invariant, and the ABI of the new symbols."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import spans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLANK, PAD, EOS, BOS = R.BLANK, R.PAD, R.EOS, R.BOS


@pytest.fixture(scope="module")
def lib():
    from streamspeech_amd import lib as L
    return L.load()


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_spans(lib, raw, n, K, d0, u0, dur, up, ids=(BLANK, PAD, BOS, EOS), spans=None, k_out=None, B=None):
    rows = 3 if n is None else len(n)
    B = rows if B is None else B
    spans = np.full((max(sum(max(int(x), 0) for x in n), 1) if n is not None else 80, 4), -7, dtype=np.int32) if spans is None else spans
    k_out = np.full(max(rows, 1), -7, dtype=np.int32) if k_out is None else k_out
    rc = lib.ss_unit_spans_host(B, _ptr(raw), None if n is None else _i32(n), None if K is None else _i32(K),
                                None if d0 is None else _i32(d0), None if u0 is None else _i32(u0), _ptr(dur), up, *ids,
                                _ptr(spans), _ptr(k_out))
    return rc, spans, k_out


def test_span_entry_points_are_declared_and_bound(lib):
    from streamspeech_amd import lib as L
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name, nargs in (("ss_batch_unit_spans", 12), ("ss_unit_spans_host", 14), ("ss_op_unit_spans", 15)):
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: the binding has another argument count"
        assert hasattr(lib, name)
    assert lib.ss_abi_version() == 2
    with open(os.path.join(ROOT, "streamspeech_amd", "csrc", "build.sh"), encoding="utf-8") as f:
        assert " unit_spans" in f.read()


def _restated(raw, up, dur, d0, u0):
    """The host's own route to the units (ctc_collapse_host, then units_from_tokens' filter), then a walk over the kept frames."""
    from streamspeech_amd.pipeline import ctc_collapse_host, units_from_tokens
    toks, index = ctc_collapse_host([int(v) for v in raw], BLANK, PAD)
    cfg = SimpleNamespace(eos=EOS)
    kept = [(t, f) for t, f in zip(toks, index) if t not in (BOS, EOS)]
    assert [t - 4 for t, _ in kept] == units_from_tokens(toks + [EOS], cfg) == units_from_tokens(toks, cfg)
    n = len(raw) // up
    out = np.zeros((n, 4), dtype=np.int64)
    units, clock = u0, 0
    for s in range(n):
        out[s, 0], out[s, 2] = units, clock
        for j, (_, f) in enumerate(kept):
            if f // up == s and j >= u0:
                out[s, 1] += 1
                out[s, 3] += int(dur[j - d0])
        units += out[s, 1]
        clock += out[s, 3]
    return out, len(kept)


def test_reference_against_the_hosts_collapse_and_a_unit_walk():
    rng = np.random.default_rng(7)
    crossing = 0
    for i in range(200):
        up = int(rng.choice([1, 3, 25]))
        n = int(rng.integers(1, 9))
        raw = R.random_row(rng, n, up, BLANK, PAD, EOS, p_blank=0.6)
        K = int(R.unit_mask(raw, BLANK, PAD, BOS, EOS).sum())
        u0 = int(rng.integers(0, K + 1))
        d0 = int(rng.integers(0, u0 + 1))
        dur = R.random_dur(rng, K - d0)
        got, k = R.unit_spans(raw, up, BLANK, PAD, BOS, EOS, dur, d0, u0)
        want, kw = _restated(raw, up, dur, d0, u0)
        assert k == kw == K and (got == want).all(), i
        R.check_tiling(got, u0, K, int(dur[u0 - d0: K - d0].sum()) if K > u0 else 0)
        b = np.arange(up, raw.size, up)
        crossing += int(((raw[b] == raw[b - 1]) & (raw[b] >= 4) & (raw[b] != BLANK)).sum())
    assert crossing >= 5          # unit runs that cross a state boundary did occur


@pytest.mark.parametrize("name", sorted(R.op_cases()))
def test_host_twin_on_the_op_cases(lib, name):
    up, rows = R.op_cases()[name]
    raw, K, d0, u0, dur = R.pack_rows(rows)
    n = [r["raw"].size // up for r in rows]
    rc, spans, k_out = host_spans(lib, raw, n, K, d0, u0, dur, up)
    assert rc == 0
    assert k_out.tolist() == K
    off = 0
    for r, nb in zip(rows, n):
        want, k = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"], r["d0"], r["u0"])
        assert k == r["K"] and (spans[off: off + nb] == want).all()
        R.check_tiling(spans[off: off + nb], r["u0"], r["K"], int(np.asarray(r["dur"])[r["u0"] - r["d0"]: r["K"] - r["d0"]].sum())
                       if r["K"] > r["u0"] else 0)
        off += nb


def test_the_named_cases_are_what_they_say():
    cases = R.op_cases()
    up, (r,) = cases["run_crosses_boundary"]
    s, k = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"])
    assert k == 1 and s[:, 1].tolist() == [1, 0] and s[1, 2] == s[0, 3] == r["dur"][0]
    up, (r,) = cases["blank_between"]
    s, k = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"])
    assert k == 2 and s[:, 1].tolist() == [1, 1]
    up, (r,) = cases["one_state_all_blank"]
    assert R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"])[0].tolist() == [[0, 0, 0, 0]]
    up, (r,) = cases["bos_eos"]
    s, k = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"])
    assert k == 4 and s[:, 1].tolist() == [2, 1, 1]
    up, (r,) = cases["u0_is_K"]
    s, _ = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"], r["d0"], r["u0"])
    assert r["K"] > 3 and (s[:, 1:] == 0).all() and (s[:, 0] == r["K"]).all()
    up, (r,) = cases["u0_inside_state"]
    s, _ = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"], r["d0"], r["u0"])
    first = np.flatnonzero(R.unit_mask(r["raw"], BLANK, PAD, BOS, EOS))
    st = first[r["u0"]] // up
    assert 0 < r["d0"] < r["u0"] and first[r["u0"] - 1] // up == st      # the first new unit is not its state's first unit
    assert s[st, 1] < (first // up == st).sum()


def test_a_wrong_count_is_reported_for_its_row_only(lib):
    up, rows = R.op_cases()["ragged_1_65_3"]
    raw, K, d0, u0, dur = R.pack_rows(rows)
    n = [r["raw"].size // up for r in rows]
    wrong = list(K)
    wrong[1] += 2                             # the durations keep their layout: row 2 moves with the count, as a caller's would
    dur2 = np.zeros(sum(wrong), dtype=np.int32)
    o = o2 = 0
    for k, k2 in zip(K, wrong):
        dur2[o2: o2 + k] = dur[o: o + k]
        o, o2 = o + k, o2 + k2
    rc, spans, k_out = host_spans(lib, raw, n, wrong, d0, u0, dur2, up)
    assert rc == 0 and k_out.tolist() == K and k_out[1] != wrong[1]
    off = 0
    for b, (r, nb) in enumerate(zip(rows, n)):
        if b != 1:
            want, _ = R.unit_spans(r["raw"], up, BLANK, PAD, BOS, EOS, r["dur"], r["d0"], r["u0"])
            assert (spans[off: off + nb] == want).all()
        off += nb


def test_every_refusal_writes_nothing(lib):
    from streamspeech_amd.lib import SS_ERR_ARG
    up, rows = R.op_cases()["ragged_1_65_3"]
    raw, K, d0, u0, dur = R.pack_rows(rows)
    n = [r["raw"].size // up for r in rows]
    d0 = [0, 1, 0]
    u0 = [0, 2, 0]
    assert host_spans(lib, raw, n, K, d0, u0, dur, up)[0] == 0

    def refused(**kw):
        a = dict(raw=raw, n=n, K=K, d0=d0, u0=u0, dur=dur, up=up)
        a.update(kw)
        rc, spans, k_out = host_spans(lib, **a)
        assert rc == SS_ERR_ARG, kw
        assert (spans == -7).all() and (k_out == -7).all(), kw

    refused(B=0)
    refused(B=-1)
    refused(raw=None)
    refused(dur=None)
    refused(n=None)
    refused(K=None)
    refused(d0=None)
    refused(u0=None)
    refused(n=[1, 0, 3])
    refused(n=[1, -4, 3])
    refused(d0=[0, 3, 0])                     # d0 > u0
    refused(u0=[0, K[1] + 1, 0])              # u0 > K
    refused(K=[K[0], -1, K[2]])
    refused(d0=[0, -1, 0])
    refused(up=0)
    for missing in ("spans", "k_out"):
        spans = np.full((sum(n), 4), -7, dtype=np.int32)
        k_out = np.full(3, -7, dtype=np.int32)
        rc = lib.ss_unit_spans_host(3, _ptr(raw), _i32(n), _i32(K), _i32(d0), _i32(u0), _ptr(dur), up, BLANK, PAD, BOS, EOS,
                                    None if missing == "spans" else _ptr(spans), None if missing == "k_out" else _ptr(k_out))
        assert rc == SS_ERR_ARG and (spans == -7).all() and (k_out == -7).all()


def test_batch_entry_refuses_before_any_device_call(lib):
    """ss_batch_unit_spans decides its refusals on the host: they answer without a device and without a model."""
    from streamspeech_amd.lib import SS_ERR_ARG
    one = _i32([1])
    buf = np.zeros(8, dtype=np.int32)
    assert lib.ss_batch_unit_spans(None, None, 1, _ptr(buf), one, one, one, one, _ptr(buf), None, _ptr(buf), _ptr(buf)) == SS_ERR_ARG
