"""Pins tests/attention_ref.py, the float64 reference tests/test_attention_gpu.py holds the attention kernels to: a wrong
reference must not bless a wrong kernel.  attn_ref against a scalar triple loop written straight from the definitions at tiny
sizes for every mask combination, and against the function the existing op tests use; the ragged / ancestry / pool forms against
attn_ref on the cases where they must coincide with it."""
import itertools
import math

import pytest
import torch

from tests import attention_ref as R

DH = 64


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _scalar_attention(q, k, v, H, scale, causal, chunk, q0, tail, P, u, vb):
    """for head, for query, for key: plain Python floats (float64), nothing vectorised beyond the 64-term dot products."""
    Tq, Tk = len(q), len(k)
    out = [[0.0] * (H * DH) for _ in range(Tq)]
    for h in range(H):
        c0 = h * DH
        for i in range(Tq):
            scores = []
            for j in range(Tk):
                hidden = j >= Tk - tail
                if causal and j > i + Tk - Tq:
                    hidden = True
                if chunk > 0 and j >= ((q0 + i) // chunk + 1) * chunk:
                    hidden = True
                if hidden:
                    scores.append(None)
                    continue
                if P is None:
                    s = sum(q[i][c0 + d] * k[j][c0 + d] for d in range(DH))
                else:
                    row = P[j - (q0 + i) + Tk - 1]
                    s = sum((q[i][c0 + d] + u[c0 + d]) * k[j][c0 + d] for d in range(DH))
                    s += sum((q[i][c0 + d] + vb[c0 + d]) * row[c0 + d] for d in range(DH))
                scores.append(s * scale)
            m = max(s for s in scores if s is not None)
            w = [0.0 if s is None else math.exp(s - m) for s in scores]
            z = sum(w)
            for d in range(DH):
                out[i][c0 + d] = sum(w[j] * v[j][c0 + d] for j in range(Tk)) / z
    return torch.tensor(out, dtype=torch.float64)


_PLAIN = [(Tq, Tk, causal, chunk, 0, tail, False)
          for (Tq, Tk) in ((3, 5), (1, 4), (4, 4))
          for causal, chunk, tail in itertools.product((0, 1), (0, 2, 3), (0, 1, 2))]
_RELPOS = [(Tk - q0, Tk, causal, chunk, q0, tail, True)
           for (Tk, q0) in ((5, 0), (5, 2), (4, 3))
           for causal, chunk, tail in itertools.product((0, 1), (0, 2, 3), (0, 1, 2))
           if not (causal and q0)]         # a causal mask is defined for q0 == 0 only (launch_attention refuses the pair)


@pytest.mark.parametrize("Tq,Tk,causal,chunk,q0,tail,relpos", _PLAIN + _RELPOS)
def test_attn_ref_equals_the_scalar_triple_loop(Tq, Tk, causal, chunk, q0, tail, relpos):
    H = 2
    q, k, v = rnd(Tq, H * DH, seed=1) * 0.5, rnd(Tk, H * DH, seed=2), rnd(Tk, H * DH, seed=3)
    P = u = vb = None
    if relpos:
        P, u, vb = rnd(2 * Tk - 1, H * DH, seed=4), rnd(H * DH, seed=5) * 0.3, rnd(H * DH, seed=6) * 0.3
    got = R.attn_ref(q, k, v, H, 0.25, bool(causal), chunk, q0, tail, P, u, vb)
    assert got.dtype == torch.float64 and got.shape == (Tq, H * DH)
    dbl = [None if t is None else t.double().tolist() for t in (q, k, v, P, u, vb)]
    want = _scalar_attention(dbl[0], dbl[1], dbl[2], H, 0.25, causal, chunk, q0, tail, dbl[3], dbl[4], dbl[5])
    assert (got - want).abs().max() < 1e-13


def test_a_hidden_key_has_no_influence_and_a_visible_one_has():
    """The masks hide exactly the keys the definition names: changing a hidden key's K / V rows leaves the output bits alone,
    changing the last visible one does not."""
    H, Tq, Tk = 1, 3, 9
    q, k, v = rnd(Tq, DH, seed=7), rnd(Tk, DH, seed=8), rnd(Tk, DH, seed=9)
    base = R.attn_ref(q, k, v, H, 1.0, k_mask_tail=2)
    k2, v2 = k.clone(), v.clone()
    k2[7:] = 1e4
    v2[7:] = 1e4
    assert torch.equal(R.attn_ref(q, k2, v2, H, 1.0, k_mask_tail=2), base)
    v2[6] += 1.0
    assert not torch.equal(R.attn_ref(q, k2, v2, H, 1.0, k_mask_tail=2), base)


def test_attn_ref_agrees_with_the_reference_of_the_op_tests():
    """Same numbers as tests/test_ops_gpu._attn_ref computes in float64 on that file's own plain and rel-pos cases."""
    from tests.test_ops_gpu import _attn_ref
    for Tq, Tk, causal in [(130, 130, 1), (1, 37, 1), (50, 21, 0), (9, 9, 0), (3, 40, 1)]:
        q, k, v = rnd(Tq, 512, seed=23) * 0.3, rnd(Tk, 512, seed=24), rnd(Tk, 512, seed=25)
        old = _attn_ref(q.double(), k.double(), v.double(), 8, 1.0, bool(causal), 0)
        assert (R.attn_ref(q, k, v, 8, 1.0, bool(causal)) - old).abs().max() < 1e-13
    for T, chunk in [(21, 0), (21, 8), (125, 16), (65, 24), (1, 0), (17, 16), (48, 24)]:
        qkv, Pt = rnd(T, 768, seed=19), rnd(2 * T - 1, 256, seed=20)
        u, vb = rnd(256, seed=21) * 0.3, rnd(256, seed=22) * 0.3
        q, k, v = qkv[:, :256], qkv[:, 256:512], qkv[:, 512:]
        old = _attn_ref(q.double(), k.double(), v.double(), 4, 0.125, False, chunk, Pt.double(), u.double(), vb.double())
        assert (R.attn_ref(q, k, v, 4, 0.125, False, chunk, 0, 0, Pt, u, vb) - old).abs().max() < 1e-13


def test_float32_run_of_the_reference_is_close_to_the_float64_run():
    q, k, v = rnd(40, 512, seed=23) * 0.3, rnd(90, 512, seed=24), rnd(90, 512, seed=25)
    o64 = R.attn_ref(q, k, v, 8, 1.0)
    o32 = R.attn_ref(q, k, v, 8, 1.0, dtype=torch.float32)
    assert o32.dtype == torch.float32
    assert 0 < (o32.double() - o64).abs().max() < 2e-5


@pytest.mark.parametrize("relpos", [False, True])
def test_ragged_ref_of_one_segment_equals_attn_ref(relpos):
    H, T, p_tmax = 2, 7, 16
    Q, K, V = rnd(12, H * DH, seed=1), rnd(15, H * DH, seed=2), rnd(15, H * DH, seed=3)
    if relpos:
        P, u, vb = rnd(2 * p_tmax - 1, H * DH, seed=4), rnd(H * DH, seed=5), rnd(H * DH, seed=6)
        got = R.ragged_ref(Q, K, V, H, 0.125, [(3, T, 5, T)], 12, chunk=4, P=P, u=u, vb=vb, p_tmax=p_tmax)
        want = R.attn_ref(Q[3:10], K[5:12], V[5:12], H, 0.125, False, 4, 0, 0, P[p_tmax - T: p_tmax + T - 1], u, vb)
    else:
        got = R.ragged_ref(Q, K, V, H, 1.0, [(3, 4, 5, T)], 12, causal=True, k_mask_tail=5, seg_tail=[2])
        want = R.attn_ref(Q[3:7], K[5:12], V[5:12], H, 1.0, True, k_mask_tail=2)     # seg_tail replaces the scalar
        assert torch.equal(got[3:7], want)
        got = R.ragged_ref(Q, K, V, H, 1.0, [(3, 4, 5, T)], 12, causal=True, k_mask_tail=2)
    rows = slice(3, 10) if relpos else slice(3, 7)
    assert torch.equal(got[rows], want)
    mask = torch.ones(12, dtype=torch.bool)
    mask[rows] = False
    assert torch.isnan(got[mask]).all() and torch.isfinite(got[rows]).all()


def test_ragged_ref_places_every_segment():
    H = 1
    Q, K, V = rnd(10, DH, seed=1), rnd(20, DH, seed=2), rnd(20, DH, seed=3)
    segs = [(6, 3, 0, 8), (0, 2, 11, 9)]
    got = R.ragged_ref(Q, K, V, H, 1.0, segs, 10, seg_tail=[0, 4])
    assert torch.equal(got[6:9], R.attn_ref(Q[6:9], K[0:8], V[0:8], H, 1.0))
    assert torch.equal(got[0:2], R.attn_ref(Q[0:2], K[11:20], V[11:20], H, 1.0, k_mask_tail=4))
    assert torch.isnan(got[2:6]).all() and torch.isnan(got[9:]).all()


def test_anc_ref_with_an_identity_table_equals_ragged_ref():
    H, slots, ld, k0 = 2, 3, 10, 2
    Q = rnd(6, H * DH, seed=1)
    K, V = rnd(slots * ld, H * DH, seed=2), rnd(slots * ld, H * DH, seed=3)
    segs = [(0, 1, k0, 5), (2, 2, k0, 8), (5, 1, k0, 1)]
    anc = [z for z in range(slots) for _ in range(ld)]
    got = R.anc_ref(Q, K, V, H, 1.0, segs, anc, ld, slots, 6, seg_tail=[0, 3, 0])
    plain = [(qs, ql, z * ld + ks, kl) for z, (qs, ql, ks, kl) in enumerate(segs)]
    want = R.ragged_ref(Q, K, V, H, 1.0, plain, 6, seg_tail=[0, 3, 0])
    assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))


def test_anc_ref_follows_the_table_and_clamps_to_the_last_slot():
    H, slots, ld = 1, 3, 4
    Q, K, V = rnd(1, DH, seed=1), rnd(slots * ld, DH, seed=2), rnd(slots * ld, DH, seed=3)
    anc = [2, 0, 9, 1]                       # position 2 names slot 9: read from the last slot (2)
    rows = [2 * ld + 0, 0 * ld + 1, 2 * ld + 2, 1 * ld + 3]
    got = R.anc_ref(Q, K, V, H, 1.0, [(0, 1, 0, 4)], anc, ld, slots, 1)
    assert torch.equal(got, R.attn_ref(Q, K[rows], V[rows], H, 1.0))


def test_pool_ref_of_one_session_equals_attn_ref_with_q0():
    H, D, slot_rows, p_tmax = 2, 2 * DH, 12, 16
    n, r0, slot, chunk = 3, 6, 1, 4
    T2 = r0 + n
    Qs, cache = rnd(5, 3 * D, seed=1), rnd(2 * slot_rows, 3 * D, seed=2)
    P, u, vb = rnd(2 * p_tmax - 1, D, seed=3), rnd(D, seed=4), rnd(D, seed=5)
    out, after = R.pool_ref(Qs, cache, H, 0.125, [(1, n, r0, T2, slot, chunk)], P, u, vb, p_tmax, slot_rows, 5)
    keys = torch.cat([cache[slot_rows: slot_rows + r0], Qs[1:4]])
    want = R.attn_ref(Qs[1:4, :D], keys[:, D:2 * D], keys[:, 2 * D:], H, 0.125, False, chunk, r0, 0,
                      P[p_tmax - T2: p_tmax + T2 - 1], u, vb)
    assert torch.equal(out[1:4], want)
    assert torch.isnan(out[0]).all() and torch.isnan(out[4]).all()
    assert torch.equal(after[slot_rows + r0: slot_rows + T2], Qs[1:4])
    keep = torch.ones(2 * slot_rows, dtype=torch.bool)
    keep[slot_rows + r0: slot_rows + T2] = False
    assert torch.equal(after[keep], cache[keep])


def test_pool_ref_fresh_session_reads_nothing_from_the_cache():
    H, D, slot_rows, p_tmax = 1, DH, 8, 8
    Qs = rnd(4, 3 * D, seed=1)
    cache = torch.full((slot_rows, 3 * D), float("nan"))
    P, u, vb = rnd(2 * p_tmax - 1, D, seed=3), rnd(D, seed=4), rnd(D, seed=5)
    out, after = R.pool_ref(Qs, cache, H, 0.125, [(0, 4, 0, 4, 0, 0)], P, u, vb, p_tmax, slot_rows, 4)
    assert torch.isfinite(out).all()
    assert torch.equal(out, R.attn_ref(Qs[:, :D], Qs[:, D:2 * D], Qs[:, 2 * D:], H, 0.125, P=P[p_tmax - 4: p_tmax + 3], u=u, vb=vb))
    assert torch.equal(after[:4], Qs) and torch.isnan(after[4:]).all()
