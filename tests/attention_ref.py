"""Plain torch references of every attention form of csrc/attention.hip, in float64 from float32 inputs.

Written from the definitions in csrc/attention.hpp (and the reference modules it cites: the espnet rel-pos attention of the
Conformer encoder, fairseq's multi-head attention), not from the kernels: the whole [Tq, Tk] score matrix is materialised, masked
with -inf, soft-maxed in one pass and multiplied with V.  Head h owns columns [64 h, 64 h + 64) of every row.
tests/test_attention_ref_cpu.py pins these functions against a scalar triple loop; tests/test_attention_gpu.py compares the
kernels with them.  ``dtype`` exists for one purpose: the float32 run of the same arithmetic, whose distance from the float64 run
is the yardstick of the peaked-data cases.
"""
import torch

DH = 64


def attn_ref(q, k, v, H, scale, causal=False, chunk=0, q0=0, k_mask_tail=0, P=None, u=None, vb=None, dtype=torch.float64):
    """q [Tq, H*64], k / v [Tk, H*64]; P [2*Tk-1, H*64], u / vb [H*64] for the rel-pos form.  Returns [Tq, H*64] in ``dtype``.

    score[i, j] = ((q_i + u) . k_j + (q_i + vb) . P[j - (q0 + i) + Tk - 1]) * scale  (the P term and the biases only with P);
    key j is hidden iff j >= Tk - k_mask_tail, or (causal) j > i + Tk - Tq, or (chunk > 0) j >= ((q0 + i) // chunk + 1) * chunk."""
    Tq, Tk = q.shape[0], k.shape[0]
    assert q.shape[1] == H * DH and k.shape == (Tk, H * DH) and v.shape == (Tk, H * DH)
    qh = q.to(dtype).reshape(Tq, H, DH).permute(1, 0, 2)
    kh = k.to(dtype).reshape(Tk, H, DH).permute(1, 0, 2)
    vh = v.to(dtype).reshape(Tk, H, DH).permute(1, 0, 2)
    i = torch.arange(Tq)[:, None]
    j = torch.arange(Tk)[None, :]
    if P is not None:
        assert P.shape == (2 * Tk - 1, H * DH) and q0 + Tq <= Tk
        ph = P.to(dtype).reshape(2 * Tk - 1, H, DH).permute(1, 0, 2)
        ac = torch.einsum("hid,hjd->hij", qh + u.to(dtype).reshape(H, 1, DH), kh)
        g = torch.einsum("hid,hrd->hir", qh + vb.to(dtype).reshape(H, 1, DH), ph)          # every query against every table row
        rel = j - (q0 + i) + Tk - 1
        assert int(rel.min()) >= 0 and int(rel.max()) <= 2 * Tk - 2
        s = (ac + torch.gather(g, 2, rel.expand(H, Tq, Tk))) * scale
    else:
        s = torch.einsum("hid,hjd->hij", qh, kh) * scale
    hidden = (j >= Tk - k_mask_tail).expand(Tq, Tk).clone()
    if causal:
        hidden |= j > i + (Tk - Tq)
    if chunk > 0:
        hidden |= j >= ((q0 + i) // chunk + 1) * chunk
    s = s.masked_fill(hidden[None], float("-inf"))
    o = torch.einsum("hij,hjd->hid", torch.softmax(s, -1), vh)
    return o.permute(1, 0, 2).reshape(Tq, H * DH)


def ragged_ref(Q, K, V, H, scale, segs, n_out, causal=False, chunk=0, k_mask_tail=0, seg_tail=None, P=None, u=None, vb=None,
               p_tmax=0, dtype=torch.float64):
    """Ragged batch: segs[s] = (q_start, q_len, k_start, k_len) into the rows of Q / K / V.  P is the FULL table [2*p_tmax-1, H*64]
    (relative offset 0 at row p_tmax - 1), sliced per segment; seg_tail[s] replaces k_mask_tail for segment s.  Returns
    [n_out, H*64] with the segments' rows filled in and NaN everywhere else."""
    out = torch.full((n_out, H * DH), float("nan"), dtype=dtype)
    for s, (q_start, q_len, k_start, k_len) in enumerate(segs):
        Ps = None
        if P is not None:
            assert q_len == k_len, "the rel-pos form is self-attention: every query row is a key row"
            Ps = P[p_tmax - k_len: p_tmax + k_len - 1]
        tail = int(seg_tail[s]) if seg_tail is not None else k_mask_tail
        out[q_start:q_start + q_len] = attn_ref(Q[q_start:q_start + q_len], K[k_start:k_start + k_len], V[k_start:k_start + k_len],
                                                H, scale, causal, chunk, 0, tail, Ps, u, vb, dtype)
    return out


def anc_ref(Q, K, V, H, scale, segs, anc, anc_ld, anc_slots, n_out, causal=False, k_mask_tail=0, seg_tail=None,
            dtype=torch.float64):
    """Ancestry form of the beam search: K / V are [anc_slots * anc_ld, H*64] (slot-major, one row per cache position); key / value
    j of segment z is row min(anc[z*anc_ld + k0 + j], anc_slots - 1) * anc_ld + k0 + j, k0 = the segment's k_start.  ``anc`` is a
    flat sequence of non-negative slot ids."""
    out = torch.full((n_out, H * DH), float("nan"), dtype=dtype)
    for z, (q_start, q_len, k0, k_len) in enumerate(segs):
        rows = torch.tensor([min(int(anc[z * anc_ld + k0 + j]), anc_slots - 1) * anc_ld + k0 + j for j in range(k_len)],
                            dtype=torch.long)
        tail = int(seg_tail[z]) if seg_tail is not None else k_mask_tail
        out[q_start:q_start + q_len] = attn_ref(Q[q_start:q_start + q_len], K[rows], V[rows], H, scale, causal, 0, 0, tail,
                                                dtype=dtype)
    return out


def pool_ref(Qs, cache, H, scale, sess, P, u, vb, p_tmax, slot_rows, n_out, dtype=torch.float64):
    """Tail-query rel-pos attention of many streaming sessions.  Qs [rows, 3*H*64] stacked q|k|v rows, cache
    [slots * slot_rows, 3*H*64]; sess[z] = (q_start, n, r0, T2, slot, chunk): the session's n query rows are absolute positions
    r0 .. T2 - 1, keys 0 .. r0 - 1 come from its slot's cache rows, keys r0 .. T2 - 1 from the stacked rows.  Returns (the outputs
    [n_out, H*64], NaN outside the sessions' rows; the cache after the call: the stacked rows copied to rows r0 .. of the slot)."""
    D = H * DH
    out = torch.full((n_out, D), float("nan"), dtype=dtype)
    cache_after = cache.clone()
    for (q_start, n, r0, T2, slot, chunk) in sess:
        assert T2 == r0 + n and T2 <= slot_rows
        new = Qs[q_start:q_start + n]
        old = cache[slot * slot_rows: slot * slot_rows + r0]
        k = torch.cat([old[:, D:2 * D], new[:, D:2 * D]])
        v = torch.cat([old[:, 2 * D:], new[:, 2 * D:]])
        out[q_start:q_start + n] = attn_ref(new[:, :D], k, v, H, scale, False, chunk, r0, 0, P[p_tmax - T2: p_tmax + T2 - 1], u, vb,
                                            dtype)
        cache_after[slot * slot_rows + r0: slot * slot_rows + T2] = new
    return out, cache_after
