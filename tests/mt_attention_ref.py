"""Float64 restatement of the head-averaged attention probabilities kernel (csrc/attn_probs.hpp), from float32 inputs.

Written from the definition in the header, not from the kernel: per head the whole [rows, k_len] score matrix, its row maximum
subtracted, exponentiated and divided by its row sum; the heads' matrices averaged; the row arg-max by an explicit scan that keeps
the FIRST maximum (torch.max's tie rule); the two row statistics.  Head h owns columns [64 h, 64 h + 64) of every row.
tests/test_mt_attention_cpu.py pins it against torch.softmax(...).mean(heads); tests/test_mt_attention_gpu.py compares the kernel
with it.  ``dtype`` exists for the float32 run of the same arithmetic, whose distance from the float64 run is the yardstick of the
peaked-data cases.
"""
import torch

DH = 64


def probs_ref(q, k, H, scale, dtype=torch.float64):
    """q [n, H*64], k [k_len, H*64] -> P [n, k_len] = (1 / H) sum_h softmax_j(scale * q_{i,h} . k_{j,h}) in ``dtype``."""
    n, k_len = q.shape[0], k.shape[0]
    assert q.shape[1] == H * DH and k.shape[1] == H * DH and k_len >= 1
    P = torch.zeros((n, k_len), dtype=dtype)
    for h in range(H):
        qh = q[:, h * DH:(h + 1) * DH].to(dtype)
        kh = k[:, h * DH:(h + 1) * DH].to(dtype)
        # one reduction per score, not a blocked GEMM: two identical key rows must give two identical columns (the tie case)
        s = (qh[:, None, :] * kh[None, :, :]).sum(-1) * scale
        e = torch.exp(s - s.max(dim=1, keepdim=True).values)
        P += e / e.sum(dim=1, keepdim=True)
    return P / H


def peak_ref(P):
    """Row arg-max of P with the lowest index of a tie -> int64 [n]."""
    out = torch.zeros(P.shape[0], dtype=torch.int64)
    for i in range(P.shape[0]):
        best, row = 0, P[i].tolist()
        for j in range(1, len(row)):
            if row[j] > row[best]:
                best = j
        out[i] = best
    return out


def stat_ref(P, peak):
    """[n, 2] = {P[i][peak[i]], sum_j j * P[i][j]} in P's dtype."""
    j = torch.arange(P.shape[1], dtype=P.dtype)
    return torch.stack([P.gather(1, peak[:, None])[:, 0], (P * j).sum(1)], 1)


def top2_gap(P):
    """Per row the gap between the largest and the second largest entry (inf for a single column)."""
    if P.shape[1] < 2:
        return torch.full((P.shape[0],), float("inf"), dtype=P.dtype)
    t = torch.topk(P, 2, dim=1).values
    return t[:, 0] - t[:, 1]


def ragged_probs_ref(Q, K, H, scale, segs, q_first, dtype=torch.float64):
    """Ragged launch: segs[s] = (q_start, q_len, k_start, k_len) into the rows of Q / K; of segment s the query rows q_first[s] ..
    q_len - 1 are answered.  -> per segment (P [n_s, k_len], peak int64 [n_s], stat [n_s, 2])."""
    out = []
    for (q_start, q_len, k_start, k_len), f in zip(segs, q_first):
        P = probs_ref(Q[q_start + f:q_start + q_len], K[k_start:k_start + k_len], H, scale, dtype)
        pk = peak_ref(P)
        out.append((P, pk, stat_ref(P, pk)))
    return out


# ---- the op-level cases shared by tests/test_mt_attention_cpu.py (the reference alone) and tests/test_mt_attention_gpu.py ----
H_OP, D_OP = 8, 512
TOL = 5e-5            # the project's bound for the attention kernels at this scaling (tests/test_attention_gpu.py)
QSCALE = 0.3          # query rows ~ N(0, 0.3^2), key rows ~ N(0, 1): scores with a standard deviation of 2.4, as in that file
K_LENS = (1, 15, 16, 17, 33, 250, 1500)
Q_LENS = (1, 16, 17, 37)


def op_cases():
    """name -> dict(q_lens, k_lens, q_first, scale, seed, ties, focus).  ties: {segment: (j1, j2)}: key row j2 is a copy of key row
    j1 < j2 and every query row of the segment points at it, so both columns hold the row maximum (the case pins the tie rule and is
    the one case the decisive-gap rule does not apply to).  focus (the peaked cases, scores scaled by 20): at that scale every head is
    one-hot, and eight heads that look at eight different keys tie at 1 / 8, so no row would be decisive; query row i therefore
    also carries focus * key row (7 i + 3) % k_len in every head, as the alignment heads of a trained decoder agree on a frame.
    Most heads then pick that key, the others their own: rows with entries near 1, 7 / 8, ... and a few at 1 / 8."""
    cases = {}
    for k in K_LENS:      # every q_len against every k_len: one launch per k_len, a segment per q_len
        cases[f"k{k}"] = dict(q_lens=list(Q_LENS), k_lens=[k] * len(Q_LENS), q_first=[0] * len(Q_LENS), scale=1.0, seed=100 + k)
    cases["ragged3"] = dict(q_lens=[17, 37, 6], k_lens=[1, 250, 33], q_first=[0, 5, 5], scale=1.0, seed=7)
    cases["q_first"] = dict(q_lens=[37, 37, 37], k_lens=[33, 33, 33], q_first=[0, 5, 36], scale=1.0, seed=8)
    for k in (17, 250, 1500):
        cases[f"peaked_k{k}"] = dict(q_lens=[37], k_lens=[k], q_first=[0], scale=20.0, seed=200 + k, focus=0.15)
    cases["tie"] = dict(q_lens=[17, 5], k_lens=[250, 70], q_first=[0, 0], scale=1.0, seed=9, ties={0: (5, 100), 1: (3, 67)})
    return cases


def _rnd(rows, seed, scale=1.0):
    return torch.randn(rows, D_OP, generator=torch.Generator().manual_seed(seed)) * scale


def case_data(c):
    """Per segment (q [q_len, 512], k [k_len, 512]) float32 of a case of op_cases()."""
    out = []
    for s, (ql, kl) in enumerate(zip(c["q_lens"], c["k_lens"])):
        q, k = _rnd(ql, c["seed"] * 1000 + 10 * s, QSCALE), _rnd(kl, c["seed"] * 1000 + 10 * s + 1)
        if s in c.get("ties", {}):
            j1, j2 = c["ties"][s]
            k[j2] = k[j1]
            q[:] = k[j1] * 0.25 + q * 0.1
        if c.get("focus"):
            q += c["focus"] * k[[(7 * i + 3) % kl for i in range(ql)]]
        out.append((q, k))
    return out


def case_bound(c, P64, P32):
    """The bound of a case: TOL, on peaked data max(TOL, 8 x the float32 run's own error) (test_attention_gpu.py's rule)."""
    if c["scale"] == 1.0:
        return TOL
    return max(TOL, 8 * max(float((a.double() - b).abs().max()) for a, b in zip(P32, P64)))
