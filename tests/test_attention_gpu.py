"""Every kernel of csrc/attention.hip, run directly (ss_op_attention_ex / ss_op_attention_pool) against the float64 references of
tests/attention_ref.py, at lengths around the tile sizes of the code (16-query and 64-query tiles, 64-key tiles, the decode
kernel's 256-key stride, the 48-row limit of the few-queries form) and with every field of AttnArgs the product sets.

Which kernel takes a launch.  The attention kernels have no profiler class (ss_prof_class_name lists the GEMM / conv tile
configurations only), so no case can read a launch counter.  Each case instead states the kernel it is written for and asserts it
against ``route()``, the routing conditions documented in csrc/attention.hpp and on launch_attention, written down once below:

  decode<ANC>          anc set (ragged, no P, max_q <= 8)                                         group 2
  decode               no P, <= 8 query rows, no_decode_kernel = 0                                group 1
  mfma                 no P, > 8 query rows or no_decode_kernel, ldq / ldo multiples of 4         group 3
  valu                 as mfma with ss_debug_attention_no_mfma(1), or ldq / ldo not aligned       group 4
  q16                  P, single utterance, <= 48 query rows, q16 hook on, one key tile or the
                       key-split scratch bound                                                    group 5
  relpos_mfma<split>   P, single utterance, scratch bound, >= 2 key tiles, split hook >= 0        group 5
  relpos_mfma          P otherwise (ragged; no scratch; one key tile)                             groups 5, 6
  valu<relpos>         P with causal or k_mask_tail, or the no_mfma hook                          groups 6, 7
  pool                 ss_op_attention_pool                                                       group 8

Data.  Normal cases use the distributions of the attention cases of test_ops_gpu.py; "peaked" cases scale q so that the scores
have a standard deviation near 4 and one wrongly visible or hidden key moves the output far beyond rounding.  Rows no kernel may
read hold NaN (guard rows around every buffer, gaps between segments, q columns of rows that are keys only, cache rows from r0
up, table rows no segment reaches); key rows inside a masked tail hold 1e4 in K and V.  Output buffers start as NaN and must be
finite on exactly the rows (and columns) the call owns.

Bounds: 5e-5 absolute against float64 (the project's bound for these kernels at this scaling); on peaked data
max(5e-5, 8 x the error of the float32 run of the same reference), see _check.
"""
import contextlib
import ctypes as C

import pytest
import torch

from tests import attention_ref as R

pytestmark = pytest.mark.gpu

TOL = 5e-5
NAN = float("nan")
BIG = 1e4            # masked key rows: finite (NaN would poison the reference too), large enough to wreck a row that sees them
G = 2                # NaN guard rows around / between everything
SS_ERR_ARG = 2


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def at(t, row=0, col=0):
    """Device address of element (row, col) of a contiguous 2-D (or 1-D) float32 / int32 tensor."""
    assert t.is_cuda and t.is_contiguous()
    ld = t.stride(0) if t.dim() == 2 else 1
    return t.data_ptr() + 4 * (row * ld + col)


def i32(x):
    return torch.tensor(x, dtype=torch.int32).reshape(-1).cuda()


def cdiv(a, b):
    return (a + b - 1) // b


@contextlib.contextmanager
def hooks(lib, q16=1, split=0, no_mfma=0):
    """Debug hooks for the duration of a block; back at the values every other suite expects whatever happens inside."""
    try:
        lib.ss_debug_attention_q16(q16)
        lib.ss_debug_attention_split(split)
        lib.ss_debug_attention_no_mfma(no_mfma)
        yield
    finally:
        lib.ss_debug_attention_split(0)
        lib.ss_debug_attention_q16(1)
        lib.ss_debug_attention_no_mfma(0)


def route(f, H, q16=1, split=0, no_mfma=0):
    """The kernel launch_attention documents for the fields ``f`` under the given hooks (attention.hpp, launch_attention)."""
    P, nseg = f.get("P"), f.get("nseg", 0)
    tq = f.get("max_q", 0) if nseg > 0 else f["Tq"]
    q0, causal, tail = f.get("q0", 0), f.get("causal", 0), f.get("k_mask_tail", 0)
    aligned = ((f["ldq"] | f["ldo"]) & 3) == 0
    if f.get("anc"):
        return "decode<anc>"
    if not P and tq <= 8 and q0 == 0 and not f.get("no_decode_kernel", 0):
        return "decode"
    if not P:
        return "mfma" if (q0 == 0 and not no_mfma and aligned) else "valu"
    if no_mfma or not aligned or tail or causal:
        return "valu<relpos>"
    nqt, nkt = cdiv(tq, 64), cdiv(f["Tk"], 64) if nseg == 0 else 0
    bound = f.get("use_split", 0)
    if nseg == 0 and tq <= 48 and q16 and (nkt == 1 or (bound and cdiv(tq, 16) * H * nkt <= 512)):
        return "q16"
    if nseg == 0 and bound and split >= 0 and nkt >= 2 and nqt * H < 128:
        tps = split if split > 0 else cdiv(nkt, min(16, max(1, 256 // (nqt * H))))
        tps = max(tps, cdiv(nkt, 16))
        if cdiv(nkt, tps) >= 2 and nqt * H * cdiv(nkt, tps) <= 512:
            return "relpos_mfma<split>"
    return "relpos_mfma"


def launch(lib, **f):
    """One ss_op_attention_ex call; pointer fields are device addresses (``at``).  Returns the launcher's return code."""
    from streamspeech_amd import lib as L
    a = L.SSOpAttnArgs()
    for k, v in f.items():
        assert hasattr(a, k), k
        setattr(a, k, v)
    rc = lib.ss_op_attention_ex(S(), C.byref(a))
    torch.cuda.synchronize()
    return rc


def _check(tag, out, ref, ncols, ref32=None, tol=TOL):
    """``out`` (device, started as NaN) against ``ref`` (float64, NaN on the rows the call does not own): finite on exactly the
    owned rows and the first ncols columns, within ``tol`` of the reference there.  With ``ref32`` (the float32 run of the same
    reference: peaked data) the bound is max(tol, 8 x ref32's own error): 8 covers the difference in summation order between a
    64-key tiled online softmax and a single pass.  Returns the error.

    First run on an MI355X, worst case per kernel over all cases of this file (kernel error on normal data; on peaked data: kernel
    error, error of the float32 reference, largest kernel / float32-reference ratio of a single case):
      decode              1.3e-6   2.0e-6  4.6e-6  1.4        q16                 9.8e-7   4.3e-6  5.9e-6  1.8
      decode<anc>         1.4e-6   2.1e-6  5.2e-6  0.8        relpos_mfma         1.4e-6   4.6e-6  5.9e-6  1.8
      mfma                3.9e-6   6.8e-6  6.6e-6  3.6        relpos_mfma<split>  1.4e-6   4.4e-6  5.9e-6  1.8
      valu                4.0e-6   6.2e-6  6.3e-6  1.0        valu<relpos>        1.5e-6   5.7e-6  5.4e-6  1.1
      pool                9.0e-7   3.5e-6  4.3e-6  2.2
    so every peaked case sits under the 5e-5 floor and the 8 x term has not been needed yet."""
    out = out.detach().cpu()
    own = ~torch.isnan(ref[:, 0])
    assert own.any() and torch.isfinite(ref[own]).all(), f"{tag}: the reference has a fully masked row (a bad case, not a kernel bug)"
    assert torch.isfinite(out[own][:, :ncols]).all(), f"{tag}: non-finite output on an owned row"
    assert torch.isnan(out[~own]).all(), f"{tag}: wrote a row it does not own"
    assert torch.isnan(out[:, ncols:]).all(), f"{tag}: wrote past the head columns"
    err = float((out[own][:, :ncols].double() - ref[own]).abs().max())
    bound, e32 = tol, None
    if ref32 is not None:
        e32 = float((ref32[own].double() - ref[own]).abs().max())
        bound = max(tol, 8 * e32)
    print(f"ATTN {tag}: err={err:.3e} ref32={'-' if e32 is None else format(e32, '.3e')} bound={bound:.3e}")
    assert err <= bound, f"{tag}: {err:.3e} > {bound:.3e} (ref32 {e32})"
    return err


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =================================================================================================
# plain attention (no P): packs of independent segments; a single utterance is a pack of one launched with nseg = 0
# =================================================================================================
HP, DP = 8, 512


class PlainPack:
    """Segments (q_len, k_len, tail) laid out in ``order`` with NaN gaps.  layout: "sep" Q / K / V in buffers of their own;
    "qkv" one buffer of q|k|v rows (the T2U encoder: self-attention, ld = 3 D); "kv" K|V in one buffer (cross-attention, ld = 2 D)."""

    def __init__(self, q_lens, k_lens, tails, seed, qscale=0.3, layout="sep", order=None):
        n = len(q_lens)
        order = list(range(n)) if order is None else order
        self.layout, self.tails = layout, list(tails)
        if layout == "qkv":
            assert list(q_lens) == list(k_lens)
        qpos = kpos = G
        self.segs = [None] * n
        for s in order:
            self.segs[s] = (qpos, q_lens[s], qpos if layout == "qkv" else kpos, k_lens[s])
            qpos += q_lens[s] + G
            kpos += k_lens[s] + G
        nq, nk = qpos, (qpos if layout == "qkv" else kpos)
        self.nq = nq
        Q, K, V = (torch.full((r, DP), NAN) for r in (nq, nk, nk))
        for s, (qs, ql, ks, kl) in enumerate(self.segs):
            Q[qs:qs + ql] = rnd(ql, DP, seed=seed + 10 * s) * qscale
            K[ks:ks + kl] = rnd(kl, DP, seed=seed + 10 * s + 1)
            V[ks:ks + kl] = rnd(kl, DP, seed=seed + 10 * s + 2)
            assert tails[s] < kl
            if tails[s]:
                K[ks + kl - tails[s]:ks + kl] = BIG
                V[ks + kl - tails[s]:ks + kl] = BIG
        self.Q, self.K, self.V = Q, K, V
        if layout == "sep":
            self.dq, self.dk, self.dv = Q.cuda(), K.cuda(), V.cuda()
            self.f = dict(ldq=DP, ldk=DP, ldv=DP)
            self.cols = (0, 0, 0)
        elif layout == "qkv":
            self.dq = self.dk = self.dv = torch.cat([Q, K, V], 1).cuda()
            self.f = dict(ldq=3 * DP, ldk=3 * DP, ldv=3 * DP)
            self.cols = (0, DP, 2 * DP)
        else:
            self.dq = Q.cuda()
            self.dk = self.dv = torch.cat([K, V], 1).cuda()
            self.f = dict(ldq=DP, ldk=2 * DP, ldv=2 * DP)
            self.cols = (0, 0, DP)

    def fields(self, out, ragged, causal=0, seg_tail=True, max_q=None, no_decode=0):
        """AttnArgs fields of the launch and the things that must outlive it.  ragged = False: the pack's only segment as a single
        utterance (scalar k_mask_tail); ragged with seg_tail = False: the scalar k_mask_tail for every segment (equal tails)."""
        f = dict(self.f, ldo=out.stride(0), H=HP, scale=1.0, causal=causal, no_decode_kernel=no_decode)
        keep = []
        if not ragged:
            (qs, ql, ks, kl), = self.segs
            f.update(Q=at(self.dq, qs, self.cols[0]), K=at(self.dk, ks, self.cols[1]), V=at(self.dv, ks, self.cols[2]),
                     O=at(out, qs), Tq=ql, Tk=kl, k_mask_tail=self.tails[0])
        else:
            dsegs = i32(self.segs)
            keep.append(dsegs)
            f.update(Q=at(self.dq, 0, self.cols[0]), K=at(self.dk, 0, self.cols[1]), V=at(self.dv, 0, self.cols[2]), O=at(out),
                     segs=at(dsegs), nseg=len(self.segs), max_q=max_q or max(s[1] for s in self.segs))
            if seg_tail:
                dtail = i32(self.tails)
                keep.append(dtail)
                f.update(seg_tail=at(dtail), k_mask_tail=3)        # the scalar is ignored when seg_tail is set
            else:
                assert len(set(self.tails)) == 1
                f.update(k_mask_tail=self.tails[0])
        return f, keep

    def ref(self, causal=0, dtype=torch.float64):
        return R.ragged_ref(self.Q, self.K, self.V, HP, 1.0, self.segs, self.nq, bool(causal), seg_tail=self.tails, dtype=dtype)

    def run(self, lib, tag, kernel, ragged, causal=0, seg_tail=True, max_q=None, no_decode=0, ldo=DP, peaked=False, no_mfma=0):
        out = torch.full((self.nq, ldo), NAN, device="cuda")
        f, keep = self.fields(out, ragged, causal, seg_tail, max_q, no_decode)
        assert route(f, HP, no_mfma=no_mfma) == kernel, (tag, route(f, HP, no_mfma=no_mfma))
        with hooks(lib, no_mfma=no_mfma):
            rc = launch(lib, **f)
        assert rc == 0, f"{tag}: rc {rc}"
        ref32 = self.ref(causal, torch.float32) if peaked else None
        _check(f"{kernel} {tag}", out, self.ref(causal), DP, ref32)
        del keep
        return out


PEAK_PLAIN = 0.5      # q . k over 64 dims with unit k: score std 8 * 0.5 = 4


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 255, 256, 257, 700, 1030])
def test_decode_kernel_single(lib, Tk, peaked):
    """Group 1, attention_decode_kernel<false>, one utterance: every wave count of the four-wave key split (Tk up to 64: one wave;
    65..128: two; past 256: a wave's second tile) and the LDS merge of the waves' partial (m, l, acc)."""
    cases = [(Tq, causal, tail) for Tq in (1, 3, 8) for causal in (0, 1) for tail in (0, 1, 5)
             if tail < Tk and not (causal and Tk < Tq)]          # every query row keeps a visible key (key 0)
    for Tq, causal, tail in cases:
        p = PlainPack([Tq], [Tk], [tail], seed=100 + Tk, qscale=PEAK_PLAIN if peaked else 0.3)
        p.run(lib, f"single Tq={Tq} Tk={Tk} causal={causal} tail={tail} peaked={peaked}", "decode", False, causal, peaked=peaked)


_DEC_PACKS = {
    1: ([5], [300], [4]),
    3: ([1, 8, 3], [65, 255, 64], [0, 7, 1]),
    7: ([1, 2, 8, 4, 1, 7, 3], [63, 64, 65, 255, 256, 257, 700], [0, 5, 0, 60, 1, 0, 130]),
}


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("nseg", [1, 3, 7])
def test_decode_kernel_ragged(lib, nseg, causal, peaked):
    """Group 1, ragged: mixed q_len 1..8 and k_len on both sides of 64 and 256 in one launch, segments stored out of order with
    gaps, seg_tail 0 and non-zero side by side; then the scalar k_mask_tail for every segment."""
    ql, kl, tails = _DEC_PACKS[nseg]
    order = list(reversed(range(nseg)))
    p = PlainPack(ql, kl, tails, seed=300 + nseg, qscale=PEAK_PLAIN if peaked else 0.3, order=order)
    p.run(lib, f"ragged nseg={nseg} causal={causal} seg_tail peaked={peaked}", "decode", True, causal, peaked=peaked)
    p = PlainPack(ql, kl, [5] * nseg, seed=320 + nseg, qscale=PEAK_PLAIN if peaked else 0.3, order=order)
    p.run(lib, f"ragged nseg={nseg} causal={causal} scalar tail peaked={peaked}", "decode", True, causal, seg_tail=False, max_q=8,
          peaked=peaked)


# ---- group 2: the ancestry form ----
def _anc_case(slots, ld, k0, kind, seed, qscale=0.3):
    g = torch.Generator().manual_seed(seed)
    nseg = slots
    room = ld - k0
    special = [v for v in (63, 64, 65, 255, 256, 257, room) if v <= room]
    k_lens = [special[z % len(special)] if z % 2 == 0 else int(torch.randint(1, room + 1, (1,), generator=g)) for z in range(nseg)]
    q_lens = [(1, 2, 1, 8, 3)[z % 5] for z in range(nseg)]
    tails = [0 if z % 3 else min(k_lens[z] - 1, (0, 2, 9)[z % 9 // 3]) for z in range(nseg)]
    if kind == "identity":
        anc = torch.arange(nseg)[:, None].expand(nseg, ld).clone()
    elif kind == "perm":               # one fixed permutation of the slots per position
        anc = torch.stack([torch.randperm(slots, generator=g) for _ in range(ld)], 1)
    else:                              # any slot at any position; "clamp": some ids past the last slot
        anc = torch.randint(0, slots, (nseg, ld), generator=g)
        if kind == "clamp":
            over = torch.rand(nseg, ld, generator=g) < 0.2
            anc = torch.where(over, slots + torch.randint(0, 5, (nseg, ld), generator=g), anc)
            anc[0, k0] = slots + 3     # at least one, on a key every case reads
    qpos, segs = G, []
    for z in range(nseg):
        segs.append((qpos, q_lens[z], k0, k_lens[z]))
        qpos += q_lens[z] + G
    Q = torch.full((qpos, DP), NAN)
    for (qs, ql, _, _), z in zip(segs, range(nseg)):
        Q[qs:qs + ql] = rnd(ql, DP, seed=seed + 7 * z) * qscale
    K, V = torch.full((slots * ld, DP), NAN), torch.full((slots * ld, DP), NAN)
    used = torch.zeros(slots * ld, dtype=torch.bool)         # only the rows some segment's table names hold data
    for z, (_, _, _, kl) in enumerate(segs):
        for j in range(kl):
            used[min(int(anc[z, k0 + j]), slots - 1) * ld + k0 + j] = True
    K[used] = rnd(int(used.sum()), DP, seed=seed + 1)
    V[used] = rnd(int(used.sum()), DP, seed=seed + 2)
    return Q, K, V, segs, tails, anc.reshape(-1).tolist()


@pytest.mark.parametrize("kind", ["identity", "perm", "random", "clamp"])
@pytest.mark.parametrize("k0", [0, 7])
@pytest.mark.parametrize("slots,ld", [(5, 40), (20, 300)])
def test_decode_kernel_ancestry(lib, slots, ld, k0, kind):
    """Group 2, attention_decode_kernel<true>: key j of segment z from the slot its table names, at cache position k0 + j.  Normal
    and peaked data.  The identity table must reproduce the bits of the plain ragged form on the same buffers (attention.hpp)."""
    for peaked in (False, True):
        Q, K, V, segs, tails, anc = _anc_case(slots, ld, k0, kind, seed=500 + slots + k0, qscale=PEAK_PLAIN if peaked else 0.3)
        dq, dk, dv, dsegs, dtail, danc = Q.cuda(), K.cuda(), V.cuda(), i32(segs), i32(tails), i32(anc)
        out = torch.full((Q.shape[0], DP), NAN, device="cuda")
        f = dict(Q=at(dq), K=at(dk), V=at(dv), O=at(out), ldq=DP, ldk=DP, ldv=DP, ldo=DP, H=HP, scale=1.0, segs=at(dsegs),
                 nseg=len(segs), max_q=8, seg_tail=at(dtail), anc=at(danc), anc_ld=ld, anc_slots=slots)
        assert route(f, HP) == "decode<anc>"
        assert launch(lib, **f) == 0
        kw = dict(seg_tail=tails)
        ref = R.anc_ref(Q, K, V, HP, 1.0, segs, anc, ld, slots, Q.shape[0], **kw)
        ref32 = R.anc_ref(Q, K, V, HP, 1.0, segs, anc, ld, slots, Q.shape[0], dtype=torch.float32, **kw) if peaked else None
        _check(f"decode<anc> slots={slots} ld={ld} k0={k0} {kind} peaked={peaked}", out, ref, DP, ref32)
        if kind == "identity":
            plain = [(qs, ql, z * ld + ks, kl) for z, (qs, ql, ks, kl) in enumerate(segs)]
            dplain = i32(plain)
            out2 = torch.full_like(out, NAN)
            g = dict(f, O=at(out2), segs=at(dplain))
            del g["anc"], g["anc_ld"], g["anc_slots"]
            assert route(g, HP) == "decode"
            assert launch(lib, **g) == 0
            assert _same_bits(out, out2), "an identity table must give the bits of the plain form"


def test_ancestry_refusals(lib):
    """launch_attention refuses the ancestry form outside the ragged decode kernel: SS_ERR_ARG, nothing launched."""
    Q, K, V, segs, tails, anc = _anc_case(5, 40, 0, "identity", seed=900)
    dq, dk, dv, dsegs, danc = Q.cuda(), K.cuda(), V.cuda(), i32(segs), i32(anc)
    dP, du = rnd(79, DP, seed=1).cuda(), rnd(DP, seed=2).cuda()
    out = torch.full((Q.shape[0], DP), NAN, device="cuda")
    ok = dict(Q=at(dq), K=at(dk), V=at(dv), O=at(out), ldq=DP, ldk=DP, ldv=DP, ldo=DP, H=HP, scale=1.0, segs=at(dsegs),
              nseg=len(segs), max_q=8, anc=at(danc), anc_ld=40, anc_slots=5)
    for name, bad in [("max_q > 8", dict(max_q=9)), ("P set", dict(P=at(dP), ldp=DP, bias_u=at(du), bias_v=at(du), p_tmax=40)),
                      ("nseg == 0", dict(nseg=0, segs=None, Tq=1, Tk=5)), ("no_decode_kernel", dict(no_decode_kernel=1)),
                      ("anc_ld <= 0", dict(anc_ld=0)), ("anc_slots <= 0", dict(anc_slots=0))]:
        assert launch(lib, **dict(ok, **bad)) == SS_ERR_ARG, name
    assert torch.isnan(out).all()
    assert launch(lib, **ok) == 0          # the unmodified call is a valid one
    _check("decode<anc> refusals' base case", out, R.anc_ref(Q, K, V, HP, 1.0, segs, anc, 40, 5, Q.shape[0]), DP)


# ---- group 3: the MFMA kernel ----
_MFMA_SHAPES = [(9, 9), (64, 64), (65, 65), (130, 130), (525, 525), (50, 21), (200, 1000), (3, 40)]


def _mfma_masks(Tq, Tk):
    """causal needs Tk >= Tq, a tail must leave a key: then key 0 is visible to every query row"""
    return [(causal, tail) for causal in (0, 1) for tail in (0, 1, 70) if tail < Tk and not (causal and Tk < Tq)]


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("Tq,Tk", _MFMA_SHAPES)
def test_mfma_kernel_single(lib, Tq, Tk, peaked):
    """Group 3, attention_mfma_kernel, one utterance: causal and key-tail masks (a tail of 70 crosses a key tile), query counts at
    and past the 64-row workgroup, (3, 40) forced onto the kernel by no_decode_kernel."""
    for causal, tail in _mfma_masks(Tq, Tk):
        p = PlainPack([Tq], [Tk], [tail], seed=700 + Tq, qscale=PEAK_PLAIN if peaked else 0.3)
        p.run(lib, f"single Tq={Tq} Tk={Tk} causal={causal} tail={tail} peaked={peaked}", "mfma", False, causal,
              no_decode=1 if Tq <= 8 else 0, peaked=peaked)


_MFMA_PACKS = {
    "sep": ([9, 64, 65, 130, 3, 50, 200], [9, 64, 65, 130, 40, 121, 1000], [0, 1, 0, 70, 5, 0, 70]),
    "qkv": ([9, 64, 65, 130, 525, 17], [9, 64, 65, 130, 525, 17], [0, 63, 1, 70, 0, 16]),
    "kv": ([12, 70, 3, 128], [21, 300, 40, 192], [1, 0, 39, 70]),
}


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("layout", ["sep", "qkv", "kv"])
def test_mfma_kernel_ragged(lib, layout, causal, peaked):
    """Group 3, ragged with per-segment tails: separate buffers, the T2U layout (q|k|v rows of one buffer, ld = 3 D) and the
    cross-attention layout (k|v rows, ld = 2 D); max_q as the pack has it and far past every q_len (workgroups that must return
    early); no_decode_kernel as the pack-invariant T2U path sets it."""
    ql, kl, tails = _MFMA_PACKS[layout]
    order = [3, 0, 5, 1, 6, 2, 4] if layout == "sep" else list(reversed(range(len(ql))))
    p = PlainPack(ql, kl, tails, seed=800, qscale=PEAK_PLAIN if peaked else 0.3, layout=layout, order=order)
    a = p.run(lib, f"ragged {layout} causal={causal} peaked={peaked}", "mfma", True, causal, no_decode=1, peaked=peaked)
    b = p.run(lib, f"ragged {layout} causal={causal} max_q=+200 peaked={peaked}", "mfma", True, causal, no_decode=1,
              max_q=max(ql) + 200, peaked=peaked)
    assert _same_bits(a, b), "idle workgroups must not change a bit"


def test_mfma_kernel_ragged_small_queries_keep_the_kernel(lib):
    """no_decode_kernel = 1 with every q_len <= 8 (a T2U pack of short rows): still the MFMA kernel, same numbers."""
    p = PlainPack([3, 8, 1], [40, 8, 65], [2, 0, 64], seed=850, layout="sep")
    p.run(lib, "ragged q<=8 no_decode_kernel", "mfma", True, 0, no_decode=1)


# ---- group 4: the VALU kernel, plain ----
_VALU_CASES = [(9, 9, 0, 0), (65, 65, 1, 0), (65, 65, 0, 1), (130, 130, 1, 70), (130, 130, 0, 70), (50, 21, 0, 1), (200, 1000, 1, 70),
               (3, 40, 1, 5), (64, 64, 1, 1)]


@pytest.mark.parametrize("how", ["no_mfma", "ldo514"])
@pytest.mark.parametrize("Tq,Tk,causal,tail", _VALU_CASES)
def test_valu_kernel_plain(lib, Tq, Tk, causal, tail, how):
    """Group 4, attention_kernel<false>: through the no_mfma hook and, on its own, through an output stride of 514 floats (not a
    multiple of 4: the launcher's own route to it).  Against float64 and against the MFMA kernel (1e-5)."""
    p = PlainPack([Tq], [Tk], [tail], seed=1000 + Tq)
    nd = 1 if Tq <= 8 else 0
    if how == "no_mfma":
        v = p.run(lib, f"single no_mfma Tq={Tq} Tk={Tk} causal={causal} tail={tail}", "valu", False, causal, no_decode=nd, no_mfma=1)
    else:
        v = p.run(lib, f"single ldo=514 Tq={Tq} Tk={Tk} causal={causal} tail={tail}", "valu", False, causal, no_decode=nd, ldo=514)
    m = p.run(lib, f"single (pair of the VALU case) Tq={Tq} Tk={Tk} causal={causal} tail={tail}", "mfma", False, causal, no_decode=nd)
    own = slice(G, G + Tq)
    d = float((v[own, :DP] - m[own]).abs().max())
    assert d <= 1e-5, f"VALU against MFMA: {d:.3e}"


@pytest.mark.parametrize("how", ["no_mfma", "ldo514"])
def test_valu_kernel_plain_ragged(lib, how):
    """Group 4, ragged with per-segment tails and idle workgroups; normal data also against the MFMA kernel (1e-5)."""
    ql, kl, tails = _MFMA_PACKS["sep"]
    kw = dict(no_mfma=1) if how == "no_mfma" else dict(ldo=514)
    p = PlainPack(ql, kl, tails, seed=1100, order=[3, 0, 5, 1, 6, 2, 4])
    v = p.run(lib, f"ragged {how}", "valu", True, 0, no_decode=1, max_q=max(ql) + 40, **kw)
    m = p.run(lib, "ragged (pair of the VALU case)", "mfma", True, 0, no_decode=1)
    own = ~torch.isnan(m[:, 0])
    d = float((v[own][:, :DP] - m[own]).abs().max())
    assert d <= 1e-5, f"VALU against MFMA: {d:.3e}"
    p = PlainPack(ql, kl, tails, seed=1150, qscale=PEAK_PLAIN, order=[3, 0, 5, 1, 6, 2, 4])
    p.run(lib, f"ragged {how} causal peaked", "valu", True, 1, no_decode=1, peaked=True, **kw)


# =================================================================================================
# rel-pos attention (P set): q|k|v rows of one buffer (ld = 768), H = 4
# =================================================================================================
HR, DR = 4, 256
PEAK_REL = 2.8        # (q . k + q . p) / 8 with unit k, p: score std sqrt(2) * 8 * 2.8 / 8 = 4


class RelSingle:
    """One utterance of Tk rows; the last Tq of them are the query rows (q0 = Tk - Tq).  q columns of the rows below q0 hold NaN:
    they are keys only.  The table is [2 Tk - 1] rows in the middle 256 columns of a 768-wide buffer (ldp = 768), NaN around."""

    def __init__(self, Tq, Tk, seed, qscale=1.0, tail=0):
        self.Tq, self.Tk, self.q0 = Tq, Tk, Tk - Tq
        qkv = torch.full((Tk + 2 * G, 3 * DR), NAN)
        body = rnd(Tk, 3 * DR, seed=seed)
        body[:, :DR] *= qscale
        body[:self.q0, :DR] = NAN
        if tail:
            body[Tk - tail:, DR:] = BIG
        qkv[G:G + Tk] = body
        Pt = torch.full((2 * Tk - 1 + 2 * G, 3 * DR), NAN)
        Pt[G:G + 2 * Tk - 1, DR:2 * DR] = rnd(2 * Tk - 1, DR, seed=seed + 1)
        self.body, self.Pt = body, Pt[G:G + 2 * Tk - 1, DR:2 * DR].contiguous()
        self.u, self.vb = rnd(DR, seed=seed + 2) * 0.3, rnd(DR, seed=seed + 3) * 0.3
        self.dqkv, self.dP, self.du, self.dv = qkv.cuda(), Pt.cuda(), self.u.cuda(), self.vb.cuda()

    def fields(self, out, chunk, use_split, causal=0, tail=0):
        return dict(Q=at(self.dqkv, G + self.q0, 0), K=at(self.dqkv, G, DR), V=at(self.dqkv, G, 2 * DR), O=at(out, G),
                    ldq=3 * DR, ldk=3 * DR, ldv=3 * DR, ldo=out.stride(0), Tq=self.Tq, Tk=self.Tk, H=HR, scale=0.125, causal=causal,
                    chunk=chunk, q0=self.q0, k_mask_tail=tail, P=at(self.dP, G, DR), ldp=3 * DR, bias_u=at(self.du),
                    bias_v=at(self.dv), use_split=use_split)

    def ref(self, chunk, causal=0, tail=0, dtype=torch.float64):
        b = self.body
        o = R.attn_ref(b[self.q0:, :DR], b[:, DR:2 * DR], b[:, 2 * DR:], HR, 0.125, bool(causal), chunk, self.q0, tail, self.Pt,
                       self.u, self.vb, dtype)
        full = torch.full((self.Tq + 2 * G, DR), NAN, dtype=dtype)
        full[G:G + self.Tq] = o
        return full

    def run(self, lib, tag, kernel, chunk, use_split, q16=1, split=0, no_mfma=0, causal=0, tail=0, peaked=False):
        """Two launches of the same call: the second must reproduce the first bit for bit (the arrival counters of the key-split
        hand-off are back at zero)."""
        outs = []
        with hooks(lib, q16=q16, split=split, no_mfma=no_mfma):
            for _ in range(2):
                out = torch.full((self.Tq + 2 * G, DR), NAN, device="cuda")
                f = self.fields(out, chunk, use_split, causal, tail)
                assert route(f, HR, q16, split, no_mfma) == kernel, (tag, route(f, HR, q16, split, no_mfma))
                assert launch(lib, **f) == 0, tag
                outs.append(out)
        assert _same_bits(outs[0], outs[1]), f"{tag}: a repeated launch changed bits"
        ref32 = self.ref(chunk, causal, tail, torch.float32) if peaked else None
        _check(f"{kernel} {tag}", outs[0], self.ref(chunk, causal, tail), DR, ref32)
        return outs[0]


def _rel_routes(Tq, Tk):
    """(q16 hook, use_split) -> the kernel the launcher documents for a single utterance of H = 4."""
    nkt = cdiv(Tk, 64)
    few = Tq <= 48
    return [
        (1, 1, "q16" if few else ("relpos_mfma<split>" if nkt >= 2 else "relpos_mfma")),
        (0, 1, "relpos_mfma<split>" if nkt >= 2 else "relpos_mfma"),
        (0, 0, "relpos_mfma"),
        (1, 0, "q16" if few and nkt == 1 else "relpos_mfma"),
    ]


@pytest.mark.parametrize("T,chunk", [(21, 0), (21, 8), (125, 0), (125, 16), (200, 8), (64, 0), (65, 24), (1, 0), (16, 8), (17, 16),
                                     (33, 8), (48, 0), (48, 24), (49, 0), (49, 16), (449, 24)])
def test_relpos_single_full(lib, T, chunk):
    """Group 5, q0 = 0 (every row a query): the lengths of test_relpos_attention, 49 (the first past the few-queries form) and 449,
    on every kernel the hooks can route the call to."""
    c = RelSingle(T, T, seed=1200 + T)
    outs = {}
    for q16, use_split, kernel in _rel_routes(T, T):
        outs[(q16, use_split)] = c.run(lib, f"T={T} chunk={chunk} q16={q16} use_split={use_split}", kernel, chunk, use_split, q16=q16)
    d = max(float((o - outs[(0, 0)])[G:G + T].abs().max()) for o in outs.values())
    assert d <= 2e-5, f"kernels against the serial walk: {d:.3e}"


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("Tk", [48, 64, 65, 200, 449])
@pytest.mark.parametrize("Tq", [1, 15, 16, 17, 48, 49])
def test_relpos_single_tail_queries(lib, Tq, Tk, peaked):
    """Group 5, q0 = Tk - Tq > 0 (the incremental streaming encoder: the last rows as queries over all keys), chunk 0 / 8 / 16 / 24,
    on attention_relpos_q16_kernel, on the tile kernel with and without the key split, and on the serial walk."""
    if Tq > Tk:
        Tk = Tq               # (49, 48) has no meaning; (49, 49) is q0 = 0 at the first size past the few-queries form
    c = RelSingle(Tq, Tk, seed=1300 + 7 * Tq + Tk, qscale=PEAK_REL if peaked else 1.0)
    for chunk in (0, 8, 16, 24):
        for q16, use_split, kernel in _rel_routes(Tq, Tk):
            c.run(lib, f"Tq={Tq} Tk={Tk} q0={Tk - Tq} chunk={chunk} q16={q16} use_split={use_split} peaked={peaked}", kernel, chunk,
                  use_split, q16=q16, peaked=peaked)


def test_relpos_single_forced_split_sizes(lib):
    """Group 5: key tiles per split forced to 1 and 3 (ss_debug_attention_split) with tail queries."""
    c = RelSingle(40, 449, seed=1400)
    for split in (1, 3):
        c.run(lib, f"Tq=40 Tk=449 split={split}", "relpos_mfma<split>", 16, 1, q16=0, split=split)
    c.run(lib, "Tq=40 Tk=449 split=-1", "relpos_mfma", 16, 1, q16=0, split=-1)


class RelPack:
    """Ragged rel-pos self-attention: segments of q|k|v rows in one buffer, the FULL table of p_tmax = 1024 (2047 rows; rows no
    segment of the pack can reach hold NaN)."""
    TMAX = 1024

    def __init__(self, lens, seed, qscale=1.0, tail=0, order=None):
        order = list(range(len(lens))) if order is None else order
        pos, self.segs = G, [None] * len(lens)
        for s in order:
            self.segs[s] = (pos, lens[s], pos, lens[s])
            pos += lens[s] + G
        self.n = pos
        buf = torch.full((pos, 3 * DR), NAN)
        for s, (st, ln, _, _) in enumerate(self.segs):
            body = rnd(ln, 3 * DR, seed=seed + 5 * s)
            body[:, :DR] *= qscale
            if tail:
                assert tail < ln
                body[ln - tail:, DR:] = BIG
            buf[st:st + ln] = body
        self.buf = buf
        m = max(lens)
        P = torch.full((2 * self.TMAX - 1, DR), NAN)
        P[self.TMAX - m: self.TMAX + m - 1] = rnd(2 * m - 1, DR, seed=seed + 1)
        self.P = P
        self.u, self.vb = rnd(DR, seed=seed + 2) * 0.3, rnd(DR, seed=seed + 3) * 0.3
        self.d = buf.cuda(), P.cuda(), self.u.cuda(), self.vb.cuda(), i32(self.segs)

    def fields(self, out, chunk, max_q=None, causal=0, tail=0):
        dbuf, dP, du, dv, dsegs = self.d
        return dict(Q=at(dbuf, 0, 0), K=at(dbuf, 0, DR), V=at(dbuf, 0, 2 * DR), O=at(out), ldq=3 * DR, ldk=3 * DR, ldv=3 * DR,
                    ldo=out.stride(0), H=HR, scale=0.125, causal=causal, chunk=chunk, k_mask_tail=tail, P=at(dP), ldp=DR,
                    bias_u=at(du), bias_v=at(dv), segs=at(dsegs), nseg=len(self.segs), max_q=max_q or max(s[1] for s in self.segs),
                    p_tmax=self.TMAX, use_split=1)

    def ref(self, chunk, causal=0, tail=0, dtype=torch.float64):
        b = self.buf
        return R.ragged_ref(b[:, :DR], b[:, DR:2 * DR], b[:, 2 * DR:], HR, 0.125, self.segs, self.n, bool(causal), chunk, tail, None,
                            self.P, self.u, self.vb, self.TMAX, dtype)

    def run(self, lib, tag, kernel, chunk, no_mfma=0, max_q=None, causal=0, tail=0, peaked=False):
        out = torch.full((self.n, DR), NAN, device="cuda")
        f = self.fields(out, chunk, max_q, causal, tail)
        assert route(f, HR, no_mfma=no_mfma) == kernel, (tag, route(f, HR, no_mfma=no_mfma))
        with hooks(lib, no_mfma=no_mfma):
            assert launch(lib, **f) == 0, tag
        ref32 = self.ref(chunk, causal, tail, torch.float32) if peaked else None
        _check(f"{kernel} {tag}", out, self.ref(chunk, causal, tail), DR, ref32)
        return out


_REL_PACKS = {1: [449], 2: [65, 1], 6: [1, 449, 64, 17, 200, 129]}


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("chunk", [0, 16])
@pytest.mark.parametrize("nseg", [1, 2, 6])
def test_relpos_ragged(lib, nseg, chunk, peaked):
    """Group 6: segments of 1 to 449 rows in one launch, each slicing the full table at a row of its own, on
    attention_relpos_mfma_kernel<false> and (no_mfma hook) on attention_kernel<true>; the two agree to 1e-5 on normal data."""
    lens = _REL_PACKS[nseg]
    p = RelPack(lens, seed=1500 + nseg, qscale=PEAK_REL if peaked else 1.0, order=list(reversed(range(nseg))))
    m = p.run(lib, f"ragged nseg={nseg} chunk={chunk} peaked={peaked}", "relpos_mfma", chunk, peaked=peaked)
    m2 = p.run(lib, f"ragged nseg={nseg} chunk={chunk} max_q=+100 peaked={peaked}", "relpos_mfma", chunk, max_q=max(lens) + 100,
               peaked=peaked)
    assert _same_bits(m, m2)
    v = p.run(lib, f"ragged nseg={nseg} chunk={chunk} no_mfma peaked={peaked}", "valu<relpos>", chunk, no_mfma=1, peaked=peaked)
    if not peaked:
        own = ~torch.isnan(m[:, 0])
        d = float((v[own] - m[own]).abs().max())
        assert d <= 1e-5, f"VALU against MFMA: {d:.3e}"


def test_relpos_refusals(lib):
    p = RelPack([20, 33], seed=1600)
    out = torch.full((p.n, DR), NAN, device="cuda")
    ok = p.fields(out, 0)
    dtail = i32([1, 1])
    for name, bad in [("p_tmax <= 0", dict(p_tmax=0)), ("q0 != 0 with segments", dict(q0=3)), ("seg_tail with P", dict(seg_tail=at(dtail))),
                      ("ldp not a multiple of 4", dict(ldp=DR + 2)), ("no bias_u", dict(bias_u=None)), ("ldk not a multiple of 4", dict(ldk=3 * DR + 1))]:
        assert launch(lib, **dict(ok, **bad)) == SS_ERR_ARG, name
    c = RelSingle(10, 30, seed=1601)
    out1 = torch.full((10 + 2 * G, DR), NAN, device="cuda")
    f = c.fields(out1, 0, 1)
    assert launch(lib, **dict(f, q0=19)) == SS_ERR_ARG, "q0 + Tq != Tk"
    assert launch(lib, **dict(f, causal=1)) == SS_ERR_ARG, "q0 != 0 with causal"
    assert torch.isnan(out).all() and torch.isnan(out1).all()
    assert launch(lib, **ok) == 0
    _check("relpos_mfma refusals' base case", out, p.ref(0), DR)


# ---- group 7: the VALU kernel, rel-pos, by the launcher's own routing (no hook) ----
@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("T", [21, 65, 130])
def test_valu_kernel_relpos_masks(lib, T, peaked):
    """Group 7, attention_kernel<true> without a hook: rel-pos with a causal mask, with a key tail, with both and a chunk mask."""
    qs = PEAK_REL if peaked else 1.0
    for causal, tail, chunk in [(1, 0, 0), (0, 5, 0), (1, 0, 16), (0, 1, 8)]:
        c = RelSingle(T, T, seed=1700 + T, qscale=qs, tail=tail)
        c.run(lib, f"T={T} causal={causal} tail={tail} chunk={chunk} peaked={peaked}", "valu<relpos>", chunk, 1, causal=causal,
              tail=tail, peaked=peaked)
    p = RelPack([65, 9, 130], seed=1750, qscale=qs, order=[2, 0, 1])
    p.run(lib, f"ragged causal peaked={peaked}", "valu<relpos>", 0, causal=1, peaked=peaked)
    p = RelPack([65, 9, 130], seed=1760, qscale=qs, tail=4, order=[1, 2, 0])
    p.run(lib, f"ragged tail=4 chunk=16 peaked={peaked}", "valu<relpos>", 16, tail=4, peaked=peaked)


# =================================================================================================
# group 8: the pool kernel
# =================================================================================================
SLOT_ROWS, NSLOTS = 512, 12
#            n   r0  slot chunk
_SESSIONS = [(1, 0, 7, 0), (15, 3, 2, 8), (16, 48, 9, 16), (17, 100, 0, 24), (33, 0, 5, 0), (48, 401, 11, 16), (16, 200, 3, 8),
             (1, 448, 1, 24), (48, 64, 8, 16)]


class PoolCase:
    def __init__(self, seed, qscale=1.0, sessions=_SESSIONS):
        pos, self.sess = G, []
        for n, r0, slot, chunk in sessions:
            self.sess.append((pos, n, r0, r0 + n, slot, chunk))
            pos += n + G
        self.n = pos
        Qs = torch.full((pos, 3 * DR), NAN)
        cache = torch.full((NSLOTS * SLOT_ROWS, 3 * DR), NAN)
        for z, (qs, n, r0, T2, slot, _) in enumerate(self.sess):
            body = rnd(n, 3 * DR, seed=seed + 3 * z)
            body[:, :DR] *= qscale
            Qs[qs:qs + n] = body
            cache[slot * SLOT_ROWS: slot * SLOT_ROWS + r0, DR:] = rnd(r0, 2 * DR, seed=seed + 3 * z + 1)     # q columns stay NaN
        self.Qs, self.cache = Qs, cache
        P = torch.full((2 * 1024 - 1, DR), NAN)
        P[1024 - 449: 1024 + 448] = rnd(2 * 449 - 1, DR, seed=seed + 100)
        self.P, self.u, self.vb = P, rnd(DR, seed=seed + 101) * 0.3, rnd(DR, seed=seed + 102) * 0.3
        self.dQs, self.dP, self.du, self.dv = Qs.cuda(), P.cuda(), self.u.cuda(), self.vb.cuda()

    def run(self, lib, which):
        """One launch over the sessions ``which`` (indices into the case's sessions) on a fresh copy of the cache."""
        from streamspeech_amd import lib as L
        sess = [self.sess[z] for z in which]
        rec = [list(s) + [0, 0] for s in sess]
        pre = [0]
        for s in sess:
            pre.append(pre[-1] + cdiv(s[1], 16))
        dsess, dpre, dcache = i32(rec), i32(pre), self.cache.cuda()
        out = torch.full((self.n, DR), NAN, device="cuda")
        a = L.SSOpPoolAttnArgs()
        a.Qs, a.cache, a.O = at(self.dQs), at(dcache), at(out)
        a.ld, a.ldo, a.slot_rows = 3 * DR, DR, SLOT_ROWS
        a.P, a.ldp, a.p_tmax = at(self.dP), DR, 1024
        a.bias_u, a.bias_v = at(self.du), at(self.dv)
        a.sess, a.qt_pre = at(dsess), at(dpre)
        a.nsess, a.qtiles, a.H, a.scale = len(sess), pre[-1], HR, 0.125
        rc = lib.ss_op_attention_pool(S(), C.byref(a))
        torch.cuda.synchronize()
        assert rc == 0
        return out, dcache, sess

    def ref(self, sess, dtype=torch.float64):
        return R.pool_ref(self.Qs, self.cache, HR, 0.125, sess, self.P, self.u, self.vb, 1024, SLOT_ROWS, self.n, dtype)


_POOL_SUBSETS = [[z] for z in range(9)] + [[5, 0, 3], [8, 2, 6]]


@pytest.mark.parametrize("peaked", [False, True])
def test_pool_kernel(lib, peaked):
    """Group 8, attention_pool_kernel: 9, 3 and 1 sessions per launch, n 1..48, fresh sessions (r0 = 0) and sessions with up to
    448 cached rows, T2 1..449, slots out of session order, a chunk per session.  Outputs against float64; the cache afterwards
    holds the stacked rows at r0 .. and is otherwise untouched, bit for bit; a session's output bits are those of a launch without
    the other sessions."""
    c = PoolCase(seed=2000, qscale=PEAK_REL if peaked else 1.0)
    out9, cache9, sess9 = c.run(lib, list(range(9)))
    ref, cache_ref = c.ref(sess9)
    ref32 = c.ref(sess9, torch.float32)[0] if peaked else None
    _check(f"pool 9 sessions peaked={peaked}", out9, ref, DR, ref32)
    assert _same_bits(cache9.cpu(), cache_ref), "cache after the call"
    for which in _POOL_SUBSETS:
        out, dcache, sess = c.run(lib, which)
        r, cr = c.ref(sess)
        _check(f"pool sessions {which} peaked={peaked}", out, r, DR, c.ref(sess, torch.float32)[0] if peaked else None)
        assert _same_bits(dcache.cpu(), cr), f"cache after the call, sessions {which}"
        for (qs, n, *_rest) in sess:
            assert _same_bits(out[qs:qs + n], out9[qs:qs + n]), f"session at row {qs}: bits depend on the rest of the launch"


def _session_on_q16(lib, c, sess):
    """One session of a PoolCase through ss_op_attention_ex(q0 = r0) on attention_relpos_q16_kernel over the same keys (cache rows,
    then the stacked rows)."""
    qs, n, r0, T2, slot, chunk = sess
    rows = torch.cat([c.cache[slot * SLOT_ROWS: slot * SLOT_ROWS + r0], c.Qs[qs:qs + n]]).cuda()
    out = torch.full((n, DR), NAN, device="cuda")
    f = dict(Q=at(rows, r0, 0), K=at(rows, 0, DR), V=at(rows, 0, 2 * DR), O=at(out), ldq=3 * DR, ldk=3 * DR, ldv=3 * DR, ldo=DR,
             Tq=n, Tk=T2, H=HR, scale=0.125, chunk=chunk, q0=r0, P=at(c.dP, 1024 - T2), ldp=DR, bias_u=at(c.du), bias_v=at(c.dv),
             use_split=1)
    assert route(f, HR) == "q16"
    assert launch(lib, **f) == 0
    return out


def test_pool_kernel_against_the_single_session_kernel(lib):
    """Group 8: every session of the pool launch against attention_relpos_q16_kernel, 2e-5 (the two merge their key tiles in
    different orders: the last arrival's two passes against a running merge)."""
    c = PoolCase(seed=2100)
    out9, _, sess9 = c.run(lib, list(range(9)))
    for sess in sess9:
        qs, n, r0 = sess[:3]
        d = float((_session_on_q16(lib, c, sess) - out9[qs:qs + n]).abs().max())
        assert d <= 2e-5, f"session n={n} r0={r0}: pool against q16 {d:.3e}"


def test_pool_kernel_one_key_tile_has_the_bits_of_the_single_session_kernel(lib):
    """Group 8: a session whose keys fit one key tile (9 rows at r0 = 40: T2 = 49).  Neither kernel merges anything then, so the
    tile arithmetic the two share (q16_tile, csrc/attn_tile.hpp) is all there is: the same bits."""
    c = PoolCase(seed=2300, sessions=[(9, 40, 4, 0)])
    out, _, (sess,) = c.run(lib, [0])
    qs, n = sess[:2]
    assert _same_bits(out[qs:qs + n], _session_on_q16(lib, c, sess)), "pool against q16 on one key tile"


def test_pool_refusals(lib):
    from streamspeech_amd import lib as L
    c = PoolCase(seed=2200)
    out = torch.full((c.n, DR), NAN, device="cuda")
    dcache, dsess, dpre = c.cache.cuda(), i32(list(c.sess[0]) + [0, 0]), i32([0, 1])

    def call(**bad):
        a = L.SSOpPoolAttnArgs()
        f = dict(Qs=at(c.dQs), cache=at(dcache), O=at(out), ld=3 * DR, ldo=DR, slot_rows=SLOT_ROWS, P=at(c.dP), ldp=DR, p_tmax=1024,
                 bias_u=at(c.du), bias_v=at(c.dv), sess=at(dsess), qt_pre=at(dpre), nsess=1, qtiles=1, H=HR, scale=0.125)
        f.update(bad)
        for k, v in f.items():
            setattr(a, k, v)
        rc = lib.ss_op_attention_pool(S(), C.byref(a))
        torch.cuda.synchronize()
        return rc
    for name, bad in [("ld != 3 H 64", dict(ld=2 * DR)), ("p_tmax <= 0", dict(p_tmax=0)), ("slot_rows <= 0", dict(slot_rows=0)),
                      ("no sess", dict(sess=None)), ("nsess <= 0", dict(nsess=0)), ("ldo not a multiple of 4", dict(ldo=DR + 2))]:
        assert call(**bad) == SS_ERR_ARG, name
    assert torch.isnan(out).all()
    assert call(qtiles=0) == 0 and torch.isnan(out).all()       # nothing to do is not an error
    assert call() == 0
    assert torch.isfinite(out[c.sess[0][0]]).all()
