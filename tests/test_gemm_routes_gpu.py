"""Op-level tests of the three kernels of csrc/gemm.hip -- gemv_kernel, smallm_gemm_kernel and the LDS-tiled conv_gemm_kernel in its
default and CANON_SEQ (BLK) forms -- route by route against tests/gemm_ref.py (float64), through ss_op_ln_linear_ex, ss_op_conv_gemm_ex
and ss_op_conv_gemm_rows.  The routes with a test file of their own (rt_linear: tests/test_rtlin_gpu.py, rt_linear_kb:
tests/test_rtlin_kb_gpu.py -- both on this file's launch(); ffn_fused, stream-K, the slab / Winograd / FP16 convs, m_begin / seg_mb) and
the hook-only tuning tiles are not launched here.

The harness is that of tests/test_slab_ops_gpu.py.  Every launch of this file:
  * inputs sit between guard rows of 1e4 and padded input columns hold 1e4, so a row or column read from outside is no small error;
  * every output (C, C2, ln_out) starts as NaN with guard rows behind it and gap columns where ld > N; afterwards rc == 0, the elements
    the op is defined to write are finite and everything else is still NaN (rows >= M, gap columns, rows of no utterance, an unbound C2);
  * the census over every profiler class shows exactly one launch, of the stated class;
  * the float64 bound is TOL = 2e-4 max abs (the project's per-conv bound on this scaling: A ~ N(0, 1), W ~ (taps Cin)^-1/2), ln_out is
    held to LN_TOL = 2e-5 (tests/test_ops_gpu.py::test_layernorm).
Next to every case stands the dispatcher arithmetic of launch_conv_gemm / launch_canon (csrc/gemm.hip) that puts it on its route, the
intra-workgroup split KS included, which the census cannot show.  The accuracy table of a run: profiles/gemm_routes_accuracy.txt.
"""
import ctypes as C
import os

import pytest
import torch

from tests import gemm_ref as G
from tests import slab_ref
from test_slab_ops_gpu import (TOL, P, S, bits, census, lib, out_buf, restore, rnd, stop_after_a_gpu_error, took_since)  # noqa: F401

pytestmark = pytest.mark.gpu

for _knob in ("SS_SMALLM_MAX_ROWS", "SS_NO_RTLIN", "SS_RTLIN_MIN_ROWS", "SS_RTLIN_MIN_UNITS", "SS_SK_MIN_GFLOP"):
    if os.environ.get(_knob):
        pytestmark = [pytest.mark.gpu, pytest.mark.skip(reason=f"{_knob} is set: the dispatch thresholds are not the defaults")]

LN_TOL = 2e-5                  # ln_out against float64 LayerNorm: the bound of tests/test_ops_gpu.py::test_layernorm
DEV = "cuda:0"
EDGE = 1.0e4                   # guard rows and padded columns of every input
GUARD = 8                      # guard rows on either side of an input, behind an output
SS_ERR_ARG = 2
NONE, SILU, RELU, LRELU, TANH = G.ACT_NONE, G.ACT_SILU, G.ACT_RELU, G.ACT_LRELU, G.ACT_TANH
SMALLM = {(4, 1): "smallm_gemm<4,1>", (2, 2): "smallm_gemm<2,2>", (1, 4): "smallm_gemm<1,4>"}


def cdiv(a, b):
    return -(-a // b)


ROUTE_WORST = {}               # route -> [worst max abs error, launches] over the cases run so far


class Worst:
    """The worst error of a route over its cases; done() books it, and the module's last act is the WORST line of every route."""

    def __init__(self, route):
        self.route, self.err, self.n = route, 0.0, 0

    def add(self, err):
        self.err, self.n = max(self.err, err), self.n + 1

    def done(self):
        tot = ROUTE_WORST.setdefault(self.route, [0.0, 0])
        tot[0], tot[1] = max(tot[0], self.err), tot[1] + self.n


@pytest.fixture(scope="module", autouse=True)
def worst_table():
    yield
    print()
    for route, (err, n) in ROUTE_WORST.items():
        print(f"WORST {route}: {err:.3e} over {n} launches")


def dev_in(t, ld=None):
    """[rows, cols] -> a device buffer [GUARD + rows + GUARD, ld] of EDGE holding t; returns (buffer, pointer to its first row)."""
    rows, cols = t.shape
    ld = cols if ld is None else ld
    buf = torch.full((rows + 2 * GUARD, ld), EDGE, device=DEV)
    buf[GUARD:GUARD + rows, :cols] = t.to(DEV)
    return buf, C.c_void_p(buf.data_ptr() + GUARD * ld * 4)


def untouched(buf, mask=None):
    """Everything of the host copy `buf` outside `mask` is still NaN."""
    return bool(torch.isnan(buf if mask is None else buf[~mask]).all())


def launch(lib, cls, what, worst, *, M=None, N, Cin, taps=1, dil=1, stride=1, pad=0, in_len=None, chunk=0, in_act=NONE, ln=False,
           ln_out=False, bias=True, act=NONE, act_slope=0.1, alpha=1.0, R=False, R2=False, div=0.0, C2=False, c2_slope=0.1, glu=0,
           lda=None, ldc=None, ldr=None, ldr2=None, ldc2=None, segs=None, canon=0, entry="conv", inplace=False, seed=0, mean=0.0,
           tol=TOL, W=None, b=None, expect_rc=0, rows=None, refs=None):
    """One launch with everything the module docstring promises checked; returns the host copies (C, C2, ln_out) and the error.
    entry "lin": ss_op_ln_linear_ex (a linear, same_rows = 1 as ln_linear() of the model sets it); "conv": ss_op_conv_gemm_ex, or
    ss_op_conv_gemm_rows when canon is set (same_rows = 0: no slab / stream-K kernel is eligible).  segs: [(out_start, out_len,
    in_start, in_len)], M / in_len then the packed totals.  expect_rc = SS_ERR_ARG: the refusal -- census unchanged, nothing written.
    rows (a plain linear only): the row indices the float64 oracle is computed on, for launches whose whole reference would take the
    host many seconds; every other check still covers every element.  refs: a dict that keeps the float64 reference (and x, w) of the
    first launch it is passed to for the later ones -- the same arguments on another kernel."""
    from streamspeech_amd.lib import SSOpConvArgs
    nout = N // 2 if glu else N
    if segs is not None:
        M, in_len = sum(s[1] for s in segs), sum(s[3] for s in segs)
        assert all(o >= 0 and o + n <= M and i >= 0 and i + L <= in_len for o, n, i, L in segs)
    in_len = M if in_len is None else in_len
    lda, ldc = lda or Cin, ldc or nout
    ldr, ldr2, ldc2 = ldr or nout, ldr2 or nout, ldc2 or nout
    assert lda >= Cin and min(ldc, ldr, ldr2, ldc2) >= nout
    x = rnd(max(in_len, 1), Cin, seed=seed + 1)[:in_len] + mean
    w = rnd(N, taps * Cin, seed=seed + 2, scale=(taps * Cin) ** -0.5) if W is None else W
    bv = (rnd(N, seed=seed + 3, scale=0.1) if b is None else b) if bias else None
    r1 = rnd(M, nout, seed=seed + 4) if (R or inplace) else None
    r2 = rnd(M, nout, seed=seed + 5) if R2 else None
    g, bt = (1.0 + rnd(Cin, seed=seed + 6, scale=0.1), rnd(Cin, seed=seed + 7, scale=0.1)) if ln else (None, None)
    dx, px = dev_in(x, lda)
    dw, db = w.to(DEV), None if bv is None else bv.to(DEV)
    dg, dbt = (g.to(DEV), bt.to(DEV)) if ln else (None, None)
    out, out2 = out_buf(M, GUARD, ldc), out_buf(M, GUARD, ldc2)
    lno = out_buf(M, GUARD, Cin)
    written = torch.zeros(M + GUARD, ldc, dtype=torch.bool)
    for o, n in ([(0, M)] if segs is None else [(s[0], s[1]) for s in segs]):
        written[o:o + n, :nout] = True
    written2 = torch.zeros(M + GUARD, ldc2, dtype=torch.bool)
    written2[:, :nout] = written[:, :nout]
    if inplace:                                           # C == R: the residual sits where the result goes
        assert ldr == ldc and segs is None
        out[:M, :nout] = r1.to(DEV)
        pr, keep_r = P(out), None
    elif R:
        keep_r, pr = dev_in(r1, ldr)
    else:
        keep_r, pr = None, None
    keep_r2, pr2 = dev_in(r2, ldr2) if R2 else (None, None)
    dsegs = None if segs is None else torch.tensor(segs, dtype=torch.int32, device=DEV)
    start = out.clone() if expect_rc else None
    before = census(lib)
    if entry == "lin":
        assert taps == 1 and stride == 1 and pad == 0 and segs is None and not R2 and not C2 and in_len == M
        rc = lib.ss_op_ln_linear_ex(S(), px, lda, P(dg), P(dbt), P(lno) if ln_out else None, P(dw), P(db), pr, ldr, P(out), ldc, M, N, Cin,
                                    act, alpha, glu, canon)
    else:
        assert not ln and not ln_out
        a = SSOpConvArgs()
        a.A, a.W, a.bias, a.R, a.R2, a.C, a.C2 = px, P(dw), P(db), pr, pr2, P(out), P(out2) if C2 else None
        a.lda, a.ldc, a.ldr, a.ldr2, a.ldc2 = lda, ldc, ldr, ldr2, ldc2
        a.M, a.N, a.Cin, a.taps, a.dil, a.stride, a.pad, a.in_len, a.chunk = M, N, Cin, taps, dil, stride, pad, in_len, chunk
        a.in_act, a.in_slope, a.act, a.act_slope, a.alpha, a.div, a.c2_slope, a.glu = in_act, 0.1, act, act_slope, alpha, div, c2_slope, glu
        if segs is not None:
            a.segs, a.nseg, a.max_seg_out = P(dsegs), len(segs), max(s[1] for s in segs)
        a.same_rows = 0
        rc = lib.ss_op_conv_gemm_ex(S(), C.byref(a)) if canon == 0 else lib.ss_op_conv_gemm_rows(S(), C.byref(a), 0, None, None, canon)
    torch.cuda.synchronize()
    took = took_since(lib, before)
    del keep_r, keep_r2, dx
    if expect_rc:
        assert rc == expect_rc, f"{what}: rc {rc}"
        assert took == {}, f"{what}: a refused call was booked as a launch: {took}"
        assert torch.equal(bits(out), bits(start)) and untouched(out2.cpu()) and untouched(lno.cpu()), f"{what}: a refused call wrote"
        return None
    assert rc == 0, f"{what}: rc {rc}"
    assert took == {cls: 1}, f"{what}: launches by class {took}, expected one of {cls}"
    out, out2, lno = out.cpu(), out2.cpu(), lno.cpu()
    kw = dict(taps=taps, dil=dil, stride=stride, pad=pad, chunk=chunk, in_slope=0.1 if in_act == LRELU else None, act=act,
              act_slope=act_slope, alpha=alpha, div=div, glu=bool(glu), c2_slope=c2_slope)

    if rows is not None:
        assert taps == 1 and stride == 1 and pad == 0 and chunk == 0 and segs is None and in_len == M and not C2 and not ln_out
        assert rows.dtype == torch.long and rows.numel() > 0 and int(rows.min()) >= 0 and int(rows.max()) < M

    def reference(dt):
        f = lambda t: None if t is None else t.to(dt)
        if rows is not None:
            pick = lambda t: None if t is None else f(t[rows])
            return G.gemm(pick(x), f(w), ln=(f(g), f(bt)) if ln else None, bias=f(bv), R=pick(r1), R2=pick(r2), **kw)
        return G.gemm(f(x), f(w), M=None if segs is not None else M, in_len=None if segs is not None else in_len,
                      ln=(f(g), f(bt)) if ln else None, bias=f(bv), R=f(r1), R2=f(r2), segs=segs, out_rows=M, **kw)
    if refs is not None and "ref" in refs:
        ref, ref2 = refs["ref"]
    else:
        ref, ref2 = reference(torch.float64)
        if refs is not None:
            refs.update(ref=(ref, ref2), x=x, w=w)
    assert torch.isfinite(out[written]).all(), f"{what}: not finite where the op writes"
    if rows is not None:
        err = (out[rows][:, :nout].double() - ref).abs().max().item()
    else:
        err = (out[:M, :nout].double() - ref)[written[:M, :nout]].abs().max().item() if written.any() else 0.0
    line = f"{worst.route} | {what}: max abs err {err:.3e}"
    if tol == "f32 chain":      # a measured bound: 4 x the error of the plain float32 chain (two-pass LayerNorm + matmul on the host)
        chain = (reference(torch.float32)[0].double() - ref).abs().max().item()
        tol = 4.0 * chain
        line += f" (float32 chain on the host {chain:.3e}, bound {tol:.3e})"
    print(line)
    assert err < tol, f"{what}: max abs err {err} (bound {tol})"
    assert untouched(out, written), f"{what}: C was written outside the op's elements (rows >= M, gap columns, rows of no utterance)"
    if C2:
        assert torch.equal(out2[written2], torch.where(out[written] > 0, out[written], out[written] * c2_slope)), \
            f"{what}: C2 != leaky_relu(C, c2_slope)"
        assert (out2[:M, :nout].double() - ref2)[written[:M, :nout]].abs().max().item() < tol, f"{what}: C2"
        assert untouched(out2, written2), f"{what}: C2 was written outside the op's elements"
    else:
        assert untouched(out2), f"{what}: an unbound C2 was written"
    if ln_out:
        e = (lno[:M].double() - G.layernorm(x.double(), g.double(), bt.double())).abs().max().item()
        print(f"{worst.route} | {what}: ln_out max abs err {e:.3e}")
        assert e < LN_TOL, f"{what}: ln_out max abs err {e}"
        assert untouched(lno[M:]), f"{what}: ln_out rows >= M were written"
    else:
        assert untouched(lno), f"{what}: an unbound ln_out was written"
    worst.add(err)
    return out, out2, lno, err


# =====================================================================================================
# gemv_kernel: M <= 4, K % 256 == 0, K <= 2048 (gemv_eligible); booked as smallm_gemm<4,1>, the class it shares with the small-M kernel
# =====================================================================================================
def gemv_eligible(M, K, glu=0):
    return M <= 4 and K % 256 == 0 and K <= 2048 and K % 64 == 0 and not glu        # on a plain linear of M <= 192 rows (smallm_eligible)


def gemv_ks(N, K):
    """launch_gemv: one wave per column, KS waves per column while N alone gives too few; KS divides K / 256."""
    kq = K // 256
    return 1 if (N >= 2048 or kq % 2) else 2 if (N * 2 >= 2048 or kq % 4) else 4


EPILOGUES = {"plain": dict(bias=False), "silu": dict(act=SILU, alpha=0.5, R=True), "relu": dict(act=RELU, alpha=0.5, R=True)}
PADDED = lambda N, K: dict(lda=K + 4, ldc=N + 3, ldr=N + 5)        # lda must stay a multiple of 4 (launch_conv_gemm)
GEMV = [(4, 1005, 768, 1), (1, 2048, 2048, 1), (3, 1005, 512, 2), (2, 5, 1024, 4), (4, 517, 2048, 4)]


@pytest.mark.parametrize("M,N,K,ks", GEMV, ids=[f"{m}x{n}x{k}-KS{s}" for m, n, k, s in GEMV])
def test_gemv(lib, M, N, K, ks):
    assert gemv_eligible(M, K) and gemv_ks(N, K) == ks
    if (M, N, K) == (4, 1005, 768):
        assert (K // 256) % 2 == 1 and N % 4 == 1                   # kq odd -> KS = 1 whatever N is; a scalar-only column count
    if (M, N, K) == (1, 2048, 2048):
        assert N >= 2048 and K // 256 == 8                          # N alone fills the chip; 8 float4 steps per lane
    if (M, N, K) == (3, 1005, 512):
        assert N * 2 < 2048 and (K // 256) % 4 != 0 and N % 2 == 1  # KS = 2: two columns per block, the last block has one live column
    if ks == 4:
        assert N * 2 < 2048 and (K // 256) % 4 == 0                 # one column per block
    w = Worst(f"gemv KS={ks}")
    for ln, ln_out in [(False, False), (True, False), (True, True)]:
        for name, epi in EPILOGUES.items():
            pads = PADDED(N, K) if name != "plain" else {}
            launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) ln={ln} ln_out={ln_out} {name}{' padded ld' if pads else ''}", w, M=M, N=N, Cin=K,
                   ln=ln, ln_out=ln_out, entry="lin", seed=10, **epi, **pads)
    w.done()


@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_gemv_row_counts(lib, M):
    N, K = 1005, 512
    assert gemv_eligible(M, K) and gemv_ks(N, K) == 2
    w = Worst("gemv KS=2 M=1..4")
    launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) ln_out silu padded ld", w, M=M, N=N, Cin=K, ln=True, ln_out=True, entry="lin", seed=20,
           **EPILOGUES["silu"], **PADDED(N, K))
    w.done()


def test_gemv_in_place(lib):
    """C == R, as the decoder's residual adds are launched."""
    M, N, K = 3, 517, 1024
    assert gemv_eligible(M, K) and gemv_ks(N, K) == 4
    w = Worst("gemv in place")
    launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) C == R ln", w, M=M, N=N, Cin=K, ln=True, entry="lin", inplace=True, alpha=0.5, ldc=N + 3,
           ldr=N + 3, seed=30)
    w.done()


@pytest.mark.parametrize("M,N,K,ln", [(3, 1005, 512, True), (4, 1005, 768, False)])
def test_gemv_and_small_m_kernel_on_the_same_data(lib, M, N, K, ln):
    """ss_debug_force_tile(1, 0, 0) keeps an M <= 4 launch off the GEMV (gemm.hip: `(!force_bm || ln_out) && gemv_eligible`): the same
    data then runs on smallm_gemm_kernel<4,1> (force_bm = 1 is not > 1, so smallm_eligible still holds; cdiv(M, 16) cdiv(N, 16) = 63
    workgroups <= 1024).  Same class in the census; both within the bound."""
    assert gemv_eligible(M, K) and cdiv(M, 16) * cdiv(N, 16) <= 1024 and (not ln or K <= 512)
    w = Worst("gemv vs small-M <4,1>")
    kw = dict(M=M, N=N, Cin=K, ln=ln, entry="lin", seed=40, **EPILOGUES["silu"], **PADDED(N, K))
    a = launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) ln={ln} gemv", w, **kw)
    try:
        assert lib.ss_debug_force_tile(1, 0, 0) == 0
        b = launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) ln={ln} smallm under force_tile(1, 0, 0)", w, **kw)
    finally:
        restore(lib)
    assert (a[0][:M, :N] - b[0][:M, :N]).abs().max().item() < 2 * TOL
    w.done()


def test_ln_out_is_refused_off_the_gemv(lib):
    """Only the GEMV publishes the normalised rows: any other shape with ln_out set is SS_ERR_ARG, books nothing, writes nothing."""
    w = Worst("refusals")
    for M, N, K, canon in [(5, 48, 512, 0), (3, 48, 320, 0), (3, 48, 512, 1), (3, 48, 512, 2)]:
        assert not gemv_eligible(M, K) or canon != 0
        launch(lib, None, f"ln_out at ({M}, {N}, {K}) canon={canon}", w, M=M, N=N, Cin=K, ln=True, ln_out=True, entry="lin", canon=canon,
               expect_rc=SS_ERR_ARG)


# =====================================================================================================
# smallm_gemm_kernel: plain linears of M <= 192 rows, K % 64 == 0 (smallm_eligible), and CANON_SMALLM up to 1024 rows
# =====================================================================================================
def smallm_form(M, N, K):
    """launch_conv_gemm: 4 waves on one 16-column tile's k-quarters while the 16 x 16 tiles are few, 2 x 2 and 1 x 4 as they grow."""
    wgs16 = cdiv(M, 16) * cdiv(N, 16)
    return (4, 1) if (K >= 1024 or wgs16 <= 1024) else (2, 2) if wgs16 <= 4096 else (1, 4)


def smallm_eligible(M, K):
    return 0 < M <= 192 and K % 64 == 0


SMALL = [(5, 48, 64), (17, 1005, 320), (16, 64, 576), (15, 32, 2048), (33, 5500, 64), (192, 5472, 64)]


@pytest.mark.parametrize("M,N,K", SMALL, ids=["x".join(map(str, s)) for s in SMALL])
def test_small_m(lib, M, N, K):
    assert smallm_eligible(M, K) and not gemv_eligible(M, K)
    form = smallm_form(M, N, K)
    kc = K // 16                                                # 16-wide chunks, split over the SK waves of a column tile
    if (M, N, K) == (5, 48, 64):
        assert form == (4, 1) and kc // 4 == 1                  # one chunk per wave: no group of four, the tail loop only
    if (M, N, K) == (17, 1005, 320):
        assert form == (4, 1) and kc // 4 == 5                  # one group of four plus a tail of one
    if (M, N, K) == (16, 64, 576):
        assert form == (4, 1) and kc // 4 == 9 and (kc * 1) // 4 == 9 and 9 % 4 != 0      # > 8 chunks: the blocked flush, c_begin = 9 off a 64-k block
    if (M, N, K) == (15, 32, 2048):
        assert form == (4, 1) and K >= 1024 and M > 4           # K >= 1024 keeps the k-quarters whatever the tile count
    if (M, N, K) == (33, 5500, 64):
        assert form == (2, 2) and cdiv(M, 16) * cdiv(N, 16) == 3 * 344 == 1032
    if (M, N, K) == (192, 5472, 64):
        assert form == (1, 4) and cdiv(M, 16) * cdiv(N, 16) == 12 * 342 == 4104
    w = Worst("small-M <%d,%d>" % form)
    for name, epi in EPILOGUES.items():
        pads = PADDED(N, K) if name != "plain" else {}
        launch(lib, SMALLM[form], f"({M}, {N}, {K}) {name}{' padded ld' if pads else ''}", w, M=M, N=N, Cin=K, entry="lin", seed=50, **epi,
               **pads)
    w.done()


@pytest.mark.parametrize("M", [15, 16, 17])
def test_small_m_rows_around_a_tile(lib, M):
    N, K = 1005, 320
    assert smallm_eligible(M, K) and smallm_form(M, N, K) == (4, 1)
    w = Worst("small-M <4,1> M=15/16/17")
    for name, epi in EPILOGUES.items():
        launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) ln {name} padded ld", w, M=M, N=N, Cin=K, ln=True, entry="lin", seed=60, **epi,
               **PADDED(N, K))
    launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) C == R", w, M=M, N=N, Cin=K, entry="lin", inplace=True, alpha=0.5, ldc=N + 3, ldr=N + 3,
           seed=61)
    w.done()


LN_SMALL = [(17, 48, 64, 0), (17, 1005, 320, 0), (20, 517, 512, 0), (33, 5500, 64, 0), (40, 96, 64, 1)]


@pytest.mark.parametrize("M,N,K,glu", LN_SMALL, ids=["x".join(map(str, s)) for s in LN_SMALL])
def test_small_m_layernorm(lib, M, N, K, glu):
    """The fused LayerNorm prologue (LNORM = true: the row in registers, K <= 512) on the three forms that have it."""
    assert smallm_eligible(M, K) and K <= 512
    form = (2, 2) if glu else smallm_form(M, N, K)
    assert form == ((2, 2) if (glu or N == 5500) else (4, 1))
    w = Worst("small-M <%d,%d> LayerNorm%s" % (form + (" GLU" if glu else "",)))
    if glu:
        assert N % 32 == 0
        for bias in (True, False):
            launch(lib, SMALLM[form], f"({M}, {N}, {K}) ln glu bias={bias}", w, M=M, N=N, Cin=K, ln=True, glu=1, bias=bias, entry="lin",
                   ldc=N // 2 + 3, lda=K + 4, seed=70)
    else:
        for name, epi in EPILOGUES.items():
            pads = PADDED(N, K) if name != "plain" else {}
            launch(lib, SMALLM[form], f"({M}, {N}, {K}) ln {name}{' padded ld' if pads else ''}", w, M=M, N=N, Cin=K, ln=True, entry="lin",
                   seed=70, **epi, **pads)
    w.done()


@pytest.mark.parametrize("bias", [True, False])
def test_small_m_glu(lib, bias):
    M, N, K = 40, 96, 128
    assert smallm_eligible(M, K) and N % 32 == 0                # GLU: always the 2 x 2 form (value and gate tiles side by side)
    w = Worst("small-M <2,2> GLU")
    launch(lib, SMALLM[2, 2], f"({M}, {N}, {K}) glu bias={bias}", w, M=M, N=N, Cin=K, glu=1, bias=bias, entry="lin", seed=80)
    launch(lib, SMALLM[2, 2], f"({M}, {N}, {K}) glu bias={bias} padded ld", w, M=M, N=N, Cin=K, glu=1, bias=bias, entry="lin", seed=81,
           lda=K + 4, ldc=N // 2 + 5)
    w.done()


def test_small_m_layernorm_of_rows_with_a_large_mean(lib):
    """Rows of mean 100 and spread 1.  The bound here is MEASURED, not fixed: 4 x the max abs error, against float64, of a float32
    two-pass LayerNorm + float32 matmul of the same data on the host.  That is the plain float32 chain, which the kernel's two-pass
    statistics should not be far from (a one-pass E[x^2] - mean^2 would lose four digits here); the factor 4 covers summation order."""
    M, N, K = 20, 517, 512
    assert smallm_eligible(M, K) and smallm_form(M, N, K) == (4, 1)
    w = Worst("small-M <4,1> LayerNorm, row mean 100")
    launch(lib, SMALLM[4, 1], f"({M}, {N}, {K}) ln mean 100", w, M=M, N=N, Cin=K, ln=True, entry="lin", seed=90, mean=100.0, tol="f32 chain")
    w.done()


def test_canon_small_m(lib):
    """CANON_SMALLM (canon = 2): the split-K form is a function of (N, K) alone -- 4 x 1 when K >= 1024 or N <= 4096, else 2 x 2 -- and
    the row cap is 1024 (smallm_shape_ok)."""
    w = Worst("small-M CANON_SMALLM")
    for M, N, K, form in [(40, 4112, 512, (2, 2)), (40, 4096, 512, (4, 1)), (1024, 32, 64, (4, 1))]:
        assert ((4, 1) if (K >= 1024 or N <= 4096) else (2, 2)) == form and M <= 1024
        launch(lib, SMALLM[form], f"({M}, {N}, {K}) canon=2 relu", w, M=M, N=N, Cin=K, entry="lin", canon=2, seed=100, **EPILOGUES["relu"],
               ldc=N + 4)
    launch(lib, SMALLM[4, 1], "(40, 4096, 512) canon=2 ln", w, M=40, N=4096, Cin=512, ln=True, entry="lin", canon=2, seed=101)
    w.done()
    launch(lib, None, "1025 rows under canon=2", w, M=1025, N=32, Cin=64, entry="lin", canon=2, expect_rc=SS_ERR_ARG)
    launch(lib, None, "ln_g at K = 1024 under canon=2", w, M=40, N=64, Cin=1024, ln=True, entry="lin", canon=2, expect_rc=SS_ERR_ARG)


def test_layernorm_linears_no_kernel_takes_are_refused(lib):
    """K > 512 on the small-M kernel (refused before the census is touched) and CANON_SEQ at K != 256 (the row-tile kernel only)."""
    w = Worst("refusals")
    for M, N, K in [(16, 512, 1024), (3, 512, 4096), (192, 512, 768)]:
        assert smallm_eligible(M, K) and not gemv_eligible(M, K) and K > 512
        launch(lib, None, f"ln_g at ({M}, {N}, {K})", w, M=M, N=N, Cin=K, ln=True, entry="lin", expect_rc=SS_ERR_ARG)
    launch(lib, None, "canon=1 with ln_g at K = 320", w, M=50, N=64, Cin=320, ln=True, entry="lin", canon=1, expect_rc=SS_ERR_ARG)


# =====================================================================================================
# conv_gemm_kernel, default arithmetic
# =====================================================================================================
def ks_ladder(tiles, nk, maxks):
    """launch_cfg_ks: double the k-split while tiles * 4 * KS waves do not cover 1024 SIMDs and every group keeps >= 2 k-steps."""
    ks = 1
    while ks < maxks and tiles * 4 * ks < 1024 and nk // (ks * 2) >= 2:
        ks *= 2
    return ks


def k_groups(nk, ks):
    """k-steps of each group of the kernel: [g * kper, min(nk, (g + 1) * kper)) with kper = ceil(nk / KS)."""
    kper = cdiv(nk, ks)
    return [max(0, min(nk, (g + 1) * kper) - g * kper) for g in range(ks)]


def default_tile(M, N, Cin, taps=1, glu=0, nseg=0, **_):
    """(class, KS) of the tail of launch_conv_gemm for a launch no other kernel takes; M: the longest utterance of a pack."""
    ns, k32 = max(nseg, 1), Cin % 32 == 0
    bk = 32 if k32 else 16
    if N <= 16:
        return "conv_gemm<128,16,16,4,1>", ks_ladder(cdiv(M, 128) * ns, taps * (Cin // 16), 2)
    if N <= 32 and not glu:
        return f"conv_gemm<128,32,{bk},4,1>", ks_ladder(cdiv(M, 128) * ns, taps * (Cin // bk), 2)
    if M <= 16:
        return f"conv_gemm<16,128,{bk},1,4>", 1
    t3264, t3232 = cdiv(M, 32) * cdiv(N, 64) * ns, cdiv(M, 32) * cdiv(N, 32) * ns
    if k32 and t3264 >= 768:
        return "conv_gemm<32,64,32,2,2>", 1
    if not k32 or glu:
        return f"conv_gemm<32,64,{bk},2,2>", ks_ladder(t3264, taps * (Cin // bk), 4)
    nk = taps * (Cin // 32)
    return "conv_gemm<32,32,32,2,2>", 1 if (t3232 >= 700 or nk < 4) else 2 if (t3232 >= 300 or nk < 8) else 4


def not_a_small_linear(M, Cin, taps=1, stride=1, pad=0, chunk=0, in_act=NONE, R2=False, C2=False, div=0.0, act=NONE, segs=None, **_):
    """smallm_eligible is false: more than 192 rows, or not a plain linear."""
    return M > 192 or Cin % 64 != 0 or taps != 1 or stride != 1 or pad != 0 or chunk != 0 or in_act != NONE or R2 or C2 or div != 0.0 or \
        act in (TANH, LRELU) or segs is not None


FULL = dict(act=TANH, alpha=0.5, R=True, R2=True, div=3.0, C2=True)         # bias + tanh + alpha + R + R2 + / 3 + the twin
# id -> (kwargs, class, KS, k-steps per group)
TILES = {
    # 128x16x16: 7 k-steps on two groups of 4 and 3
    "128x16x16-KS2-4+3": (dict(M=300, N=16, Cin=16, taps=7, dil=3, pad=9, **FULL), "conv_gemm<128,16,16,4,1>", 2, [4, 3]),
    # ... one output column; the tanh keeps this 129-row linear off the small-M kernel (smallm_eligible takes none / SiLU / ReLU only)
    "128x16x16-N1": (dict(M=129, N=1, Cin=128, act=TANH), "conv_gemm<128,16,16,4,1>", 2, [4, 4]),
    "128x16x16-KS1": (dict(M=200, N=16, Cin=16, taps=3, pad=1, in_act=LRELU), "conv_gemm<128,16,16,4,1>", 1, [3]),
    "128x32x32-KS1": (dict(M=150, N=32, Cin=32, taps=3, pad=1, R=True), "conv_gemm<128,32,32,4,1>", 1, [3]),
    "128x32x32-KS2-3+2": (dict(M=150, N=32, Cin=32, taps=5, pad=2, **FULL), "conv_gemm<128,32,32,4,1>", 2, [3, 2]),
    "128x32x16-N20": (dict(M=131, N=20, Cin=48, taps=3, pad=1, act=LRELU, act_slope=0.3), "conv_gemm<128,32,16,4,1>", 2, [5, 4]),
    "16x128x32": (dict(M=16, N=200, Cin=32, taps=2, pad=0, in_len=17, R=True), "conv_gemm<16,128,32,1,4>", 1, [2]),
    "16x128x16": (dict(M=7, N=1005, Cin=48, taps=3, pad=1, **FULL), "conv_gemm<16,128,16,1,4>", 1, [9]),
    # 768 tiles of 32 x 64: the batched form, no split; 32 m-tiles is already a multiple of 8
    "32x64x32-big": (dict(M=1024, N=1536, Cin=32, R=True, act=SILU), "conv_gemm<32,64,32,2,2>", 1, [1]),
    # the subsampler's first conv as the model launches it: 25 k-steps of 16 on four groups of 7 / 7 / 7 / 4, which begin at
    # (channel block, tap) = (0, 0), (1, 2), (2, 4), (4, 1) -- in the middle of a channel block's taps
    "32x64x16-sub1": (dict(M=42, N=1024, Cin=80, taps=5, stride=2, pad=2, in_len=83, glu=1), "conv_gemm<32,64,16,2,2>", 4, [7, 7, 7, 4]),
    "32x64x16-sub1-chunk8": (dict(M=42, N=1024, Cin=80, taps=5, stride=2, pad=2, in_len=83, glu=1, chunk=8), "conv_gemm<32,64,16,2,2>",
                             4, [7, 7, 7, 4]),
    # its second conv (512 -> 512 GLU) on those 42 rows: 80 k-steps of 32 on four groups of 20
    "32x64x32-sub2": (dict(M=21, N=512, Cin=512, taps=5, stride=2, pad=2, in_len=42, glu=1, chunk=8), "conv_gemm<32,64,32,2,2>", 4,
                      [20, 20, 20, 20]),
    # ... and at T = 11: 6 output rows, which the M <= 16 rung of the ladder takes before the 32 x 64 GLU rung is reached
    "16x128x32-sub2-T11": (dict(M=6, N=512, Cin=512, taps=5, stride=2, pad=2, in_len=11, glu=1), "conv_gemm<16,128,32,1,4>", 1, [80]),
    "32x32x32-KS1": (dict(M=100, N=96, Cin=32, taps=3, pad=1, R=True), "conv_gemm<32,32,32,2,2>", 1, [3]),
    "32x32x32-KS2": (dict(M=100, N=96, Cin=64, taps=3, pad=1, **FULL), "conv_gemm<32,32,32,2,2>", 2, [3, 3]),
    "32x32x32-KS4-4+4+4+2": (dict(M=100, N=96, Cin=64, taps=7, pad=3, **FULL), "conv_gemm<32,32,32,2,2>", 4, [4, 4, 4, 2]),
    # nine k-steps on four groups of three: the last group is empty (kb0 = 9 >= nk) and only adds zeros
    "32x32x32-KS4-empty-group": (dict(M=100, N=96, Cin=96, taps=3, pad=1, R=True), "conv_gemm<32,32,32,2,2>", 4, [3, 3, 3, 0]),
    # M != in_len: 70 output rows over an input of 50 -- rows past in_len read as zero, the guard rows behind it hold 1e4
    "rows-past-in_len": (dict(M=70, N=96, Cin=32, taps=3, pad=1, in_len=50), "conv_gemm<32,32,32,2,2>", 1, [3]),
    # the scalar epilogue (vec == false): N % 4 != 0 ...
    "scalar-N37": (dict(M=40, N=37, Cin=32, taps=3, pad=1, **FULL), "conv_gemm<32,32,32,2,2>", 1, [3]),
    "scalar-N1005": (dict(M=40, N=1005, Cin=32, taps=2, pad=0, in_len=41, **FULL), "conv_gemm<32,32,32,2,2>", 1, [2]),
    # ... and N % 4 == 0 with one leading dimension that is not
    "scalar-ldc67": (dict(M=40, N=64, Cin=32, taps=3, pad=1, ldc=67, **FULL), "conv_gemm<32,32,32,2,2>", 1, [3]),
    "scalar-ldr2-65": (dict(M=40, N=64, Cin=32, taps=3, pad=1, ldr2=65, **FULL), "conv_gemm<32,32,32,2,2>", 1, [3]),
    "scalar-ldr-66-ldc2-70": (dict(M=40, N=64, Cin=32, taps=3, pad=1, ldr=66, ldc2=70, **FULL), "conv_gemm<32,32,32,2,2>", 1, [3]),
    "scalar-lrelu": (dict(M=40, N=37, Cin=64, taps=3, pad=1, act=LRELU, act_slope=0.3, alpha=0.5, R=True, R2=True, div=3.0, C2=True,
                          c2_slope=0.2), "conv_gemm<32,32,32,2,2>", 2, [3, 3]),
    # the vector epilogue with every operand and padded leading dimensions that stay multiples of 4
    "vector-full-padded": (dict(M=40, N=64, Cin=32, taps=3, pad=1, lda=36, ldc=68, ldr=72, ldr2=76, ldc2=80, act=LRELU, act_slope=0.3,
                                alpha=0.5, R=True, R2=True, div=3.0, C2=True, c2_slope=0.2), "conv_gemm<32,32,32,2,2>", 1, [3]),
}


def check_tile_route(kw, cls, ks, groups):
    """The stated (class, KS, groups) are what the dispatcher's arithmetic gives for these arguments."""
    segs = kw.get("segs")
    M = max(s[1] for s in segs) if segs else kw["M"]
    rows = sum(s[1] for s in segs) if segs else kw["M"]
    assert not_a_small_linear(**{**kw, "M": M}), "a plain linear of <= 192 rows: the small-M kernel's"
    assert rows < 2048                                          # (and same_rows = 0: no slab, Winograd or stream-K kernel is eligible)
    assert not (kw.get("taps", 1) == 1 and kw["Cin"] == 256)    # K = 256 linears are rt_linear's
    assert default_tile(M, kw["N"], kw["Cin"], kw.get("taps", 1), kw.get("glu", 0), len(segs) if segs else 0) == (cls, ks)
    bk = int(cls.split(",")[2])
    nk = kw.get("taps", 1) * (kw["Cin"] // bk)
    assert k_groups(nk, ks) == groups, f"nk = {nk}, KS = {ks}: groups {k_groups(nk, ks)}"


@pytest.mark.parametrize("case", list(TILES))
def test_tile(lib, case):
    kw, cls, ks, groups = TILES[case]
    check_tile_route(kw, cls, ks, groups)
    w = Worst(f"{cls} KS={ks}")
    launch(lib, cls, case, w, seed=200, **kw)
    w.done()


def test_tile_polyphase_upsampler(lib):
    """The vocoder's upsampler as it is launched: leaky-ReLU(0.1) on the input, the ConvTranspose1d (64 -> 32 channels, k = 8, stride 4)
    as a 3-tap conv with pad 1 and N = stride * Cout, bias -- against the reference and against torch's own conv_transpose1d."""
    from streamspeech_amd.weights import convT_polyphase
    cin, cout, k, stride, M = 64, 32, 8, 4, 100
    wt, b = rnd(cin, cout, k, seed=311, scale=(cin * k / stride) ** -0.5), rnd(cout, seed=312, scale=0.1)
    wp, bp = convT_polyphase(wt, b, stride)
    kw = dict(M=M, N=stride * cout, Cin=cin, taps=3, pad=1, in_act=LRELU)
    cls, ks = "conv_gemm<32,32,32,2,2>", 2                      # 4 x 4 tiles < 300 and 6 k-steps < 8
    check_tile_route(kw, cls, ks, [3, 3])
    w = Worst(f"{cls} KS={ks}")
    out, _, _, _ = launch(lib, cls, "polyphase upsampler 64->32 k=8 s=4", w, seed=300, W=wp, b=bp, **kw)
    x = rnd(M, cin, seed=301)                                  # launch()'s input: seed + 1
    ref = slab_ref.upsample(x.double(), wt.double(), b.double(), [(0, M)], stride, in_slope=0.1)
    assert (out[:M].reshape(M * stride, cout).double() - ref).abs().max().item() < TOL
    w.done()


def strided_pack(lens, taps, stride, pad):
    """Segment table of a strided conv over a pack: out_len = (in_len + 2 pad - taps) // stride + 1 floored at 0, out_start != in_start."""
    segs, o, i = [], 0, 0
    for L in lens:
        n = max(0, (L + 2 * pad - taps) // stride + 1)
        assert n == G.out_len_of(L, taps, stride, pad)
        segs.append((o, n, i, L))
        o, i = o + n, i + L
    return segs


@pytest.mark.parametrize("chunk", [0, 8])
@pytest.mark.parametrize("form", ["32x32x32", "32x64x16-glu"])
def test_tile_ragged_strided_pack(lib, form, chunk):
    """A stride-2 conv over a ragged pack (one grid plane per utterance), every utterance convolved alone in the reference: in_len 1, 2
    and 5 (shorter than the five taps), 64, 65, 131, and one of no rows, whose plane leaves at once (m0 >= out_len)."""
    segs = strided_pack([1, 2, 5, 64, 0, 65, 131], 5, 2, 2)
    assert [s[1] for s in segs] == [1, 1, 3, 32, 0, 33, 66] and any(s[0] != s[2] for s in segs)
    if form == "32x32x32":          # 3 x 3 x 7 = 63 tiles, 10 k-steps on four groups of 3 / 3 / 3 / 1
        kw, cls, ks, groups = dict(N=96, Cin=64, R=True, act=RELU), "conv_gemm<32,32,32,2,2>", 4, [3, 3, 3, 1]
    else:                           # the subsampler's first conv over a pack: BK = 16, 25 k-steps, 3 x 2 x 7 = 42 tiles
        kw, cls, ks, groups = dict(N=128, Cin=80, glu=1), "conv_gemm<32,64,16,2,2>", 4, [7, 7, 7, 4]
    kw.update(taps=5, stride=2, pad=2, chunk=chunk, segs=segs)
    check_tile_route(kw, cls, ks, groups)
    w = Worst(f"{cls} KS={ks} ragged stride 2")
    launch(lib, cls, f"{form} chunk={chunk} ragged stride-2 pack", w, seed=400, **kw)
    w.done()


def test_tile_grid_padding(lib):
    """launch_cfg rounds grid.x up to a multiple of 8 from 32 m-tiles on (XCD affinity): an utterance of 1025 rows gives 33 -> 40
    m-tiles per plane, and the seven padding blocks must write nothing (the NaN rows behind each utterance and behind the pack).
    At N = 128 the pack has 33 x 2 x 2 = 132 tiles of 32 x 64 < 768, so it takes the 32 x 32 tile (one k-step: no split); N = 768
    gives 33 x 12 x 2 = 792 >= 768 -- the batched 32 x 64 form."""
    segs = [(0, 1025, 0, 1025), (1025, 40, 1025, 40)]
    for N, cls in [(128, "conv_gemm<32,32,32,2,2>"), (768, "conv_gemm<32,64,32,2,2>")]:
        kw = dict(N=N, Cin=32, R=True, segs=segs)
        check_tile_route(kw, cls, 1, [1])
        assert cdiv(1025, 32) == 33 and (33 + 7) & ~7 == 40 and cdiv(N, int(cls.split(",")[1])) * len(segs) > 1
        w = Worst(f"{cls} KS=1 grid padding")
        launch(lib, cls, f"(1025 + 40, {N}, 32) two utterances, 33 -> 40 m-tiles", w, seed=500, **kw)
        w.done()


# =====================================================================================================
# conv_gemm_kernel<.., BLK = true>: CANON_SEQ (canon = 1), one case per form of launch_canon, dense and as a ragged pack
# =====================================================================================================
def canon_tile(M, N, Cin, glu=0, nseg=0):
    """The tile of launch_canon (no split-K there) for a launch neither rt_linear nor rt_linear_kb takes."""
    ns, k32 = max(nseg, 1), Cin % 32 == 0
    bk = 32 if k32 else 16
    if N <= 16:
        return "conv_gemm<128,16,16,4,1>"
    if N <= 32 and not glu:
        return f"conv_gemm<128,32,{bk},4,1>"
    if M <= 16:
        return f"conv_gemm<16,128,{bk},1,4>"
    if not k32:
        return "conv_gemm<32,64,16,2,2>"
    if glu or cdiv(M, 32) * cdiv(N, 64) * ns >= 768:
        return "conv_gemm<32,64,32,2,2>"
    return "conv_gemm<32,32,32,2,2>"


# id -> (kwargs of the dense launch, utterance lengths of the ragged one, class); K = taps * Cin: 64 (no flush of the 64-k block chain),
# 128 (one), 160 / 320 of 32-wide steps whose blocks cross taps, and K = 32
CANON = {
    "128x16x16-K64": (dict(M=150, N=16, Cin=16, taps=4, pad=1, **FULL), [1, 129, 20], "conv_gemm<128,16,16,4,1>"),
    "128x32x32-K160": (dict(M=150, N=32, Cin=32, taps=5, pad=2, R=True), [130, 3, 17], "conv_gemm<128,32,32,4,1>"),
    "128x32x16-K144": (dict(M=131, N=20, Cin=48, taps=3, pad=1, **FULL), [2, 128, 1], "conv_gemm<128,32,16,4,1>"),
    "16x128x32-K128": (dict(M=16, N=200, Cin=128, act=SILU, R=True), [16, 1, 7], "conv_gemm<16,128,32,1,4>"),
    "16x128x16-K320": (dict(M=7, N=1005, Cin=80, taps=4, pad=1, **FULL), [7, 2], "conv_gemm<16,128,16,1,4>"),
    "32x64x16-K144": (dict(M=50, N=100, Cin=48, taps=3, pad=1, **FULL), [33, 1, 17], "conv_gemm<32,64,16,2,2>"),
    "32x64x32-glu-K320": (dict(M=33, N=128, Cin=64, taps=5, stride=2, pad=2, in_len=65, glu=1, chunk=8), [65, 5, 0, 131],
                          "conv_gemm<32,64,32,2,2>"),
    "32x64x32-big-K32": (dict(M=1024, N=1536, Cin=32, R=True), [500, 490], "conv_gemm<32,64,32,2,2>"),
    "32x32x32-K160": (dict(M=100, N=96, Cin=32, taps=5, pad=2, **FULL), [33, 64, 1], "conv_gemm<32,32,32,2,2>"),
    "32x32x32-K128-linear": (dict(M=200, N=96, Cin=128, act=RELU, R=True), [100, 31, 65], "conv_gemm<32,32,32,2,2>"),
}


@pytest.mark.parametrize("case", list(CANON))
def test_canon_seq_tile(lib, case):
    kw, lens, cls = CANON[case]
    taps, stride, pad = kw.get("taps", 1), kw.get("stride", 1), kw.get("pad", 0)
    K = taps * kw["Cin"]
    assert not (taps == 1 and K % 256 == 0)                     # K = 256 / 512 ... linears belong to rt_linear / rt_linear_kb
    assert canon_tile(kw["M"], kw["N"], kw["Cin"], kw.get("glu", 0)) == cls
    segs = strided_pack(lens, taps, stride, pad) if stride > 1 else [(s, n, s, n) for s, n in slab_ref.seg_table(lens)]
    if stride == 1:
        assert 2 * pad == taps - 1 or taps % 2 == 0             # "same" rows: out_len == in_len
    assert canon_tile(max(s[1] for s in segs), kw["N"], kw["Cin"], kw.get("glu", 0), len(segs)) == cls
    w = Worst(f"{cls} CANON_SEQ")
    launch(lib, cls, f"{case} dense", w, seed=600, canon=1, **kw)
    ragged = {k: v for k, v in kw.items() if k not in ("M", "in_len")}
    launch(lib, cls, f"{case} ragged {lens}", w, seed=601, canon=1, segs=segs, **ragged)
    w.done()


# =====================================================================================================
# a row limit set in the environment reaches the dispatcher through the Dispatch store (dispatch.hip: env_defaults -> disp())
# =====================================================================================================
def smallm_max_rows_child():
    """What the child process of the test below runs, SS_SMALLM_MAX_ROWS=16 in its environment (launch() asserts rc, the census, the
    float64 bound and the untouched elements)."""
    from streamspeech_amd import lib as L
    lib, w = L.load(), Worst("SS_SMALLM_MAX_ROWS=16")
    launch(lib, SMALLM[4, 1], "(16, 48, 64) at the limit", w, M=16, N=48, Cin=64, entry="lin", seed=700)
    before = census(lib)
    launch(lib, "conv_gemm<32,32,32,2,2>", "(17, 48, 64) one row past it", w, M=17, N=48, Cin=64, entry="lin", seed=701)
    assert not any(c in SMALLM.values() for c in took_since(lib, before))
    print("CHILD OK")


def test_smallm_row_limit_from_the_environment():
    """SS_SMALLM_MAX_ROWS is read once, into Dispatch::smallm_max_rows, and smallm_eligible reads it from there.  In a fresh process
    with the limit at 16 (default 192), a (16, 48, 64) linear is one launch of smallm_gemm<4,1> (5 <= M: not the GEMV; 1 x 3 workgroups
    <= 1024) and a (17, 48, 64) one goes down the tile ladder: N > 32, M > 16, K % 32 == 0, 1 x 1 32x64 tiles < 768, no GLU -> the
    32x32x32 rung at KS = 1 (nk = 2 < 4); nothing under any small-M class.  Both within TOL of tests/gemm_ref.py."""
    import subprocess
    import sys
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]; import test_gemm_routes_gpu as t; t.smallm_max_rows_child()"
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], env=dict(os.environ, SS_SMALLM_MAX_ROWS="16"),
                       capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "CHILD OK" in r.stdout, f"child exit {r.returncode}"
