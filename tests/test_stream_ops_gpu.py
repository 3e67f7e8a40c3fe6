"""Op-level tests of the kernels behind the streaming encoder against tests/stream_ref.py (NumPy float64): the subsampler's conv-GEMM
started at a row (GemmArgs::m_begin) and in the session pool's ragged form (seg_mb / seg_A on the CANON_SEQ tile), dwconv_bn_silu in
its ragged and row-range forms, the pool's own kernels (pool_dwconv, both pool_gather forms, pool_stack_rows) and LayerNorm with row
strides and in place -- through ss_op_conv_gemm_rows, ss_op_dwconv_bn_silu_ex, ss_op_pool_* and ss_op_layernorm.

What every case has in common: every output and cache buffer starts as one sentinel bit pattern (a NaN), with guard rows around it and
gap columns where the op has a row stride, and everything outside the rows the op is defined to write must still be that pattern
afterwards, bit for bit.  The failures aimed at are off-by-one errors in a tile's first row: a halo row from the wrong source at the
cache boundary, a write below m_begin / t_begin / seg_mb, a chunk limit taken from a tile-relative row.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import stream_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-4                     # the per-conv bound of tests/test_ops_gpu.py (O(1)-scaled data, exact FP32 accumulation)
DW_TOL = 2e-5                  # the bound of test_ops_gpu.py::test_dwconv_bn_silu
LN_TOL = 2e-5                  # the bound of test_ops_gpu.py::test_layernorm
DEV = "cuda:0"
SENT = 0x7FC5A5A5              # what every output / cache word holds before a launch
GUARD = 80                     # guard rows in front of and behind every output
SS_ERR_ARG = 2


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """A launch that faulted leaves the process without a usable device: end the run there instead of failing every later test."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def i32(rows):
    return torch.tensor(rows, dtype=torch.int32, device=DEV)


class Out:
    """A sentinel-filled device buffer [GUARD + rows + GUARD, ld]; ptr = row GUARD.  bits(): the rows from `ptr` on as int32 on the
    host; intact(): every word not in `written` (a bool mask [rows, ld] over the rows from ptr on, None: nothing) is the sentinel."""

    def __init__(self, rows, ld, dtype=torch.float32):
        self.rows, self.ld = rows, ld
        self.raw = torch.full((rows + 2 * GUARD, ld), SENT, dtype=torch.int32, device=DEV)
        self.t = self.raw.view(dtype)
        self.ptr = C.c_void_p(self.raw.data_ptr() + GUARD * ld * 4)

    def bits(self):
        torch.cuda.synchronize()
        return self.raw.cpu().numpy()[GUARD:GUARD + self.rows]

    def f32(self):
        return self.bits().view(np.float32)

    def intact(self, written=None):
        torch.cuda.synchronize()
        allb = self.raw.cpu().numpy()
        mask = np.zeros(allb.shape, bool)
        if written is not None:
            mask[GUARD:GUARD + self.rows] = written
        return bool((allb[~mask] == SENT).all())


def row_mask(rows, ld, cols, ranges):
    m = np.zeros((rows, ld), bool)
    for a, b in ranges:
        m[a:b, :cols] = True
    return m


def maxerr(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max())


# =====================================================================================================
# subsampler conv: taps 5, stride 2, pad 2, GLU, bias
# =====================================================================================================
CONV_SHAPES = [(80, 128, 83), (64, 128, 131), (512, 64, 42)]        # (Cin, N, T): BK = 16 as the model's conv 1, BK = 32, BK = 32


@functools.lru_cache(maxsize=None)
def conv_weights(cin, n):
    from streamspeech_amd.weights import conv_tap_major, glu_interleave
    w = glu_interleave(rnd(n, cin, 5, seed=100 + cin, scale=(cin * 5) ** -0.5))
    b = glu_interleave(rnd(n, seed=101 + cin, scale=0.1))
    return w.numpy(), b.numpy(), conv_tap_major(w).to(DEV), b.to(DEV)


@functools.lru_cache(maxsize=None)
def conv_input(cin, T, seed):
    x = rnd(T, cin, seed=seed)
    return x.numpy(), x.to(DEV)


@functools.lru_cache(maxsize=None)
def conv_ref(cin, n, T, chunk, seed=5):
    """All rows of one utterance, float64: computed once per (shape, chunk) and shared."""
    w, b, _, _ = conv_weights(cin, n)
    ref = R.chunk_conv(conv_input(cin, T, seed)[0], w, b, stride=2, pad=2, chunk=chunk, glu=True)
    ref.setflags(write=False)
    return ref


def conv_args(cin, n, dA, lda, out, M, in_len, chunk, segs=None, nseg=0, max_seg_out=0):
    from streamspeech_amd import lib as L
    _, _, dW, db = conv_weights(cin, n)
    a = L.SSOpConvArgs()
    a.A = None if dA is None else dA.data_ptr()
    a.W, a.bias, a.C = dW.data_ptr(), db.data_ptr(), out.ptr.value
    a.lda, a.ldc = lda, out.ld
    a.M, a.N, a.Cin, a.taps, a.dil, a.stride, a.pad, a.in_len, a.chunk = M, n, cin, 5, 1, 2, 2, in_len, chunk
    a.in_slope = a.act_slope = a.c2_slope = 0.1
    a.alpha, a.glu = 1.0, 1
    a.segs = None if segs is None else segs.data_ptr()
    a.nseg, a.max_seg_out = nseg, max_seg_out
    a._keep = (dW, db, dA, segs)
    return a


def run_conv_rows(lib, cin, n, T, chunk, m_begin, canon=0):
    """One utterance from row m_begin; returns (rc, Out)."""
    M = (T - 1) // 2 + 1
    _, dx = conv_input(cin, T, 5)
    out = Out(M, n // 2 + 4)
    a = conv_args(cin, n, dx, cin, out, M, T, chunk)
    rc = lib.ss_op_conv_gemm_rows(S(), C.byref(a), m_begin, None, None, canon)
    return rc, out


@pytest.mark.parametrize("m_begin", [0, 1, 31, 32, 33, "last"])
@pytest.mark.parametrize("chunk", [0, 8, 16])
@pytest.mark.parametrize("cin,n,T", CONV_SHAPES)
def test_conv_m_begin(lib, cin, n, T, chunk, m_begin):
    M, oc = (T - 1) // 2 + 1, n // 2
    mb = M - 1 if m_begin == "last" else m_begin
    ref = conv_ref(cin, n, T, chunk)
    assert ref.shape == (M, oc) and M == {83: 42, 131: 66, 42: 21}[T]
    rc, out = run_conv_rows(lib, cin, n, T, chunk, mb)
    if mb >= M:                                              # (the 21-row shape) refused, nothing written
        assert rc == SS_ERR_ARG and out.intact(), f"m_begin {mb} >= M {M}"
    else:
        assert rc == 0, f"rc {rc}"
        e = maxerr(out.f32()[mb:, :oc], ref[mb:])
        print(f"conv Cin {cin} N {n} T {T} chunk {chunk} m_begin {mb}: max err {e:.3g}")
        assert e < TOL, f"max err {e}"
        assert out.intact(row_mask(M, out.ld, oc, [(mb, M)])), f"a word outside rows [{mb}, {M}) changed"
    # the pack-invariant route clears m_begin: every row is written, and rows [m_begin, M) are the bits of its m_begin = 0 launch
    try:
        assert lib.ss_debug_canon(1) == 0
        rc0, base = run_conv_rows(lib, cin, n, T, chunk, 0)
        rc1, can = run_conv_rows(lib, cin, n, T, chunk, mb)
    finally:
        lib.ss_debug_canon(0)
    assert rc0 == 0 and rc1 == 0
    for o in (base, can):
        assert o.intact(row_mask(M, o.ld, oc, [(0, M)]))
        e = maxerr(o.f32()[:, :oc], ref)
        assert e < TOL, f"canon: max err {e}"
    lo = min(mb, M)
    assert np.array_equal(can.bits()[lo:, :oc], base.bits()[lo:, :oc])


def test_conv_rows_refusals(lib):
    cin, n, T = 80, 128, 83
    M = 42
    _, dx = conv_input(cin, T, 5)
    segs = i32([[0, M, 0, T]])
    mb = i32([[3, 8]])
    pA = torch.tensor([dx.data_ptr()], dtype=torch.int64, device=DEV)

    def call(m_begin=0, seg_mb=None, seg_A=None, canon=0, nseg=0, n_=n, cin_=cin):
        out = Out(M, n_ // 2 + 4)
        x = dx if cin_ == cin else conv_input(cin_, T, 5)[1]
        a = conv_args(cin_, n_, x, cin_, out, M, T, 8, segs if nseg else None, nseg, M if nseg else 0)
        rc = lib.ss_op_conv_gemm_rows(S(), C.byref(a), m_begin, P(seg_mb), P(seg_A), canon)
        return rc, out.intact()

    assert call(m_begin=M) == (SS_ERR_ARG, True) and call(m_begin=M + 8) == (SS_ERR_ARG, True)
    assert call(m_begin=3, nseg=1) == (SS_ERR_ARG, True)                       # a row range of a ragged pack
    assert call(m_begin=3, n_=32, cin_=64) == (SS_ERR_ARG, True)               # N <= 32: not the LDS-tile kernel
    assert call(seg_mb=mb, nseg=1) == (SS_ERR_ARG, True)                       # seg_mb / seg_A without canon
    assert call(seg_A=pA, nseg=1) == (SS_ERR_ARG, True)
    assert call(seg_mb=mb, seg_A=pA, nseg=1) == (SS_ERR_ARG, True)
    assert call(seg_mb=mb, canon=1) == (SS_ERR_ARG, True)                      # seg_mb with nseg == 0
    assert call(seg_mb=mb, canon=0) == (SS_ERR_ARG, True)
    assert call(seg_mb=mb, seg_A=pA, nseg=1, canon=2) == (SS_ERR_ARG, True)    # ... and on the small-M route
    rc, untouched = call(seg_mb=mb, seg_A=pA, nseg=1, canon=1)                 # the legal form of the same call goes through
    assert rc == 0 and not untouched


# ---- the pooled form: seg_mb (+ seg_A) on the CANON_SEQ 32x64 tile -------------------------------------
# sessions (T, first row, chunk); out_len = 66 / 42 / 10 / 3 for T = 131 / 83 / 20 / 5
POOL_CONV = {
    "1a": [(131, 33, 8)], "1b": [(83, 0, 16)], "1c": [(20, 9, 0)],
    "3": [(83, 41, 8), (5, 0, 0), (131, 33, 16)],
    "5": [(20, 0, 16), (131, 65, 0), (5, 2, 8), (83, 7, 16), (131, 32, 8)],
}


def run_pooled_conv(lib, cin, n, sess, own_inputs, only=None):
    """The sessions (or session `only` alone) laid out as pool_plan lays conv 1 out: out_start = h1_off - first row.  own_inputs: one
    input buffer per session through seg_A, else one packed input and in_start.  Returns (Out, [(h1_off, rows)])."""
    idx = range(len(sess)) if only is None else [only]
    segs, mbt, ptrs, lay, keep = [], [], [], [], []
    h1_off, in_off = 0, 0
    packed = []
    for i in idx:
        T, mb, chunk = sess[i]
        L = (T - 1) // 2 + 1
        xh, xd = conv_input(cin, T, 40 + i)
        segs.append([h1_off - mb, L, 0 if own_inputs else in_off, T])
        mbt.append([mb, chunk])
        ptrs.append(xd.data_ptr())
        packed.append(xd)
        lay.append((h1_off, L - mb))
        h1_off += L - mb
        in_off += T
    out = Out(h1_off, n // 2 + 4)
    dsegs, dmb = i32(segs), i32(mbt)
    dA = torch.tensor(ptrs, dtype=torch.int64, device=DEV) if own_inputs else None
    dx = None if own_inputs else torch.cat(packed)
    a = conv_args(cin, n, dx, cin, out, h1_off, 1, 0, dsegs, len(segs), max(r for _, r in lay))
    rc = lib.ss_op_conv_gemm_rows(S(), C.byref(a), 0, P(dmb), P(dA), 1)
    assert rc == 0, f"rc {rc}"
    torch.cuda.synchronize()
    return out, lay


@pytest.mark.parametrize("own_inputs", [True, False], ids=["seg_A", "packed"])
@pytest.mark.parametrize("cfg", list(POOL_CONV))
def test_conv_pooled(lib, cfg, own_inputs):
    cin, n = (80, 128) if own_inputs else (64, 128)           # conv 1 (BK = 16, an input per session) / conv 2 (BK = 32, one packed input)
    sess, oc = POOL_CONV[cfg], n // 2
    w, b, _, _ = conv_weights(cin, n)
    out, lay = run_pooled_conv(lib, cin, n, sess, own_inputs)
    assert out.intact(row_mask(out.rows, out.ld, oc, [(o, o + r) for o, r in lay])), "a word outside the sessions' rows changed"
    got, gbits = out.f32(), out.bits()
    for i, (T, mb, chunk) in enumerate(sess):
        L = (T - 1) // 2 + 1
        ref = R.chunk_conv(conv_input(cin, T, 40 + i)[0], w, b, stride=2, pad=2, chunk=chunk, glu=True, rows=(mb, L))[mb:]
        o, r = lay[i]
        e = maxerr(got[o:o + r, :oc], ref)
        print(f"pooled conv {cfg} session {i} (T {T}, first row {mb}, chunk {chunk}): max err {e:.3g}")
        assert e < TOL, f"session {i}: max err {e}"
        alone, alay = run_pooled_conv(lib, cin, n, sess, own_inputs, only=i)
        assert alay == [(0, r)] and alone.intact(row_mask(r, alone.ld, oc, [(0, r)]))
        assert np.array_equal(alone.bits()[:, :oc], gbits[o:o + r, :oc]), f"session {i}: its bits depend on the pack"


# =====================================================================================================
# dwconv_bn_silu: ragged and by row range
# =====================================================================================================
@functools.lru_cache(maxsize=None)
def dw_params(Cc, K):
    w = rnd(Cc, K, seed=27 + K, scale=K ** -0.5)
    mean, var = rnd(Cc, seed=28) * 0.1, torch.rand(Cc, generator=torch.Generator().manual_seed(29)) + 0.5
    g, b = rnd(Cc, seed=30) * 0.1 + 1, rnd(Cc, seed=31) * 0.1
    host = tuple(t.numpy() for t in (w, mean, var, g, b))
    dev = tuple(t.to(DEV) for t in (w.t().contiguous(), mean, var, g, b))          # the kernel's weights: [K][C]
    return host, dev


def run_dw(lib, dx, ldx, rows, Cc, K, T, chunk, segs=None, nseg=0, t_begin=0, x_off_rows=0):
    _, (dwt, dm, dv, dg, db) = dw_params(Cc, min(K, 31) | 1)
    out = Out(rows, Cc + 4)
    xp = C.c_void_p(dx.data_ptr() + x_off_rows * ldx * 4)
    rc = lib.ss_op_dwconv_bn_silu_ex(S(), xp, ldx, out.ptr, out.ld, P(dwt), K, P(dm), P(dv), P(dg), P(db), 1e-5, T, Cc, chunk,
                                     P(segs), nseg, t_begin)
    return rc, out


DW_PACKS = [([70], 0, 0), ([1, 33], 8, 0), ([14, 15, 16], 16, 0), ([31, 32, 1, 70], 24, 0), ([16, 33, 15, 70], 8, 15)]   # lens, chunk, t_begin


@pytest.mark.parametrize("K", [3, 15, 31])
@pytest.mark.parametrize("Cc", [64, 80, 256, 512])
def test_dwconv_ragged(lib, Cc, K):
    (w, mean, var, g, b), _ = dw_params(Cc, K)
    ldx = Cc + 8
    for lens, chunk, tb in DW_PACKS:
        segs, at = [], 3                                    # rows 0..2 and the tail belong to no utterance
        for L in lens:
            segs.append((at, L))
            at += L
        M = at + 2
        x = rnd(M, ldx, seed=300 + len(lens))
        dx = x.to(DEV)
        ref = R.dwconv_bn_silu_ragged(x.numpy()[:, :Cc], segs, w, mean, var, g, b, chunk=chunk, t_begin=tb)
        rc, out = run_dw(lib, dx, ldx, M, Cc, K, max(lens), chunk, i32([list(s) for s in segs]), len(segs), tb)
        assert rc == 0
        written = [(s + tb, s + L) for s, L in segs if L > tb]
        assert out.intact(row_mask(M, out.ld, Cc, written)), f"pack {lens}: a word outside the utterances' rows changed"
        got, gbits = out.f32(), out.bits()
        for s, L in segs:
            if L <= tb:
                continue
            e = maxerr(got[s + tb:s + L, :Cc], ref[s + tb:s + L])
            assert e < DW_TOL, f"pack {lens} chunk {chunk} utterance of {L}: max err {e}"
            rc, alone = run_dw(lib, dx, ldx, L, Cc, K, L, chunk, t_begin=tb, x_off_rows=s)
            assert rc == 0 and alone.intact(row_mask(L, alone.ld, Cc, [(tb, L)]))
            assert np.array_equal(alone.bits()[tb:, :Cc], gbits[s + tb:s + L, :Cc]), f"pack {lens}: utterance of {L} differs from alone"


@pytest.mark.parametrize("K", [3, 15, 31])
@pytest.mark.parametrize("Cc", [64, 80, 256, 512])
def test_dwconv_row_range(lib, Cc, K):
    (w, mean, var, g, b), _ = dw_params(Cc, K)
    ldx = Cc + 8
    for T in (48, 70):
        x = rnd(T, ldx, seed=310 + T)
        dx = x.to(DEV)
        for chunk in (0, 8, 16, 24):
            ref = R.dwconv_bn_silu(x.numpy()[:, :Cc], w, mean, var, g, b, chunk=chunk)
            rc, base = run_dw(lib, dx, ldx, T, Cc, K, T, chunk)
            assert rc == 0 and base.intact(row_mask(T, base.ld, Cc, [(0, T)]))
            e = maxerr(base.f32()[:, :Cc], ref)
            assert e < DW_TOL, f"T {T} chunk {chunk}: max err {e}"
            base_bits = base.bits()[:, :Cc]
            for tb in (1, 14, 15, 16, 32, 47, T - 1):
                rc, out = run_dw(lib, dx, ldx, T, Cc, K, T, chunk, t_begin=tb)
                assert rc == 0
                assert out.intact(row_mask(T, out.ld, Cc, [(tb, T)])), f"T {T} t_begin {tb}: a word outside rows [{tb}, {T}) changed"
                assert np.array_equal(out.bits()[tb:, :Cc], base_bits[tb:]), f"T {T} chunk {chunk} t_begin {tb}: not the t_begin = 0 bits"


def test_dwconv_refusals(lib):
    dx = rnd(48, 264, seed=320).to(DEV)
    for K in (2, 30, 32, 33):
        rc, out = run_dw(lib, dx, 264, 48, 256, K, 48, 8)
        assert rc == SS_ERR_ARG and out.intact(), f"K = {K}"
    rc, out = run_dw(lib, dx, 264, 48, 256, 31, 48, 8, t_begin=-1)
    assert rc == SS_ERR_ARG and out.intact()
    rc, out = run_dw(lib, dx, 264, 48, 256, 31, 48, 8, t_begin=48)             # an empty row range: nothing to do
    assert rc == 0 and out.intact()


# =====================================================================================================
# pool_dwconv
# =====================================================================================================
SLOTS, SLOT_ROWS = 4, 96
# calls of sessions (r0, n, slot, chunk): slots not ascending, chunks mixed
POOL_DW_CALLS = [
    [(0, 1, 3, 8), (0, 40, 0, 0), (7, 9, 2, 16)],                       # r0 = 0; r0 below the half window
    [(15, 1, 2, 16), (16, 33, 3, 8), (40, 32, 1, 0), (63, 33, 0, 24)],  # two row tiles; the halo spans cache and stack inside a tile
]


@pytest.mark.parametrize("call", [0, 1])
@pytest.mark.parametrize("Cc,K", [(256, 31), (64, 15)])
def test_pool_dwconv(lib, Cc, K, call):
    (w, mean, var, g, b), (dwt, dm, dv, dg, db) = dw_params(Cc, K)
    sess_in = POOL_DW_CALLS[call]
    cache = np.full((SLOTS, SLOT_ROWS, Cc), SENT, dtype=np.int32).view(np.float32)
    table, rsess, q = [], [], 0
    for i, (r0, n, slot, chunk) in enumerate(sess_in):
        cache[slot, :r0] = rnd(r0, Cc, seed=400 + i).numpy()
        table.append([q, n, r0, r0 + n, slot, 0, chunk, 0])
        rsess.append((q, n, r0, r0 + n, slot, chunk))
        q += n
    gs = rnd(q, Cc, seed=410 + call)
    dgs = gs.to(DEV)
    dcache = Out(SLOTS * SLOT_ROWS, Cc)
    dcache.raw[GUARD:GUARD + SLOTS * SLOT_ROWS] = torch.from_numpy(cache.view(np.int32).reshape(-1, Cc)).to(DEV)
    y = Out(q, Cc)
    dtable = i32(table)
    rc = lib.ss_op_pool_dwconv(S(), P(dgs), dcache.ptr, SLOT_ROWS, y.ptr, P(dwt), K, P(dm), P(dv), P(dg), P(db), 1e-5, Cc,
                               P(dtable), len(table), max(n for _, n, _, _ in sess_in))
    assert rc == 0
    ref_y, ref_cache = R.pool_dwconv(gs.numpy(), cache, rsess, w, mean, var, g, b)
    assert y.intact(row_mask(q, Cc, Cc, [(0, q)]))
    got, gbits = y.f32(), y.bits()
    for (qs, n, r0, T, slot, chunk) in rsess:
        e = maxerr(got[qs:qs + n], ref_y[qs:qs + n])
        print(f"pool_dwconv C {Cc} K {K} (r0 {r0}, n {n}, chunk {chunk}): max err {e:.3g}")
        assert e < DW_TOL, f"(r0 {r0}, n {n}): max err {e}"
        # the same arithmetic as the row-range launch on the concatenated input
        full = torch.cat([torch.from_numpy(cache[slot, :r0].copy()), gs[qs:qs + n]]).to(DEV)
        rc, rr = run_dw(lib, full, Cc, T, Cc, K, T, chunk, t_begin=r0)
        assert rc == 0
        assert np.array_equal(rr.bits()[r0:, :Cc], gbits[qs:qs + n]), f"(r0 {r0}, n {n}): not the bits of dwconv_bn_silu from row r0"
    # the cache: rows [r0, r0 + n) of each session's slot are the stacked rows, every other word (guards included) as it was
    after = dcache.bits().reshape(SLOTS, SLOT_ROWS, Cc)
    assert np.array_equal(after, ref_cache.view(np.int32)), "the slot cache after the call"
    written = np.zeros((SLOTS * SLOT_ROWS, Cc), bool)
    written[:] = (cache.view(np.int32).reshape(-1, Cc) != SENT) | (ref_cache.view(np.int32).reshape(-1, Cc) != SENT)
    assert dcache.intact(written)


# =====================================================================================================
# pool_gather (both forms) and pool_stack_rows: exact
# =====================================================================================================
# sessions (len, k0, nf): k0 = 0, k0 = len (all from the cache), nf = k0 (nothing written back), nf = len, len = 1
GATHER = {
    "rows": {1: [(7, 3, 6)], 2: [(5, 2, 2), (4, 0, 4)], 7: [(1, 0, 1), (5, 5, 5), (3, 0, 0), (12, 4, 12), (1, 1, 1), (7, 2, 5), (6, 0, 6)]},
    "ids": {1: [(301, 44, 300)], 2: [(257, 256, 256), (200, 0, 200)],
            7: [(1, 0, 1), (300, 300, 300), (77, 0, 0), (256, 100, 256), (1, 1, 1), (130, 2, 5), (64, 0, 64)]},
}
SLOT_ORDER = [5, 0, 6, 2, 7, 1, 3]


@pytest.mark.parametrize("nsess", [1, 2, 7])
@pytest.mark.parametrize("form", ["rows", "ids"])
def test_pool_gather(lib, form, nsess):
    sess = GATHER[form][nsess]
    W, slot_rows, nslots = (256, 12, 8) if form == "rows" else (1, 301, 8)
    total = sum(L for L, _, _ in sess)
    assert total % (4 if form == "rows" else 256) != 0
    rng = np.random.default_rng(500 + nsess)
    cache = np.full((nslots, slot_rows, W), SENT, dtype=np.int32)
    tab, rtab, pre, s0 = [], [], [0], 0
    for i, (L, k0, nf) in enumerate(sess):
        slot = SLOT_ORDER[i]
        cache[slot, :k0] = rng.integers(-2 ** 30, 2 ** 30, (k0, W), dtype=np.int32)
        tab.append([pre[-1], L, k0, nf, slot, s0])
        rtab.append((L, k0, nf, slot, s0))
        pre.append(pre[-1] + L)
        s0 += L - k0
    stk = rng.integers(-2 ** 30, 2 ** 30, (max(s0, 1), W), dtype=np.int32)
    ref_out, ref_cache = R.pool_gather(stk, cache, rtab)
    dstk = torch.from_numpy(stk).to(DEV)
    dcache = Out(nslots * slot_rows, W, torch.int32)
    dcache.raw[GUARD:GUARD + nslots * slot_rows] = torch.from_numpy(cache.reshape(-1, W)).to(DEV)
    out = Out(total, W, torch.int32)
    dtab, dpre = i32(tab), i32(pre)
    if form == "rows":
        rc = lib.ss_op_pool_gather_rows(S(), out.ptr, P(dstk), dcache.ptr, slot_rows, W, P(dtab), P(dpre), nsess, total)
    else:
        rc = lib.ss_op_pool_gather_ids(S(), out.ptr, P(dstk), dcache.ptr, slot_rows, P(dtab), P(dpre), nsess, total)
    assert rc == 0
    assert np.array_equal(out.bits(), ref_out) and out.intact(np.ones((total, W), bool))
    assert np.array_equal(dcache.bits().reshape(cache.shape), ref_cache), "the slot cache after the call"
    wr = np.zeros(cache.shape, bool)
    for L, k0, nf, slot, _ in rtab:
        wr[slot, :max(k0, nf)] = True                       # rows below k0 held data before, rows [k0, nf) are written
        assert np.array_equal(ref_cache[slot, nf:], cache[slot, nf:]) and np.array_equal(ref_cache[slot, :k0], cache[slot, :k0])
    assert dcache.intact(wr.reshape(-1, W)), "a cache word outside rows [k0, nf) changed"


@pytest.mark.parametrize("nsess", [1, 2, 7])
@pytest.mark.parametrize("W", [256, 512, 1024, 12])
def test_pool_stack_rows(lib, W, nsess):
    lens = {1: [5], 2: [1, 6], 7: [1, 9, 2, 1, 17, 4, 3]}[nsess]
    rng = np.random.default_rng(600 + W)
    enc = rng.integers(-2 ** 30, 2 ** 30, (64, W), dtype=np.int32)
    src = [int(v) for v in rng.integers(0, 64 - max(lens), nsess)]
    pre = [0]
    for L in lens:
        pre.append(pre[-1] + L)
    ref = R.pool_stack_rows(enc, src, pre)
    out = Out(pre[-1], W)
    denc, dsrc, dpre = torch.from_numpy(enc).to(DEV), i32(src), i32(pre)
    rc = lib.ss_op_pool_stack_rows(S(), out.ptr, P(denc), W, P(dsrc), P(dpre), nsess, pre[-1])
    assert rc == 0
    assert np.array_equal(out.bits(), ref) and out.intact(np.ones((pre[-1], W), bool))


def test_pool_launcher_refusals(lib):
    Cc = 256
    _, (dwt, dm, dv, dg, db) = dw_params(Cc, 31)
    gs, tab = rnd(8, Cc, seed=700).to(DEV), i32([[0, 8, 0, 8, 0, 0, 0, 0]])
    for K, nsess in ((30, 1), (2, 1), (33, 1), (31, 0), (31, -1)):
        cache, y = Out(SLOT_ROWS, Cc), Out(8, Cc)
        rc = lib.ss_op_pool_dwconv(S(), P(gs), cache.ptr, SLOT_ROWS, y.ptr, P(dwt), K, P(dm), P(dv), P(dg), P(db), 1e-5, Cc, P(tab), nsess, 8)
        assert rc == SS_ERR_ARG and cache.intact() and y.intact(), f"K {K} nsess {nsess}"
    gt, pre = i32([[0, 8, 0, 8, 0, 0]]), i32([0, 8])
    for nsess in (0, -1):
        cache, out = Out(12, 256), Out(8, 256)
        assert lib.ss_op_pool_gather_rows(S(), out.ptr, P(gs), cache.ptr, 12, 256, P(gt), P(pre), nsess, 8) == SS_ERR_ARG
        assert lib.ss_op_pool_gather_ids(S(), out.ptr, P(gs), cache.ptr, 12, P(gt), P(pre), nsess, 8) == SS_ERR_ARG
        assert lib.ss_op_pool_stack_rows(S(), out.ptr, P(gs), 256, P(pre), P(pre), nsess, 8) == SS_ERR_ARG
        assert cache.intact() and out.intact()
    for W in (254, 6, 1028, 2048, 0):
        out = Out(8, 256)
        assert lib.ss_op_pool_stack_rows(S(), out.ptr, P(gs), W, P(pre), P(pre), 1, 8) == SS_ERR_ARG and out.intact(), f"W {W}"
    out, cache = Out(8, 256), Out(12, 256)
    assert lib.ss_op_pool_gather_rows(S(), out.ptr, P(gs), cache.ptr, 12, 128, P(gt), P(pre), 1, 8) == SS_ERR_ARG and out.intact()


# =====================================================================================================
# LayerNorm: strided, in place, large mean
# =====================================================================================================
def run_ln(lib, x, D, M, ldx, ldy, in_place, g, b):
    """x [M, D] host.  Out of place: x rows at stride ldx (gaps hold 1e4), y sentinel at stride ldy.  In place: x sits in the
    sentinel-filled output buffer at stride ldy."""
    dg, db = g.to(DEV), b.to(DEV)
    out = Out(M, ldy)
    if in_place:
        out.t[GUARD:GUARD + M, :D] = x.to(DEV)
        rc = lib.ss_op_layernorm(S(), out.ptr, ldy, out.ptr, ldy, P(dg), P(db), M, D, 1e-5)
    else:
        dx = torch.full((M, ldx), 1.0e4, device=DEV)
        dx[:, :D] = x.to(DEV)
        rc = lib.ss_op_layernorm(S(), P(dx), ldx, out.ptr, ldy, P(dg), P(db), M, D, 1e-5)
    return rc, out


@pytest.mark.parametrize("M", [1, 3, 4, 5, 131])
@pytest.mark.parametrize("D", [64, 128, 256, 512, 1024])
def test_layernorm_strided_and_in_place(lib, D, M):
    """On O(1) data the bar of test_ops_gpu.py::test_layernorm.  On rows of mean 100 and standard deviation 0.01 the bar is 4 x the
    maximum error of a plain two-pass LayerNorm in NumPy float32 on the same input (the margin: summation order across 64 lanes)."""
    g, b = rnd(D, seed=17) * 0.1 + 1, rnd(D, seed=18) * 0.1
    x = rnd(M, D, seed=16) * 3 + 1
    ref = R.layernorm(x.numpy(), g.numpy(), b.numpy())
    for in_place in (False, True):
        rc, out = run_ln(lib, x, D, M, D + 12, D + 4, in_place, g, b)
        assert rc == 0
        assert out.intact(row_mask(M, out.ld, D, [(0, M)])), f"in_place {in_place}: a word outside the rows' D columns changed"
        e = maxerr(out.f32()[:, :D], ref)
        assert e < LN_TOL, f"in_place {in_place}: max err {e}"
    big = rnd(M, D, seed=19) * 0.01 + 100.0
    ref = R.layernorm(big.numpy(), g.numpy(), b.numpy())
    yard = maxerr(R.layernorm(big.numpy(), g.numpy(), b.numpy(), dtype=np.float32), ref)
    for in_place in (False, True):
        rc, out = run_ln(lib, big, D, M, D + 12, D + 4, in_place, g, b)
        assert rc == 0 and out.intact(row_mask(M, out.ld, D, [(0, M)]))
        e = maxerr(out.f32()[:, :D], ref)
        print(f"layernorm D {D} M {M} in_place {in_place} mean 100 / std 0.01: float32 two-pass yardstick {yard:.4g}, kernel {e:.4g}")
        assert e <= 4 * yard, f"D {D} M {M} in_place {in_place}: kernel error {e:.4g} > 4 x the float32 two-pass yardstick {yard:.4g}"


def test_layernorm_refuses_an_uninstantiated_width(lib):
    g, b = rnd(96, seed=17), rnd(96, seed=18)
    rc, out = run_ln(lib, rnd(5, 96, seed=16), 96, 5, 96, 100, False, g, b)
    assert rc == SS_ERR_ARG and out.intact()
