"""GPU parity of the row-tile linear kernel (csrc/rtlin.hip): every K = 256 linear of more than 192 rows -- encoder QKV /
attention output / pointwise convs / input projection, CTC heads, MT cross K|V -- against torch float64, across epilogues, the
LayerNorm prologue, GLU, ragged last tiles and forced grids (units are independent: any grid must give the same bits), and against
the LDS-tiled kernel it replaces (ss_debug_rtlin(0, 0)).

The second half of the file puts the kernel on launch() of tests/test_gemm_routes_gpu.py (guard rows and padded columns of 1e4 around
the inputs, NaN-started outputs with guard rows and gap columns that must stay NaN, exactly one launch of rt_linear<48,256> in the
census, float64 at TOL = 2e-4): padded leading dimensions, LayerNorm linears of 1 .. 192 rows in the pack-invariant mode, parts with
fewer units than the workgroup has waves, parts that start in mid-tile, rows with a large mean -- and, for everything without a
LayerNorm, bit equality of every element with the LDS-tiled blocked-chain kernel under canon = 1.  Its accuracy table, with that of
tests/test_rtlin_kb_gpu.py: profiles/rtlin_accuracy.txt."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from test_slab_ops_gpu import bits, stop_after_a_gpu_error  # noqa: F401
from test_gemm_routes_gpu import NONE, RELU, ROUTE_WORST, SILU, Worst, canon_tile, cdiv, launch

pytestmark = pytest.mark.gpu
K = 256


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def run(lib, x, W, b, ln=None, R=None, act=0, alpha=1.0, glu=0, inplace_r=False):
    from streamspeech_amd import lib as L
    M, N = x.shape[0], W.shape[0]
    oc = N // 2 if glu else N
    dx, dW = x.contiguous().cuda(), W.contiguous().cuda()
    db = None if b is None else b.cuda()
    dR = None if R is None else R.contiguous().cuda()
    dC = dR if inplace_r else torch.full((M, oc), float("nan")).cuda()
    if ln is None:
        rc = lib.ss_op_conv_gemm(S(), P(dx), K, P(dW), P(db), P(dR), oc, None, 0, P(dC), oc, M, N, K, 1, 1, 1, 0, M, 0, 0, 0.1, act,
                                 alpha, 0.0, glu)
    else:
        dg, dbt = ln[0].cuda(), ln[1].cuda()
        rc = lib.ss_op_ln_linear(S(), P(dx), K, P(dg), P(dbt), P(dW), P(db), P(dR), oc, P(dC), oc, M, N, K, act, alpha, glu)
    L.check(rc, "linear")
    torch.cuda.synchronize()
    return dC.cpu()


def reference(x, W, b, ln=None, R=None, act=0, alpha=1.0, glu=0):
    x, W = x.double(), W.double()
    if ln is not None:
        x = F.layer_norm(x, (K,), ln[0].double(), ln[1].double(), 1e-5)
    y = F.linear(x, W, None if b is None else b.double())
    if glu:
        n = W.shape[0]
        y = y.view(-1, n // 32, 2, 16)
        return (y[:, :, 0] * torch.sigmoid(y[:, :, 1])).reshape(-1, n // 2)      # [16 value | 16 gate] blocks (pack-time interleave)
    y = F.silu(y) if act == 1 else F.relu(y) if act == 2 else y
    y = y * alpha
    return y if R is None else y + R.double()


def class_launches(lib, name):
    for c in range(lib.ss_prof_num_classes()):
        if lib.ss_prof_class_name(c).decode() == name:
            n = C.c_int64()
            lib.ss_prof_totals(c, None, None, C.byref(n))
            return n.value
    raise KeyError(name)


@pytest.mark.parametrize("M,N,bias,ln,res,act,alpha,glu,grid", [
    (193, 768, True, True, False, 0, 1.0, 0, 60), (240, 256, True, False, True, 0, 1.0, 0, 20), (700, 512, False, True, False, 0, 1.0, 1, 256),
    (700, 512, True, False, False, 0, 1.0, 1, 3), (4200, 768, True, True, False, 0, 1.0, 0, 0), (4200, 256, True, False, True, 0, 0.5, 0, 700),
    (4200, 2048, True, True, False, 1, 1.0, 0, 0), (4200, 1024, True, False, False, 2, 1.0, 0, 97), (4173, 6000, True, False, False, 0, 1.0, 0, 0),
    (12001, 16, False, False, False, 0, 1.0, 0, 1), (12001, 512, False, True, False, 0, 1.0, 1, 0), (333, 6000, False, False, False, 0, 1.0, 0, 0)])
def test_row_tile_linear_vs_float64(lib, M, N, bias, ln, res, act, alpha, glu, grid):
    x = rnd(M, K, seed=M + N)
    W = rnd(N, K, seed=N + 1, scale=K ** -0.5)
    b = rnd(N, seed=N + 2, scale=0.1) if bias else None
    lnp = (1 + rnd(K, seed=5, scale=0.1), rnd(K, seed=6, scale=0.1)) if ln else None
    R = rnd(M, N, seed=7) if res else None
    n0 = class_launches(lib, "rt_linear<48,256>")
    assert lib.ss_debug_rtlin(grid, 1) == 0
    try:
        got = run(lib, x, W, b, lnp, R, act, alpha, glu, inplace_r=res)
        assert lib.ss_debug_rtlin(5 if grid != 5 else 11, 1) == 0
        again = run(lib, x, W, b, lnp, R, act, alpha, glu)
    finally:
        lib.ss_debug_rtlin(0, 1)
    assert class_launches(lib, "rt_linear<48,256>") == n0 + 2, "the row-tile kernel must have taken both launches"
    ref = reference(x, W, b, lnp, R, act, alpha, glu)
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got.double() - ref).abs().max().item()
    assert err < 2e-5, f"max err {err}"
    assert torch.equal(got, again), "units are independent: the grid must not change a bit"


def test_row_tile_linear_vs_the_tiled_kernel(lib):
    """Same launches on the LDS-tiled kernel (ss_debug_rtlin(0, 0)): agreement to summation order."""
    M, N = 4500, 768
    x, W, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3, scale=0.1)
    R = rnd(M, N, seed=4)
    new = run(lib, x, W, b, None, R, 1, 0.5)
    n0 = class_launches(lib, "rt_linear<48,256>")
    lib.ss_debug_rtlin(0, 0)
    try:
        old = run(lib, x, W, b, None, R, 1, 0.5)
    finally:
        lib.ss_debug_rtlin(0, 1)
    assert class_launches(lib, "rt_linear<48,256>") == n0
    assert (new - old).abs().max() < 1e-5


# =====================================================================================================
# on the guarded launch harness of tests/test_gemm_routes_gpu.py
# =====================================================================================================
RT = "rt_linear<48,256>"
BM = 48                        # rows of a tile (RT_BM)


@pytest.fixture(scope="module", autouse=True)
def worst_table():
    yield
    print()
    for route, (err, n) in ROUTE_WORST.items():
        if route.startswith("rt_linear") and not route.startswith("rt_linear_kb"):
            print(f"WORST {route}: {err:.3e} over {n} launches")


@pytest.fixture()
def hook(lib):
    """set(grid, on): ss_debug_rtlin; the default is back after the test."""
    def set_hook(grid=0, on=1):
        assert lib.ss_debug_rtlin(grid, on) == 0
    try:
        yield set_hook
    finally:
        lib.ss_debug_rtlin(0, 1)


def padded(N, glu=0):
    return dict(lda=K + 4, ldc=(N // 2 if glu else N) + 4, ldr=N + 12)


def on_rt(lib, hook, what, *, grid=0, canon=1, refs=None, **kw):
    """One launch on rt_linear with the harness's checks; LayerNorm linears through ss_op_ln_linear_ex, the others through the conv
    entry.  Returns the host copy of C."""
    hook(grid, 1)
    w = Worst("rt_linear" + (" LayerNorm" if kw.get("ln") else "") + (" GLU" if kw.get("glu") else ""))
    out = launch(lib, RT, f"{what} grid={grid} canon={canon}", w, Cin=K, canon=canon, entry="lin" if kw.get("ln") else "conv", refs=refs,
                 **kw)[0]
    w.done()
    return out


def on_tiles(lib, hook, what, refs, **kw):
    """The same launch on the LDS-tiled blocked-chain kernel (canon = 1 with the row-tile kernel off); no LayerNorm form exists there."""
    assert not kw.get("ln")
    hook(0, 0)
    w = Worst("rt_linear's bit oracle: conv_gemm BLK tiles")
    out = launch(lib, canon_tile(kw["M"], kw["N"], K, kw.get("glu", 0)), f"{what} on the tiled kernel", w, Cin=K, canon=1, refs=refs, **kw)[0]
    w.done()
    return out


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), f"{what}: not the same bits ({int((bits(a) != bits(b)).sum())} elements differ)"


def both(lib, hook, what, grids, **kw):
    """rt_linear under canon = 1 at every forced grid (M >= 193: rtlin_eligible) and the tiled kernel: one result, bit for bit."""
    assert kw["M"] >= 193 and all(g > 0 for g in grids)
    refs = {}
    outs = [on_rt(lib, hook, what, grid=g, refs=refs, **kw) for g in grids]
    for g, o in zip(grids[1:], outs[1:]):
        same_bits(outs[0], o, f"{what}: grid {grids[0]} against grid {g}")
    same_bits(outs[0], on_tiles(lib, hook, what, refs, **kw), f"{what}: against the tiled kernel")


@pytest.mark.parametrize("M,N,glu,extra", [(193, 768, 0, {}), (700, 512, 1, {}), (4200, 256, 0, dict(R=True, alpha=0.5))],
                         ids=["193x768", "700x512-glu", "4200x256-residual"])
def test_padded_leading_dimensions(lib, hook, M, N, glu, extra):
    """lda = 260, ldc = N + 4, ldr = N + 12, as callers that write into a slice of a wider buffer pass them."""
    assert padded(N)["lda"] == 260
    both(lib, hook, f"({M}, {N}) padded ld", [60, 11], M=M, N=N, glu=glu, seed=2000, **padded(N, glu), **extra)
    if not extra:
        on_rt(lib, hook, f"({M}, {N}) LayerNorm padded ld", grid=60, M=M, N=N, glu=glu, ln=True, seed=2001, **padded(N, glu))


@pytest.mark.parametrize("N,glu", [(768, 0), (512, 1)], ids=["768", "512-glu"])
@pytest.mark.parametrize("M", [1, 47, 48, 49, 95, 192])
def test_layernorm_linear_below_the_row_threshold(lib, hook, M, N, glu):
    """Under canon = 1 a LayerNorm linear of ANY row count takes this kernel (launch_canon: `a.ln_g || rtlin_eligible`) -- a single
    streaming utterance is such a launch.  Nothing forced: the grid is launch_rtlin's own (at most U / 4 workgroups)."""
    assert M < 193
    on_rt(lib, hook, f"({M}, {N}) LayerNorm", M=M, N=N, glu=glu, ln=True, seed=2100, **padded(N, glu))


SMALL_PARTS = [(16, 0), (32, 1), (96, 1), (48, 0)]          # units per tile: 1, 1, 3, 3 -- fewer than the four waves of a workgroup


@pytest.mark.parametrize("N,glu", SMALL_PARTS, ids=[f"N{n}{'-glu' if g else ''}" for n, g in SMALL_PARTS])
@pytest.mark.parametrize("M", [193, 300])
def test_parts_with_fewer_units_than_waves(lib, hook, M, N, glu):
    """Every part has at most NU <= 3 units, so one to three waves of every workgroup have my_n <= 0 and skip the contraction between
    the barriers.  Grid 1: one workgroup walks every tile; 7: parts of less than a tile's units at NU = 3; tiles x NU: one unit each."""
    nu = N // 32 if glu else N // 16
    assert nu < 4
    both(lib, hook, f"({M}, {N}{' glu' if glu else ''})", [1, 7, cdiv(M, BM) * nu], M=M, N=N, glu=glu, seed=2200)
    on_rt(lib, hook, f"({M}, {N}{' glu' if glu else ''}) LayerNorm", grid=7, M=M, N=N, glu=glu, ln=True, seed=2201)


@pytest.mark.parametrize("bias", [True, False])
def test_glu_with_and_without_bias(lib, hook, bias):
    both(lib, hook, f"(700, 512 glu) bias={bias}", [256, 3], M=700, N=512, glu=1, bias=bias, seed=2300)
    on_rt(lib, hook, f"(700, 512 glu) LayerNorm bias={bias}", grid=256, M=700, N=512, glu=1, bias=bias, ln=True, seed=2301)


def test_prime_grid_parts_start_in_mid_tile(lib, hook):
    """15 tiles x 48 units on 13 workgroups: 720 / 13 is no whole number of tiles, so parts begin and end inside a tile (ka > 0) and a
    tile's units are shared by two workgroups."""
    M, N, G = 700, 768, 13
    U = cdiv(M, BM) * (N // 16)
    assert U % G != 0 and any((w * U // G) % (N // 16) for w in range(G))
    both(lib, hook, "(700, 768) relu", [G, 60], M=M, N=N, act=RELU, seed=2400)
    on_rt(lib, hook, "(700, 768) LayerNorm", grid=G, M=M, N=N, ln=True, seed=2401)


def test_epilogues(lib, hook):
    M, N = 240, 256
    both(lib, hook, "(240, 256) silu * 0.5 + R in place", [20, 7], M=M, N=N, act=SILU, alpha=0.5, inplace=True, ldc=N + 4, ldr=N + 4,
         seed=2500)
    both(lib, hook, "(240, 256) relu + R", [20, 7], M=M, N=N, act=RELU, R=True, **padded(N), seed=2501)
    both(lib, hook, "(240, 256) no bias", [20, 7], M=M, N=N, bias=False, seed=2502)


@pytest.mark.parametrize("N,glu", [(768, 0), (512, 1)], ids=["768", "512-glu"])
def test_layernorm_of_rows_with_a_large_mean(lib, hook, N, glu):
    """Rows of mean 100 and spread 1.  The bound is MEASURED (tol = "f32 chain" of the harness): 4 x the max abs error, against float64,
    of a float32 two-pass LayerNorm + float32 matmul of the same data on the host; a one-pass E[x^2] - mean^2 would lose four digits."""
    on_rt(lib, hook, f"(300, {N}) LayerNorm, row mean 100", grid=7, canon=0, M=300, N=N, glu=glu, ln=True, mean=100.0, tol="f32 chain",
          seed=2600)
    on_rt(lib, hook, f"(300, {N}) LayerNorm, row mean 100", canon=1, M=300, N=N, glu=glu, ln=True, mean=100.0, tol="f32 chain", seed=2600)
