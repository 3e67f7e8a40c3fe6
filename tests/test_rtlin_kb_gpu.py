"""Op-level tests of rt_linear_kb_kernel<UW> (csrc/rtlin.hip): the K = 512 ... 8192 linears of the pack-invariant mode (canon = 1) --
T2U encoder / unit-decoder QKV, output projections, both FFN halves -- form by form: the three template widths (UW = 1, 2, 4
sixteen-column units per wave) and the two unit orders (a contiguous range of (row tile, column group) units per workgroup; the
XCD-aware order `xmap` with its own index arithmetic), forced through ss_debug_rtlin_kb at the smallest shapes at which each path can
go wrong, and as launch_rtlin_kb picks them by itself at row counts derived from the device's CU count.

Every launch goes through launch() of tests/test_gemm_routes_gpu.py with canon = 1 (the kernel is reachable only from launch_canon) and
gets that harness's checks: inputs between guard rows of 1e4 and padded input columns of 1e4; outputs that start as NaN with guard rows
and gap columns; rc == 0, the op's elements finite and everything else still NaN; exactly one launch, of class rt_linear_kb<48,256>.
On top of that ss_debug_rtlin_kb_last must report the expected {UW, NCG, G, xmap}, restated here in kb_form() from launch_rtlin_kb.

Two oracles per launch: float64 (tests/gemm_ref.py) at TOL = 2e-4 max abs, and BIT equality of every output element with the same
launch on the LDS-tiled blocked-chain kernel conv_gemm_kernel<.., BLK = true> (ss_debug_rtlin(0, 0)), which rtlin.hip and gemm.hpp
document.  The float64 oracle covers every row where M N K <= 2e9, else a seeded sample (float64_rows); the bit oracle always covers
every element, so no row is left to neither.  The K = 2048 cases also hold the project's chain-quality bar of
tests/test_pack_invariance_gpu.py: RMS error against float64 <= 1.1 x that of torch's CPU float32 matmul on the same operands.
The accuracy table of a run: profiles/rtlin_accuracy.txt.
"""
import ctypes as C
import os

import pytest
import torch

from test_slab_ops_gpu import TOL, bits, census, lib, stop_after_a_gpu_error, took_since  # noqa: F401
from test_gemm_routes_gpu import NONE, RELU, ROUTE_WORST, SILU, SS_ERR_ARG, Worst, canon_tile, cdiv, launch

pytestmark = pytest.mark.gpu

for _knob in sorted(os.environ):
    if (_knob == "SS_NO_RTLIN" or _knob.startswith("SS_RTLIN_")) and os.environ[_knob]:       # (SS_RTLIN_KB_* too)
        pytestmark = [pytest.mark.gpu, pytest.mark.skip(reason=f"{_knob} is set: the dispatch of the row-tile linears is not the default")]

KB = "rt_linear_kb<48,256>"
BM = 48                        # rows of a tile (RT_BM)
CONTIGUOUS, HEURISTIC, XCD = 0, 1, 2      # the order argument of ss_debug_rtlin_kb
KB_MIN_UNITS = 256             # Dispatch::rt_kb_min_units: (tile, 64-column group) units from which an unforced launch takes the kernel


@pytest.fixture(scope="module", autouse=True)
def worst_table():
    yield
    print()
    for route, (err, n) in ROUTE_WORST.items():
        if route.startswith("rt_linear_kb"):
            print(f"WORST {route}: {err:.3e} over {n} launches")


@pytest.fixture(scope="module")
def cus(lib):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture()
def hooks(lib):
    """set(grid, on, uw, order): ss_debug_rtlin(grid, on) + ss_debug_rtlin_kb(uw, order); the defaults are back after the test."""
    def set_hooks(grid=0, on=1, uw=0, order=HEURISTIC):
        assert lib.ss_debug_rtlin(grid, on) == 0 and lib.ss_debug_rtlin_kb(uw, order) == 0
    try:
        yield set_hooks
    finally:
        lib.ss_debug_rtlin(0, 1)
        lib.ss_debug_rtlin_kb(0, HEURISTIC)


def kb_form(M, N, cus, uw=0, order=HEURISTIC, grid=0):
    """{UW, NCG, G, xmap} of launch_rtlin_kb, or None where it refuses.  Width: 4 units per wave, halved while the launch then has
    fewer (tile, column group) units than three workgroups per CU.  Grid: the forced one or 3 per CU, clamped to the unit count --
    except under a forced order with a forced grid, which runs as given.  xmap: forced (its conditions G % 8 == 0 and
    (G / 8) % NCG == 0, or a refusal), or by itself when nothing is forced, G == 3 CUs, CUs % 8 == 0 and every workgroup has >= 2 units."""
    tiles = cdiv(M, BM)
    if uw == 0:
        uw = 4
        while uw > 1 and tiles * (N // (64 * uw)) < 3 * cus:
            uw //= 2
    ncg = N // (64 * uw)
    U, G = tiles * ncg, grid or 3 * cus
    if order == XCD:
        return (uw, ncg, G, 1) if G % 8 == 0 and (G // 8) % ncg == 0 else None
    if G > U and not (order == CONTIGUOUS and grid):
        G = U
    xmap = order == HEURISTIC and not grid and G == 3 * cus and cus % 8 == 0 and (G // 8) % ncg == 0 and U >= 2 * G
    return (uw, ncg, max(G, 1), int(xmap))


def last_form(lib):
    a = (C.c_int32 * 4)()
    assert lib.ss_debug_rtlin_kb_last(a) == 0
    return tuple(a)


def on_kb(lib, hooks, what, cus, refs, *, uw=0, order=HEURISTIC, grid=0, **kw):
    """One launch on rt_linear_kb under the given hooks, the harness's checks + the reported form; returns the host copy of C."""
    form = kb_form(kw["M"], kw["N"], cus, uw, order, grid)
    assert form is not None and (uw == 0 or form[0] == uw)
    hooks(grid, 1, uw, order)
    w = Worst(f"rt_linear_kb UW={form[0]} {'XCD-aware' if form[3] else 'contiguous'}{'' if (uw or grid or order != HEURISTIC) else ', unforced'}")
    out = launch(lib, KB, f"{what} uw={uw} order={order} grid={grid} -> UW, NCG, G, xmap = {form}", w, canon=1, refs=refs, **kw)[0]
    w.done()
    assert last_form(lib) == form, f"{what}: the launch reports {last_form(lib)}, expected {form}"
    return out


def on_tiles(lib, hooks, what, refs, **kw):
    """The same launch on the LDS-tiled blocked-chain kernel (row-tile kernels off): the tile class of launch_canon, same checks."""
    hooks(0, 0)
    before = last_form(lib)
    w = Worst("rt_linear_kb's bit oracle: conv_gemm BLK tiles")
    out = launch(lib, canon_tile(kw["M"], kw["N"], kw["Cin"], kw.get("glu", 0)), f"{what} on the tiled kernel", w, canon=1, refs=refs, **kw)[0]
    w.done()
    assert last_form(lib) == before
    return out


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), f"{what}: not the same bits ({int((bits(a) != bits(b)).sum())} elements differ)"


def chain_quality(out, refs, M, N, rows, what):
    """RMS error against float64 of the kernel and of torch's CPU float32 matmul on the same operands (a launch with no epilogue)."""
    sel = torch.arange(M) if rows is None else rows
    ref = refs["ref"][0]
    cpu = (refs["x"][sel] @ refs["w"].t()).double()
    e_hip = float(((out[sel][:, :N].double() - ref) ** 2).mean().sqrt())
    e_cpu = float(((cpu - ref) ** 2).mean().sqrt())
    print(f"{what}: rms vs float64: HIP {e_hip:.3e}, torch CPU {e_cpu:.3e}, ratio {e_hip / e_cpu:.3f}")
    assert e_hip <= 1.1 * e_cpu, f"{what}: rms {e_hip} against torch CPU's {e_cpu}"


# =====================================================================================================
# forced forms at small shapes
# =====================================================================================================
UWS, KS, NS, MS = (1, 2, 4), (512, 768, 2048), (256, 512, 768, 2048), (1, 47, 48, 49, 97, 300)
GRIDS = ("1", "5", "U", "U+3")                  # U: the unit count; U + 3: more workgroups than units


def forced_cases():
    """Six cases per width, one per row count; N, K and the grid walk their axes with a shift per width, so every value of every axis
    meets every UW and every (UW, K) pair appears (asserted below).  2, 3 and 8 k-blocks: the ring prefetch crosses a block boundary and
    the first block initialises the running total; N = 256 at UW = 4 is a tile of one column group, 768 at UW = 4 gives NCG = 3.
    K = 2048 never meets M = 1: the chain-quality bar needs more than one row of samples."""
    out = []
    for ui, uw in enumerate(UWS):
        for i, M in enumerate(MS):
            out.append((uw, M, NS[(i + ui) % 4], KS[(i + (1 if ui == 1 else 0)) % 3], GRIDS[(i + 2 * ui + 1) % 4]))
    return out


FORCED = forced_cases()
for _uw in UWS:
    _mine = [c for c in FORCED if c[0] == _uw]
    assert {c[1] for c in _mine} == set(MS) and {c[2] for c in _mine} == set(NS) and {c[3] for c in _mine} == set(KS)
    assert {c[4] for c in _mine} == set(GRIDS)
assert all(M >= 47 for _, M, _, K, _ in FORCED if K == 2048)
assert (4, 256) in {(c[0], c[2]) for c in FORCED} and (4, 768) in {(c[0], c[2]) for c in FORCED}


def forced_grid(g, M, N, uw):
    U = cdiv(M, BM) * (N // (64 * uw))
    return {"1": 1, "5": 5, "U": U, "U+3": U + 3}[g]


@pytest.mark.parametrize("uw,M,N,K,g", FORCED, ids=[f"UW{u}-{m}x{n}x{k}-G{g}" for u, m, n, k, g in FORCED])
def test_forced_width(lib, hooks, cus, uw, M, N, K, g):
    """The contiguous order at a forced grid, used as given: grid 5 cuts the unit range unevenly (and leaves workgroups without a unit
    where U < 5), U + 3 has three workgroups past the last unit.  The U + 3 cases also run under the launcher's own order, which clamps
    the grid to U.  K = 2048: no epilogue, for the chain-quality bar; else bias + ReLU * 0.5 + residual on padded leading dimensions."""
    grid = forced_grid(g, M, N, uw)
    plain = K == 2048
    kw = dict(M=M, N=N, Cin=K, seed=1000 + uw, bias=not plain)
    if not plain:
        kw.update(act=RELU, alpha=0.5, R=True, lda=K + 8, ldc=N + 4, ldr=N + 12)
    refs, what = {}, f"({M}, {N}, {K})"
    got = on_kb(lib, hooks, what, cus, refs, uw=uw, order=CONTIGUOUS, grid=grid, **kw)
    assert last_form(lib)[2] == grid
    if g == "U+3":
        clamped = on_kb(lib, hooks, what, cus, refs, uw=uw, order=HEURISTIC, grid=grid, **kw)
        assert last_form(lib)[2] == grid - 3
        same_bits(clamped, got, f"{what} grid U + 3 clamped to U")
    same_bits(got, on_tiles(lib, hooks, what, refs, **kw), f"{what} UW={uw} against the tiled kernel")
    if plain:
        chain_quality(got, refs, M, N, None, f"{what} UW={uw}")


def test_longest_contraction(lib, hooks, cus):
    """K = 8192, the bound of rtlin_kb_shape_ok: 32 k-blocks; N = 256 at UW = 4 is one column group per tile, M = 49 two tiles."""
    kw = dict(M=49, N=256, Cin=8192, seed=1100, act=SILU, R=True)
    refs, what = {}, "(49, 256, 8192)"
    got = on_kb(lib, hooks, what, cus, refs, uw=4, order=CONTIGUOUS, grid=2, **kw)
    same_bits(got, on_tiles(lib, hooks, what, refs, **kw), what)


def test_contraction_past_the_bound_is_not_taken(lib, hooks):
    """K = 8448 > 8192: rtlin_kb_shape_ok is false, the launch stays on the tiles."""
    hooks(2, 1, 4, CONTIGUOUS)
    w = Worst("rt_linear_kb's bit oracle: conv_gemm BLK tiles")
    launch(lib, canon_tile(49, 256, 8448), "(49, 256, 8448)", w, M=49, N=256, Cin=8448, canon=1, seed=1101)
    w.done()


# =====================================================================================================
# epilogue
# =====================================================================================================
@pytest.mark.parametrize("res", ["none", "separate", "in-place"])
def test_epilogue(lib, hooks, cus, res):
    """97 x 512 x 512 at UW = 2 (NCG = 4, three tiles, the last of one row): bias x activation x alpha with no residual, a separate
    one (ldr = N + 12) and C == R; lda = K + 8 and ldc = N + 4 throughout."""
    M, N, K = 97, 512, 512
    for bias in (True, False):
        for act in (NONE, SILU, RELU):
            for alpha in (1.0, 0.5):
                kw = dict(M=M, N=N, Cin=K, seed=1200, bias=bias, act=act, alpha=alpha, lda=K + 8, ldc=N + 4)
                if res == "separate":
                    kw.update(R=True, ldr=N + 12)
                elif res == "in-place":
                    kw.update(inplace=True, ldr=N + 4)
                refs, what = {}, f"(97, 512, 512) bias={bias} act={act} alpha={alpha} residual {res}"
                got = on_kb(lib, hooks, what, cus, refs, uw=2, order=CONTIGUOUS, grid=5, **kw)
                same_bits(got, on_tiles(lib, hooks, what, refs, **kw), what)


# =====================================================================================================
# the XCD-aware order, forced
# =====================================================================================================
# (G, NCG) -> (UW, N, K): N / (64 UW) column groups per tile
XMAP = {(8, 1): (4, 256, 512), (16, 2): (2, 256, 512), (64, 4): (1, 256, 512), (48, 6): (2, 768, 768), (64, 8): (1, 512, 512)}


def xmap_walk(G, ncg, tiles):
    """The kernel's unit loop under xmap restated: workgroup w sits at XCD index w % 8 with local index q = w / 8 and takes, in step
    it, (tile, group) = ((it tps + q / NCG) 8 + w % 8, q % NCG), tps = G / 8 / NCG.  Returns how often every unit is visited."""
    tps = G // 8 // ncg
    seen = {}
    for w in range(G):
        xx, q = w % 8, w // 8
        first = (q // ncg) * 8 + xx
        nit = cdiv(tiles - first, tps * 8) if first < tiles else 0
        for it in range(nit):
            unit = ((it * tps + q // ncg) * 8 + xx, q % ncg)
            seen[unit] = seen.get(unit, 0) + 1
    return seen


@pytest.mark.parametrize("G,ncg", list(XMAP), ids=[f"G{g}-NCG{n}" for g, n in XMAP])
def test_forced_xcd_order(lib, hooks, cus, G, ncg):
    """1, 7, 8, 9, 8 tps and 8 tps + 3 row tiles (the last one ragged): XCD indices with no tile, with one, and a ragged last step.
    Each against float64, against the contiguous order at the same grid and against the tiled kernel, bit for bit."""
    uw, N, K = XMAP[G, ncg]
    assert N // (64 * uw) == ncg and G % 8 == 0 and (G // 8) % ncg == 0
    tps = G // 8 // ncg
    for tiles in sorted({1, 7, 8, 9, 8 * tps, 8 * tps + 3}):
        assert xmap_walk(G, ncg, tiles) == {(t, c): 1 for t in range(tiles) for c in range(ncg)}      # (the order as documented is a cover)
        M = tiles * BM - 5
        kw = dict(M=M, N=N, Cin=K, seed=1300 + tiles, act=RELU, R=True, ldc=N + 4)
        refs, what = {}, f"({M}, {N}, {K}) {tiles} tiles, tps={tps}"
        got = on_kb(lib, hooks, what, cus, refs, uw=uw, order=XCD, grid=G, **kw)
        assert last_form(lib) == (uw, ncg, G, 1)
        same_bits(got, on_kb(lib, hooks, what, cus, refs, uw=uw, order=CONTIGUOUS, grid=G, **kw), f"{what} against the contiguous order")
        same_bits(got, on_tiles(lib, hooks, what, refs, **kw), f"{what} against the tiled kernel")


@pytest.mark.parametrize("G,ncg,uw,N", [(12, 2, 2, 256), (16, 3, 4, 768)])
def test_forced_xcd_order_refuses_a_grid_it_cannot_take(lib, hooks, cus, G, ncg, uw, N):
    """G % 8 != 0, and (G / 8) % NCG != 0: SS_ERR_ARG, nothing booked, nothing written, no fall-back to the contiguous order."""
    assert N // (64 * uw) == ncg and kb_form(300, N, cus, uw, XCD, G) is None
    hooks(G, 1, uw, XCD)
    before = last_form(lib)
    launch(lib, None, f"(300, {N}, 512) forced XCD-aware order at G={G}, NCG={ncg}", Worst("refusals"), M=300, N=N, Cin=512, canon=1,
           expect_rc=SS_ERR_ARG)
    assert last_form(lib) == before


def test_hook_arguments(lib, hooks):
    hooks()
    for uw, order in [(3, 1), (8, 1), (-1, 1), (0, 3), (0, -2)]:
        assert lib.ss_debug_rtlin_kb(uw, order) == SS_ERR_ARG
    assert lib.ss_debug_rtlin_kb_last(None) == SS_ERR_ARG


def test_xcd_order_gives_the_same_bits_every_time(lib, hooks, cus):
    """Units are independent -- nothing is reduced across waves or workgroups: five launches, one result."""
    uw, N, K = XMAP[64, 4]
    kw = dict(M=19 * BM - 5, N=N, Cin=K, seed=1400, act=SILU, R=True)
    refs = {}
    first = on_kb(lib, hooks, "repeat 0", cus, refs, uw=uw, order=XCD, grid=64, **kw)
    for i in range(1, 5):
        same_bits(first, on_kb(lib, hooks, f"repeat {i}", cus, refs, uw=uw, order=XCD, grid=64, **kw), f"repeat {i}")


# =====================================================================================================
# the forms the dispatcher picks by itself
# =====================================================================================================
def picked(name, cus):
    """(M, N, K, UW, xmap it should have on a device whose 3 CUs / 8 workgroups per XCD divide into NCG = 8) by the width rule of
    launch_rtlin_kb -- halve UW while tiles * N / (64 UW) < 3 CUs -- at N = 2048, K = 512 (fc1): tiles >= 3 CUs / 16 for UW = 2,
    >= 3 CUs / 8 for UW = 4, and xmap from U = 8 tiles >= 2 G = 6 CUs.  On 256 CUs: 340, 2256 / 2257, 4560 / 4561 and 9169 rows.
    The first is the smallest tile count an unforced launch takes at all (tiles * N / 64 >= 256 units)."""
    N, K = 2048, 512
    t_min, t2, t4, tx = cdiv(KB_MIN_UNITS, N // 64), cdiv(3 * cus, N // 128), cdiv(3 * cus, N // 256), cdiv(6 * cus, N // 256)
    assert t_min < t2 < t4 < tx
    if name == "fc2-uw2":      # N = 512, K = 2048: UW = 2 from 3 CUs / 4 tiles up to 3 CUs / 2 (9169 .. 18384 rows on 256 CUs)
        tiles = cdiv(3 * cus, 4) + 8
        assert tiles < cdiv(3 * cus, 2)
        return tiles * BM, 512, 2048, 2, 0
    M, uw, xmap = {"uw1": (BM * (t_min - 1) + 4, 1, 0), "uw1-last": (BM * (t2 - 1), 1, 0), "uw2-first": (BM * (t2 - 1) + 1, 2, 0),
                   "uw2-last": (BM * (t4 - 1), 2, 0), "uw4-first": (BM * (t4 - 1) + 1, 4, 0), "xmap-first": (BM * (tx - 1) + 1, 4, 1)}[name]
    return M, N, K, uw, xmap


def float64_rows(M, N, K, seed):
    """None (every row) where M N K <= 2e9; else the first and last 96 rows plus 32 whole 48-row tiles, four of every residue mod 8
    (the XCD index of a tile under xmap), drawn with a fixed seed: at least 1536 rows."""
    if M * N * K <= 2e9:
        return None
    tiles, g = cdiv(M, BM), torch.Generator().manual_seed(seed)
    mid = torch.arange(2, tiles - 2)
    rows = set(range(96)) | set(range(M - 96, M))
    for r in range(8):
        c = mid[mid % 8 == r]
        assert c.numel() >= 4
        for t in c[torch.randperm(c.numel(), generator=g)[:4]].tolist():
            rows |= set(range(t * BM, (t + 1) * BM))
    rows = torch.tensor(sorted(rows), dtype=torch.long)
    assert rows.numel() >= 1536 and {int(t) % 8 for t in rows // BM} == set(range(8))
    return rows


PICKED = ["uw1", "uw1-last", "uw2-first", "uw2-last", "uw4-first", "xmap-first", "fc2-uw2"]


@pytest.mark.parametrize("name", PICKED)
def test_form_the_dispatcher_picks(lib, hooks, cus, name):
    """Nothing forced.  The bit oracle covers every element of every launch; the float64 one every row or the seeded sample."""
    M, N, K, uw, xmap = picked(name, cus)
    form = kb_form(M, N, cus)
    assert form[0] == uw and (form[3] == xmap or cus % 64 != 0) and cdiv(M, BM) * (N // 64) >= KB_MIN_UNITS
    rows = float64_rows(M, N, K, seed=1500)
    plain = K == 2048
    kw = dict(M=M, N=N, Cin=K, seed=1500, bias=not plain, act=NONE if plain else RELU, rows=rows)
    refs, what = {}, f"{name} ({M}, {N}, {K}) on {cus} CUs, float64 on {'every row' if rows is None else f'{rows.numel()} rows'}"
    got = on_kb(lib, hooks, what, cus, refs, **kw)
    same_bits(got, on_tiles(lib, hooks, what, refs, **kw), what)
    if plain:
        chain_quality(got, refs, M, N, rows, what)


def test_the_dispatcher_reaches_every_form(cus):
    """With nothing forced the cases above land on UW = 1, 2 and 4 and on both orders (each asserts what ss_debug_rtlin_kb_last says)."""
    forms = [kb_form(*picked(name, cus)[:2], cus) for name in PICKED]
    assert {f[0] for f in forms} == {1, 2, 4}
    assert {f[3] for f in forms} == ({0, 1} if cus % 64 == 0 else {0})


# =====================================================================================================
# not this kernel
# =====================================================================================================
@pytest.mark.parametrize("what,kw", [("N = 320", dict(N=320, Cin=512)), ("N = 1005", dict(N=1005, Cin=512)), ("K = 320", dict(N=512, Cin=320)),
                                      ("glu", dict(N=512, Cin=512, glu=1))], ids=["N320", "N1005", "K320", "glu"])
def test_shapes_the_kernel_does_not_take(lib, hooks, what, kw):
    """Under canon = 1 with a forced grid (every rtlin_kb_shape_ok launch would go to the kernel): N % 256 != 0, K % 256 != 0 and GLU
    stay on the tiles."""
    hooks(5, 1)
    before = last_form(lib)
    w = Worst("rt_linear_kb's bit oracle: conv_gemm BLK tiles")
    launch(lib, canon_tile(100, kw["N"], kw["Cin"], kw.get("glu", 0)), f"(100, {kw['N']}, {kw['Cin']}) {what}", w, M=100, canon=1, seed=1600,
           **kw)
    w.done()
    assert last_form(lib) == before


def test_layernorm_prologue_at_k_512_is_refused(lib, hooks):
    hooks(5, 1)
    launch(lib, None, "(100, 512, 512) with ln_g under canon=1", Worst("refusals"), M=100, N=512, Cin=512, ln=True, entry="lin", canon=1,
           expect_rc=SS_ERR_ARG)
