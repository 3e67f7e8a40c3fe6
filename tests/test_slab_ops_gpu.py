"""Op-level tests of the packed-batch slab convs and the fused ResBlock against tests/slab_ref.py (float64, every utterance convolved
alone): conv_slab / conv_pair (csrc/conv_slab.hip), resblock_fused (csrc/resblock.hip), conv_c16 / c32 / c64 and the Winograd forms
conv_c64w / c32w / c128w / c256w (csrc/conv_c64w.hip), all through ss_op_conv_gemm_ex / ss_op_conv_pair / ss_op_resblock_fused.

What every case has in common:
  * a ragged pack: contiguous utterances of 1, 2, d - 1, d, d + 1, BM - 1, BM, BM + 1 and 2 BM + 3 rows plus a long one (BM: the
    kernel's block height, d: the dilation), a few thousand rows in all -- zero padding at every utterance edge, blocks that end on an
    edge, utterances shorter than the halo / the Winograd pair distance, at dilation 1 an utterance of no rows;
  * the input buffers carry rows of 1e4 on either side of the pack, so a halo row read from outside it is no small error;
  * outputs start as NaN and have a guard block of NaN rows behind the pack that must still be NaN afterwards;
  * two runs, at the default grid and at ss_debug_slab(3, 0) -- three workgroups that each walk many blocks across utterance edges
    (conv_c256w: its minimum of 16 workgroups, on a pack of 8200 rows) -- which must agree bit for bit.
"""
import ctypes as C

import pytest
import torch

from tests import slab_ref as R

pytestmark = pytest.mark.gpu

TOL = 2e-4                     # the per-conv bound of tests/test_ops_gpu.py (O(1)-scaled data, exact FP32 accumulation)
DEV = "cuda:0"
EDGE = 1.0e4                   # what the rows next to the pack hold in every input buffer
SS_ERR_ARG = 2
KD = [(3, 1), (3, 5), (7, 3), (11, 1), (11, 5)]


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


def census(lib):
    """Launches so far of every profiler class, by name."""
    out = {}
    for c in range(lib.ss_prof_num_classes()):
        n = C.c_int64()
        lib.ss_prof_totals(c, None, None, C.byref(n))
        out[lib.ss_prof_class_name(c).decode()] = n.value
    return out


def launches(lib, name):
    return census(lib)[name]


def took_since(lib, before):
    """{class: launches} of every class that launched since `before` (a census)."""
    now = census(lib)
    return {c: now[c] - before[c] for c in now if now[c] != before[c]}


def restore(lib):
    """Every hook these tests touch, back at its default."""
    lib.ss_debug_slab(0, -1)
    lib.ss_debug_force_tile(0, 0, 0)
    lib.ss_debug_conv_c16(1)
    for v in (1, 5):
        lib.ss_debug_conv_c32(v)
    for v in (1, 5, 7, 9):
        lib.ss_debug_conv_c64(v)


class Rows:
    """An input tensor [M, cols] on the device between two guard blocks of EDGE rows; ptr = its first row."""

    def __init__(self, t, guard):
        M, cols = t.shape
        self.buf = torch.full((M + 2 * guard, cols), EDGE, device=DEV)
        self.buf[guard:guard + M] = t.to(DEV)
        self.ptr = C.c_void_p(self.buf.data_ptr() + guard * cols * 4)


def out_buf(M, guard, ld):
    return torch.full((M + guard, ld), float("nan"), device=DEV)


def seg_dev(segs):
    return torch.tensor([[s, n, s, n] for s, n in segs], dtype=torch.int32, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def pack_lens(bm, d, min_rows=0, extra=()):
    """The utterance lengths of a test pack (see the module docstring); the long utterance grows until the pack has min_rows."""
    lens = [3 * bm + 77, 1, bm, 2, bm - 1, d - 1, bm + 1, d, 2 * bm + 3, d + 1] + list(extra) + [1]
    lens[0] += max(0, min_rows - sum(lens))             # (d = 1: the d - 1 entry is an utterance of no rows, which gets no block)
    return lens


# ---- the per-conv kernels ------------------------------------------------------------------------
WBM = {1: 256, 3: 252, 5: 240}          # Winograd block heights (whole pairs)
# route -> channels, profiler class (None: the generic tile kernel), hooks that send the launch there, block height, takes a twin,
# smallest pack (conv_slab: 2048 rows, the dispatch's own bound), (taps, dil) it takes
ROUTES = {
    "conv_slab32": dict(C=32, cls="conv_slab<32>", hooks=[("ss_debug_conv_c32", 0)], bm=lambda k, d: 128, twin=True, min_rows=2100),
    "conv_slab16": dict(C=16, cls="conv_slab<16>", hooks=[("ss_debug_conv_c16", 0)], bm=lambda k, d: 128, twin=True, min_rows=2100),
    "conv_c16": dict(C=16, cls="conv_c16<256,16>", hooks=[], bm=lambda k, d: 256, twin=True),
    "conv_c32": dict(C=32, cls="conv_c32<256,32>", hooks=[("ss_debug_conv_c32", 4)], bm=lambda k, d: 256, twin=True),
    "conv_c32w": dict(C=32, cls="conv_c32w<256,32>", hooks=[("ss_debug_conv_c32", 5)], bm=lambda k, d: WBM[d], twin=False),
    # conv_c64: 64 x WM rows -- 256, or 192 where two 256-row slabs do not fit a CU's LDS (k = 11 at dilation 5)
    "conv_c64": dict(C=64, cls="conv_c64<256,64>", hooks=[("ss_debug_conv_c64", 4)], bm=lambda k, d: 192 if (k, d) == (11, 5) else 256,
                     twin=True),
    "conv_c64w": dict(C=64, cls="conv_c64w<256,64>", hooks=[("ss_debug_conv_c64", 5)], bm=lambda k, d: WBM[d], twin=False,
                      kd=[(3, 1), (3, 5), (7, 3), (11, 1)]),          # k = 11 at dilation 5 stays on conv_c64 (LDS)
    "conv_c128w": dict(C=128, cls="conv_c128w<256,128>", hooks=[("ss_debug_conv_c64", 7)], bm=lambda k, d: WBM[d], twin=True),
    # conv_c256w never runs fewer than 16 workgroups (8 blocks x 2 column halves at a time): a pack of ~8k rows (~45 blocks) so that the
    # capped grid still walks 5-6 blocks per workgroup
    "conv_c256w": dict(C=256, cls="conv_c256w<256,128>", hooks=[("ss_debug_conv_c64", 9)], bm=lambda k, d: WBM[d], twin=True,
                       min_rows=8200),
    # the generic tile kernel with a segment table: where a ragged launch goes when no slab kernel takes it
    "tile32": dict(C=32, cls=None, hooks=[("ss_debug_force_tile", 2, 0, 0)], bm=lambda k, d: 128, twin=True, kd=[(3, 5), (11, 1)]),
    "tile64": dict(C=64, cls=None, hooks=[("ss_debug_force_tile", 2, 0, 0)], bm=lambda k, d: 32, twin=True, kd=[(7, 3), (11, 5)]),
}
CONV_CASES = [(name, k, d) for name, r in ROUTES.items() for (k, d) in r.get("kd", KD)]


class ConvPack:
    """Inputs of one conv over one pack, on the host (float32 + what the float64 reference needs) and on the device: x [M, Cc],
    w [N, Cc, k] (N = Cc unless given; every output-side leading dimension is N).

    `on` picks the epilogue: True -- every option; False -- the plain conv; "up" -- what the vocoder's upsamplers issue on a
    pre-activated input (no input activation, bias, the twin at slope 0.1, nothing else).
    `grid`: the (bm, bn) of an ss_debug_force_tile route whose third argument is the workgroup count (the stream-K kernels,
    tests/test_sk_ops_gpu.py); run(grid=G) then sets the hook to (bm, bn, G) before the launch.  The caller restores it."""

    def __init__(self, Cc, k, d, lens, guard, seed=0, N=None, grid=None):
        from streamspeech_amd.weights import conv_tap_major
        self.C, self.k, self.d, self.guard = Cc, k, d, guard
        self.N = N = Cc if N is None else N
        self.grid = grid
        self.segs = R.seg_table(lens)
        self.M = M = sum(lens)
        self.x, self.w = rnd(M, Cc, seed=seed + 1), rnd(N, Cc, k, seed=seed + 2, scale=(Cc * k) ** -0.5)
        self.b, self.R, self.R2 = rnd(N, seed=seed + 3, scale=0.1), rnd(M, N, seed=seed + 4), rnd(M, N, seed=seed + 5)
        self.dx, self.dR, self.dR2 = Rows(self.x, guard), Rows(self.R, guard), Rows(self.R2, guard)
        self.dw, self.db = conv_tap_major(self.w).to(DEV), self.b.to(DEV)
        self.dsegs = seg_dev(self.segs)

    def args(self, on, twin, out, out2, segmented=True):
        from streamspeech_amd.lib import SSOpConvArgs
        Cc, k, d = self.C, self.k, self.d
        a = SSOpConvArgs()
        a.A, a.W, a.C = self.dx.ptr, P(self.dw), P(out)
        a.lda = Cc
        a.ldc = a.ldr = a.ldr2 = a.ldc2 = self.N
        a.M = a.in_len = self.M
        a.N, a.Cin = self.N, Cc
        a.taps, a.dil, a.stride, a.pad = k, d, 1, d * (k - 1) // 2
        a.in_slope, a.act_slope, a.alpha, a.c2_slope = 0.1, 0.1, 1.0, 0.1
        a.same_rows = 1
        if segmented:
            a.segs, a.nseg, a.max_seg_out = P(self.dsegs), len(self.segs), max(n for _, n in self.segs)
        if on == "up":
            a.bias = P(self.db)
            if twin:
                a.C2 = P(out2)
        elif on:     # every option: input leaky-ReLU, bias, epilogue leaky-ReLU with its own slope, alpha, R, R2, the mean, the twin
            a.bias, a.R, a.R2 = P(self.db), self.dR.ptr, self.dR2.ptr
            a.in_act, a.act, a.act_slope, a.alpha, a.div = 3, 3, 0.2, 0.5, 3.0
            if twin:
                a.C2, a.c2_slope = P(out2), 0.3
        return a

    def ref(self, on, twin):
        x, w = self.x.double(), self.w.double()
        if not on:
            return R.conv(x, w, self.segs, self.d), None
        if on == "up":
            got = R.conv(x, w, self.segs, self.d, bias=self.b.double(), c2_slope=0.1)
        else:
            got = R.conv(x, w, self.segs, self.d, in_slope=0.1, bias=self.b.double(), act_slope=0.2, alpha=0.5, R=self.R.double(),
                         R2=self.R2.double(), div=3.0, c2_slope=0.3)
        return got if twin else (got[0], None)

    def run(self, lib, on, twin, segmented=True, grid=None):
        out, out2 = out_buf(self.M, self.guard, self.N), out_buf(self.M, self.guard, self.N)
        a = self.args(on, twin, out, out2, segmented)
        if self.grid is not None:
            assert lib.ss_debug_force_tile(self.grid[0], self.grid[1], grid or 0) == 0
        rc = lib.ss_op_conv_gemm_ex(S(), C.byref(a))
        torch.cuda.synchronize()
        return rc, out.cpu(), out2.cpu()


def check_conv(lib, name, k, d, lens, expect_cls=True):
    """Both epilogue settings of one (route, taps, dilation, pack): class, float64 error, twin, guard rows, grid-3 bits."""
    r = ROUTES[name]
    p = ConvPack(r["C"], k, d, lens, guard=r["bm"](k, d))
    M = p.M
    try:
        for hook in r["hooks"]:
            assert getattr(lib, hook[0])(*hook[1:]) == 0
        for on in (True, False):
            twin = r["twin"] and on
            ref, ref2 = p.ref(on, twin)
            runs = []
            for grid in (0, 3):
                assert lib.ss_debug_slab(grid, 0) == 0
                before = census(lib)
                rc, out, out2 = p.run(lib, on, twin)
                assert rc == 0, f"{name} on={on} grid={grid}: rc {rc}"
                took = took_since(lib, before)                  # over EVERY class: stream-K or any other taker shows up here
                if expect_cls and r["cls"]:
                    assert took == {r["cls"]: 1}, f"{name} on={on} grid={grid}: launches by class {took}"
                else:                                           # the generic LDS-tiled kernel, whichever tile: one launch, nothing else
                    assert len(took) == 1 and list(took.values()) == [1] and next(iter(took)).startswith("conv_gemm<"), \
                        f"{name} on={on} grid={grid}: launches by class {took}"
                runs.append((out, out2))
            out, out2 = runs[0]
            err = (out[:M].double() - ref).abs().max().item()
            print(f"{name} k={k} d={d} on={on} M={M} nseg={len(lens)}: max abs err {err:.3e}")
            assert torch.isfinite(out[:M]).all() and err < TOL, f"{name} on={on}: max abs err {err}"
            assert torch.isnan(out[M:]).all(), "rows behind the pack were written"
            if twin:
                assert torch.equal(out2[:M], torch.where(out[:M] > 0, out[:M], out[:M] * 0.3)), "twin != leaky_relu(C, c2_slope)"
                assert (out2[:M].double() - ref2).abs().max() < TOL
                assert torch.isnan(out2[M:]).all()
            else:
                assert torch.isnan(out2).all(), "an unbound twin was written"
            assert torch.equal(bits(runs[0][0]), bits(runs[1][0])), f"{name} on={on}: three workgroups give other bits"
            assert torch.equal(bits(runs[0][1]), bits(runs[1][1]))
    finally:
        restore(lib)


@pytest.mark.parametrize("name,k,d", CONV_CASES, ids=[f"{n}-k{k}-d{d}" for n, k, d in CONV_CASES])
def test_conv_ragged_pack(lib, name, k, d):
    r = ROUTES[name]
    check_conv(lib, name, k, d, pack_lens(r["bm"](k, d), d, r.get("min_rows", 0)))


SHORT_256 = [1 + (7 * i) % 16 for i in range(256)]      # 256 utterances of 1..16 rows, 2176 rows in all


@pytest.mark.parametrize("name", list(ROUTES))
def test_conv_256_short_utterances(lib, name):
    """The largest segment table the slab kernels take: every block is a partial one, every utterance shorter than the k = 7 halo."""
    k, d = (7, 3) if (7, 3) in ROUTES[name].get("kd", KD) else (11, 1)
    check_conv(lib, name, k, d, SHORT_256)


@pytest.mark.parametrize("name", [n for n, r in ROUTES.items() if r["cls"]])
def test_conv_257_utterances_go_to_the_tile_kernel(lib, name):
    """One utterance more than the slab kernels' block table holds (nseg <= 256 in every *_eligible): launch_conv_gemm falls through to
    the generic tile kernel (one grid plane per utterance), same result."""
    k, d = (7, 3) if (7, 3) in ROUTES[name].get("kd", KD) else (11, 1)
    check_conv(lib, name, k, d, SHORT_256 + [9], expect_cls=False)


@pytest.mark.parametrize("name", [n for n, r in ROUTES.items() if r["cls"]])
def test_conv_rows_do_not_depend_on_the_pack(lib, name):
    """One utterance's rows, bit for bit: alone (no segment table), as a single segment, and at positions 0, 5 and 15 of a 16-utterance
    pack (blocks are numbered per utterance, so its rows sit at the same block positions everywhere).  The slab kernels only: the
    generic tile kernel picks its split-K from the tile count of the launch (launch_cfg_ks), so its bits depend on the pack by design --
    the pack-invariant tile form is the CANON_SEQ route of tests/test_pack_invariance_gpu.py."""
    r = ROUTES[name]
    k, d = (7, 3) if (7, 3) in r.get("kd", KD) else (11, 1)
    bm = r["bm"](k, d)
    L = max(2 * bm + 37, r.get("min_rows", 0))
    others = [1 + (37 * i) % 211 for i in range(15)]
    utt = rnd(L, r["C"], seed=77)
    utt_R, utt_R2 = rnd(L, r["C"], seed=78), rnd(L, r["C"], seed=79)
    got = {}
    try:
        for hook in r["hooks"]:
            assert getattr(lib, hook[0])(*hook[1:]) == 0
        assert lib.ss_debug_slab(0, 0) == 0
        for label, lens, pos in [("alone", [L], 0), ("one segment", [L], 0), ("pos 0", [L] + others, 0),
                                 ("pos 5", others[:5] + [L] + others[5:], 5), ("pos 15", others + [L], 15)]:
            p = ConvPack(r["C"], k, d, lens, guard=bm, seed=100 + pos)        # other neighbours every time, the same weights below
            s0 = p.segs[pos][0]
            for src, dst in ((utt, p.dx), (utt_R, p.dR), (utt_R2, p.dR2)):
                dst.buf[bm + s0: bm + s0 + L] = src.to(DEV)
            p.dw.copy_(got.setdefault("w", p.dw))
            p.db.copy_(got.setdefault("b", p.db))
            n0 = launches(lib, r["cls"])
            rc, out, out2 = p.run(lib, True, r["twin"], segmented=label != "alone")
            assert rc == 0 and launches(lib, r["cls"]) == n0 + 1, label
            got[label] = (out[s0:s0 + L], out2[s0:s0 + L])
            assert torch.isfinite(got[label][0]).all()
    finally:
        restore(lib)
    for label in ("one segment", "pos 0", "pos 5", "pos 15"):
        assert torch.equal(bits(got[label][0]), bits(got["alone"][0])), f"{name}: {label} differs from the utterance alone"
        assert torch.equal(bits(got[label][1]), bits(got["alone"][1]))


# ---- conv_pair -----------------------------------------------------------------------------------
class ChainPack:
    """Inputs of a conv pair / a ResBlock (three pairs) over one pack."""

    def __init__(self, Cc, k, lens, guard, seed=0):
        from streamspeech_amd.weights import conv_tap_major
        self.C, self.k, self.guard = Cc, k, guard
        self.segs = R.seg_table(lens)
        self.M = M = sum(lens)
        self.x, self.R2 = rnd(M, Cc, seed=seed + 1), rnd(M, Cc, seed=seed + 2)
        self.W1 = [rnd(Cc, Cc, k, seed=seed + 3 + i, scale=(Cc * k) ** -0.5) for i in range(3)]
        self.W2 = [rnd(Cc, Cc, k, seed=seed + 6 + i, scale=(Cc * k) ** -0.5) for i in range(3)]
        self.B1 = [rnd(Cc, seed=seed + 9 + i, scale=0.1) for i in range(3)]
        self.B2 = [rnd(Cc, seed=seed + 12 + i, scale=0.1) for i in range(3)]
        self.dx, self.dR2 = Rows(self.x, guard), Rows(self.R2, guard)
        self.dW1, self.dW2 = [conv_tap_major(w).to(DEV) for w in self.W1], [conv_tap_major(w).to(DEV) for w in self.W2]
        self.dB1, self.dB2 = [b.to(DEV) for b in self.B1], [b.to(DEV) for b in self.B2]
        self.dsegs = seg_dev(self.segs)

    def cast(self, dtype):
        f = lambda ts: [t.to(dtype) for t in ts]
        return self.x.to(dtype), f(self.W1), f(self.B1), f(self.W2), f(self.B2), self.R2.to(dtype)

    def slab_conv(self, lib, src_ptr, dw, db, d, out, Rptr=None, R2ptr=None, div=0.0):
        """One conv of the multi-launch form on conv_slab: leaky-ReLU(0.1) input, bias, [+ R] [R2 +] [/ div]."""
        from streamspeech_amd.lib import SSOpConvArgs
        a = SSOpConvArgs()
        a.A, a.W, a.bias, a.C, a.R, a.R2 = src_ptr, P(dw), P(db), P(out), Rptr, R2ptr
        a.lda = a.ldc = a.ldr = a.ldr2 = a.ldc2 = self.C
        a.M = a.in_len = self.M
        a.N = a.Cin = self.C
        a.taps, a.dil, a.stride, a.pad = self.k, d, 1, d * (self.k - 1) // 2
        a.in_act, a.in_slope, a.act_slope, a.alpha, a.c2_slope, a.div = 3, 0.1, 0.1, 1.0, 0.1, div
        a.same_rows = 1
        a.segs, a.nseg, a.max_seg_out = P(self.dsegs), len(self.segs), max(n for _, n in self.segs)
        cls = f"conv_slab<{self.C}>"
        n0 = launches(lib, cls)
        assert lib.ss_op_conv_gemm_ex(S(), C.byref(a)) == 0 and launches(lib, cls) == n0 + 1, "the composition must run on conv_slab"

    def slab_pair(self, lib, src_ptr, i, d, out, R2ptr=None, div=0.0):
        """Pair i as two conv_slab launches: out = conv2(lrelu(conv1_d(lrelu(src)) + b1)) + b2 + src [+ R2] [/ div]."""
        mid = out_buf(self.M, self.guard, self.C)
        self.slab_conv(lib, src_ptr, self.dW1[i], self.dB1[i], d, mid)
        self.slab_conv(lib, P(mid), self.dW2[i], self.dB2[i], 1, out, Rptr=src_ptr, R2ptr=R2ptr, div=div)


def slab_route(lib, Cc):
    """The narrow stages' per-conv kernels off: the launches of ChainPack.slab_conv land on conv_slab."""
    assert (lib.ss_debug_conv_c32(0) if Cc == 32 else lib.ss_debug_conv_c16(0)) == 0


# conv_pair_eligible: both weight matrices, the input slab and the 144-row mid slab in 72 KB of LDS -- every k at 16 channels, k = 3 only
# at 32 (k = 7: 102 KB, k = 11: 150 KB); (taps - 1) dil <= 50
PAIR_CASES = [(16, 3, 1), (16, 3, 5), (16, 7, 3), (16, 11, 1), (16, 11, 5), (32, 3, 1), (32, 3, 5)]


def chain_bound(ref64, f32, what):
    """What a float32 chain may be off by: 4 x the max abs error of a float32 torch CPU evaluation of the same chain on the same inputs
    (both are float32 chains of the same length; the factor covers summation order only)."""
    e = (f32.double() - ref64).abs()
    e = e[torch.isfinite(e)].max().item()
    print(f"{what}: float32 torch chain vs float64 {e:.3e} -> bound {4 * e:.3e}")
    return 4 * e


def check_pair(lib, Cc, k, d, lens):
    """conv_pair on one pack, with R2 / the mean / the twin and without: class, float64 bound, guard rows, twin, grid-3 bits, and bit for
    bit its two launches on conv_slab."""
    p = ChainPack(Cc, k, lens, guard=128)
    M, cls = p.M, f"conv_slab<{Cc}>"
    x, W1, B1, W2, B2, R2 = p.cast(torch.float64)
    xf, W1f, B1f, W2f, B2f, R2f = p.cast(torch.float32)
    try:
        for on in (True, False):
            ref = R.pair(x, p.segs, W1[0], B1[0], W2[0], B2[0], d, 0.1, R2 if on else None, 3.0 if on else 0.0)
            bound = chain_bound(ref, R.pair(xf, p.segs, W1f[0], B1f[0], W2f[0], B2f[0], d, 0.1, R2f if on else None,
                                            3.0 if on else 0.0), f"conv_pair C={Cc} k={k} d={d} on={on}")
            runs = []
            for grid in (0, 3):
                assert lib.ss_debug_slab(grid, 0) == 0
                out, out2 = out_buf(M, 128, Cc), out_buf(M, 128, Cc)
                n0 = launches(lib, cls)
                rc = lib.ss_op_conv_pair(S(), p.dx.ptr, Cc, P(p.dW1[0]), P(p.dB1[0]), P(p.dW2[0]), P(p.dB2[0]), P(out), Cc,
                                         p.dR2.ptr if on else None, Cc, 3.0 if on else 0.0, P(out2) if on else None, Cc, 0.3, Cc, k, d,
                                         M, M, 0.1, P(p.dsegs), len(p.segs))
                torch.cuda.synchronize()
                assert rc == 0 and launches(lib, cls) == n0 + 1
                runs.append((out.cpu(), out2.cpu()))
            out, out2 = runs[0]
            err = (out[:M].double() - ref).abs().max().item()
            print(f"conv_pair C={Cc} k={k} d={d} on={on} M={M} nseg={len(lens)}: max abs err {err:.3e}")
            assert torch.isfinite(out[:M]).all() and err < bound, f"max abs err {err} (bound {bound})"
            assert torch.isnan(out[M:]).all()
            if on:
                assert torch.equal(out2[:M], torch.where(out[:M] > 0, out[:M], out[:M] * 0.3)) and torch.isnan(out2[M:]).all()
            else:
                assert torch.isnan(out2).all()
            assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
            # the two-launch form (the kernel claims the same bits: same tap / channel order inside each conv)
            lib.ss_debug_slab(0, -1)
            slab_route(lib, Cc)
            two = out_buf(M, 128, Cc)
            p.slab_pair(lib, p.dx.ptr, 0, d, two, p.dR2.ptr if on else None, 3.0 if on else 0.0)
            torch.cuda.synchronize()
            assert torch.equal(bits(two.cpu()), bits(out)), "conv_pair != its two conv_slab launches"
            restore(lib)
    finally:
        restore(lib)


@pytest.mark.parametrize("Cc,k,d", PAIR_CASES)
def test_conv_pair(lib, Cc, k, d):
    """conv_pair on the ragged pack of the module docstring (BM = 128)."""
    check_pair(lib, Cc, k, d, pack_lens(128, d, 2100))


@pytest.mark.parametrize("Cc,k,d", [(16, 3, 1), (16, 7, 3), (16, 11, 5), (32, 3, 5)])
def test_conv_pair_256_short_utterances(lib, Cc, k, d):
    """The largest block table conv_pair takes (it sits behind both weight matrices and both slabs in LDS): 256 utterances of 1..16 rows,
    every block a partial one, every utterance shorter than the pair's halo at k >= 7."""
    check_pair(lib, Cc, k, d, SHORT_256)


def test_conv_pair_refusals(lib):
    """What launch_conv_pair does not take comes back as SS_ERR_ARG with the output untouched."""
    Cc, M = 16, 2304
    x = torch.zeros(M + 128, Cc, device=DEV)
    w, b = torch.zeros(Cc, 11 * Cc, device=DEV), torch.zeros(Cc, device=DEV)
    out = out_buf(M, 128, Cc)
    segs = seg_dev(R.seg_table([9] * 256 + [0]))       # a table of 257 entries for the nseg = 257 call

    def call(A=x, Cout=out, C_=Cc, k=3, d=1, rows=M, nseg=0):
        return lib.ss_op_conv_pair(S(), P(A), C_, P(w), P(b), P(w), P(b), P(Cout), C_, None, C_, 0.0, None, C_, 0.1, C_, k, d, rows, rows,
                                   0.1, P(segs) if nseg else None, nseg)
    try:
        assert call(Cout=x) == SS_ERR_ARG                       # A == C: neighbouring blocks read A's halo
        assert call(k=4) == SS_ERR_ARG                          # even taps
        assert call(k=11, d=6) == SS_ERR_ARG                    # (taps - 1) dil = 60 > 50
        assert call(rows=2047) == SS_ERR_ARG                    # below its 2048 rows
        assert call(nseg=257) == SS_ERR_ARG
        assert call(C_=32, k=7) == SS_ERR_ARG and call(C_=32, k=11) == SS_ERR_ARG     # 32 channels: only k = 3 fits the LDS
        assert call(C_=64) == SS_ERR_ARG
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and not x.any()
        assert call() == 0                                      # (the same call without a fault is taken)
        torch.cuda.synchronize()
        assert torch.isfinite(out[:M]).all() and torch.isnan(out[M:]).all()
    finally:
        restore(lib)


# ---- resblock_fused ------------------------------------------------------------------------------
def rb_geom(Cc, k, dils):
    """RbGeom of csrc/resblock.hip: slab rows RX, halo H, block height BM = RX - 2 H, tiles per slot TSTRIDE, slots per wave."""
    ntile = (23 if k >= 11 else 24) if Cc == 32 else 40
    ts = 4 if Cc == 32 else 8
    H = (k - 1) // 2 * (sum(dils) + 3)
    return dict(RX=16 * ntile, H=H, BM=16 * ntile - 2 * H, TS=ts, SLOTS=(ntile + ts - 1) // ts)


def rb_slot_lens(Cc, k, dils):
    """Utterance lengths that end the LAST block's in-utterance rows inside chosen tile slots of a wave.  Slab row rho of a block is
    packed row m0 - H + rho, tile rho // 16, slot tile // TSTRIDE (a wave owns tile tw + TSTRIDE s in slot s); a last block with Lr
    rows left has its in-utterance rows end at slab row e = H + Lr.
      first slot:  e = 16 TSTRIDE (the last row of slot 0)            -> Lr = 16 TSTRIDE - H    (H <= 64 <= 16 TSTRIDE)
      middle slot: e = 16 TSTRIDE (SLOTS // 2) + 8 TSTRIDE            -> Lr = e - H
      last slot:   e = 16 TSTRIDE (SLOTS - 1) + 1 where an output row gets there (e <= RX - H), else the highest it gets, Lr = BM - 1
    The first two come as BM + Lr (the last block follows a full one), the third as Lr alone (the first block is the last)."""
    g = rb_geom(Cc, k, dils)
    first = max(1, 16 * g["TS"] - g["H"])
    middle = 16 * g["TS"] * (g["SLOTS"] // 2) + 8 * g["TS"] - g["H"]
    last = 16 * g["TS"] * (g["SLOTS"] - 1) + 1 - g["H"]
    if not 0 < last <= g["BM"]:
        last = g["BM"] - 1
    assert 0 < first <= g["BM"] and 0 < middle <= g["BM"]
    return [g["BM"] + first, g["BM"] + middle, last]


def rb_launch(lib, p, dils, out, ldy, on, M=None, nseg=None, x_ptr=None, Cc=None, k=None):
    arr = lambda ts: (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    rc = lib.ss_op_resblock_fused(S(), x_ptr or p.dx.ptr, Cc or p.C, arr(p.dW1), arr(p.dB1), arr(p.dW2), arr(p.dB2),
                                  (C.c_int32 * 3)(*dils), P(out), ldy, p.dR2.ptr if on else None, p.C, 3.0 if on else 0.0,
                                  Cc or p.C, k or p.k, M or p.M, 0.1, P(p.dsegs), len(p.segs) if nseg is None else nseg)
    torch.cuda.synchronize()
    return rc


def rb_compose(lib, p, dils, on):
    """The multi-launch form on the direct-form kernels: six conv_slab launches."""
    slab_route(lib, p.C)
    cur, bufs = p.dx.ptr, []
    for i in range(3):
        out = out_buf(p.M, p.guard, p.C)
        last = i == 2
        p.slab_pair(lib, cur, i, dils[i], out, p.dR2.ptr if (on and last) else None, 3.0 if (on and last) else 0.0)
        bufs.append(out)
        cur = P(out)
    torch.cuda.synchronize()
    return bufs[-1].cpu()


RB_CASES = [(Cc, k, dils) for Cc in (32, 16) for k in (3, 7, 11) for dils in ((1, 3, 5), (1, 1, 1), (5, 3, 1))]


def check_resblock(lib, Cc, k, dils, lens):
    """The fused ResBlock on one pack against float64 (bound: 4 x a float32 torch chain's own error, see chain_bound) and bit for bit
    against the six conv_slab launches it replaces; ldy = C + 4 with untouched padding columns; R2 with the mean / neither; guard rows;
    grid-3 bits."""
    bm = rb_geom(Cc, k, dils)["BM"]
    p = ChainPack(Cc, k, lens, guard=bm, seed=40)
    M, cls, ldy = p.M, f"resblock_fused<{Cc}>", Cc + 4
    x, W1, B1, W2, B2, R2 = p.cast(torch.float64)
    xf, W1f, B1f, W2f, B2f, R2f = p.cast(torch.float32)
    try:
        for on in (True, False):
            ref = R.resblock(x, p.segs, W1, B1, W2, B2, dils, 0.1, R2 if on else None, 3.0 if on else 0.0)
            bound = chain_bound(ref, R.resblock(xf, p.segs, W1f, B1f, W2f, B2f, dils, 0.1, R2f if on else None, 3.0 if on else 0.0),
                                f"resblock_fused C={Cc} k={k} dil={dils} on={on}")
            runs = []
            for grid in (0, 3):
                assert lib.ss_debug_slab(grid, 0) == 0
                out = out_buf(M, bm, ldy)
                n0 = launches(lib, cls)
                assert rb_launch(lib, p, dils, out, ldy, on) == 0 and launches(lib, cls) == n0 + 1
                runs.append(out.cpu())
            out = runs[0]
            err = (out[:M, :Cc].double() - ref).abs().max().item()
            print(f"resblock_fused C={Cc} k={k} dil={dils} on={on} M={M} nseg={len(lens)} BM={bm}: max abs err {err:.3e}")
            assert torch.isfinite(out[:M, :Cc]).all() and err < bound, f"max abs err {err} (bound {bound})"
            assert torch.isnan(out[M:]).all(), "rows behind the pack were written"
            assert torch.isnan(out[:, Cc:]).all(), "the padding columns of Y were written"
            assert torch.equal(bits(runs[0]), bits(runs[1])), "three workgroups give other bits"
            lib.ss_debug_slab(0, -1)
            multi = rb_compose(lib, p, dils, on)
            restore(lib)
            assert torch.equal(bits(multi[:M]), bits(out[:M, :Cc])), "resblock_fused != its six conv_slab launches"
    finally:
        restore(lib)


@pytest.mark.parametrize("Cc,k,dils", RB_CASES, ids=[f"c{c}-k{k}-d{''.join(map(str, d))}" for c, k, d in RB_CASES])
def test_resblock_fused(lib, Cc, k, dils):
    """The ragged pack of the module docstring plus utterances of H - 1, H, H + 1 rows and the slot lengths of rb_slot_lens."""
    g = rb_geom(Cc, k, dils)
    check_resblock(lib, Cc, k, dils, pack_lens(g["BM"], max(dils), 2100, extra=[g["H"] - 1, g["H"], g["H"] + 1] + rb_slot_lens(Cc, k, dils)))


@pytest.mark.parametrize("Cc,k", [(Cc, k) for Cc in (32, 16) for k in (3, 7, 11)])
def test_resblock_256_short_utterances(lib, Cc, k):
    """The largest block table resblock_fused takes (RB_MAXSEG + 2 ints behind the bias table, the last bytes of its LDS), all six
    instantiations: 256 utterances of 1..16 rows -- every block a partial one whose in-utterance rows end in the first tile slot, every
    utterance shorter than H at k >= 7 (H = 36 / 60), around H at k = 3 (H = 12)."""
    check_resblock(lib, Cc, k, (1, 3, 5), SHORT_256)


@pytest.mark.parametrize("Cc,k", [(32, 11), (16, 7)])
def test_resblock_default_grid_walks_more_than_one_block(lib, Cc, k):
    """The real grid (one workgroup per CU), a pack just past 2 x CUs x BM rows: every workgroup fetches its next block's rows under the
    last conv of the current one.  Against float64, the six conv_slab launches and the three-workgroup walk."""
    dils = (1, 3, 5)
    bm = rb_geom(Cc, k, dils)["BM"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 2 * cus * bm + bm + 3
    lens = [rows // 2 + 11, 1, rows - rows // 2 - 12]
    p = ChainPack(Cc, k, lens, guard=bm, seed=60)
    M, cls = p.M, f"resblock_fused<{Cc}>"
    assert M > 2 * cus * bm
    x, W1, B1, W2, B2, R2 = p.cast(torch.float64)
    xf, W1f, B1f, W2f, B2f, R2f = p.cast(torch.float32)
    ref = R.resblock(x, p.segs, W1, B1, W2, B2, dils, 0.1, R2, 3.0)
    bound = chain_bound(ref, R.resblock(xf, p.segs, W1f, B1f, W2f, B2f, dils, 0.1, R2f, 3.0), f"resblock_fused C={Cc} k={k} big")
    try:
        runs = []
        for grid in (0, 3):
            assert lib.ss_debug_slab(grid, -1) == 0
            out = out_buf(M, bm, Cc)
            n0 = launches(lib, cls)
            assert rb_launch(lib, p, dils, out, Cc, True) == 0 and launches(lib, cls) == n0 + 1
            runs.append(out.cpu())
        out = runs[0]
        err = (out[:M].double() - ref).abs().max().item()
        print(f"resblock_fused C={Cc} k={k} M={M} (CUs {cus}, BM {bm}): max abs err {err:.3e}")
        assert torch.isfinite(out[:M]).all() and err < bound, f"max abs err {err} (bound {bound})"
        assert torch.isnan(out[M:]).all()
        assert torch.equal(bits(runs[0]), bits(runs[1]))
        lib.ss_debug_slab(0, -1)
        assert torch.equal(bits(rb_compose(lib, p, dils, True)), bits(out))
    finally:
        restore(lib)


def test_resblock_refusals(lib):
    """What launch_resblock_fused does not take: SS_ERR_ARG, the output stays all NaN."""
    lens = [700, 1, 1400]
    p = ChainPack(32, 11, lens, guard=16, seed=80)
    out = out_buf(p.M, 16, 32)
    many = seg_dev(R.seg_table([8] * 257))
    p64 = ChainPack(64, 3, [300], guard=16, seed=81)
    out64 = out_buf(300, 16, 64)
    try:
        assert rb_launch(lib, p, (1, 3, 6), out, 32, False) == SS_ERR_ARG          # H = 5 (1 + 3 + 6 + 3) = 65 > 64
        assert rb_launch(lib, p, (1, 3, 5), out, 32, False, x_ptr=P(out)) == SS_ERR_ARG     # X == Y
        assert rb_launch(lib, p, (0, 3, 5), out, 32, False) == SS_ERR_ARG
        assert rb_launch(lib, p, (1, 3, 5), out, 34, False) == SS_ERR_ARG          # ldy % 4
        assert rb_launch(lib, p, (1, 3, 5), out, 32, False, k=5) == SS_ERR_ARG
        p.dsegs = many
        assert rb_launch(lib, p, (1, 3, 5), out, 32, False, M=8 * 257, nseg=257) == SS_ERR_ARG
        assert rb_launch(lib, p64, (1, 3, 5), out64, 64, False) == SS_ERR_ARG       # C = 64
        assert torch.isnan(out).all() and torch.isnan(out64).all()
    finally:
        restore(lib)
