"""Op-level tests of the persistent stream-K convs conv_sk (csrc/conv_sk.hip) and conv_sk2 / conv_sk2_bf16x3 (csrc/conv_sk2.hip) on
RAGGED packs, against tests/slab_ref.py (float64, every utterance convolved alone) -- the segment code of the two kernels (the binary
search of a row's utterance, the s_lo / s_hi row bounds in LDS, conv_sk2 recomputing them only when the row tile of a part changes)
while workgroups start and stop in the middle of tiles.  Every launch goes through ss_op_conv_gemm_ex with a segment table; the route
is picked with ss_debug_force_tile(bm, bn, G).

The harness is that of tests/test_slab_ops_gpu.py: 1e4 guard rows around every input, NaN outputs with a NaN guard block behind the
pack, a census over every profiler class (one launch, of the stream-K class, nothing else).  On top of it:
  * rectangular convs (N != Cin: conv_pre, the polyphase upsamplers), both tile widths (N % 128 == 0 / == 64), one k-block per tap
    up to 88 k-steps, a halo of 25 rows (longer than most utterances), a segmented linear;
  * grids G = 0 (the launcher's choice), 1 (no split) and two small co-prime ones, so that parts begin and end inside tiles and
    inside utterances: two launches at one G agree bit for bit, across G only the bound holds (the split changes the summation order);
  * three epilogues: every option / plain / what the upsamplers issue on a pre-activated input (bias + twin at 0.1).
Bounds: the f32 routes TOL = 2e-4 (the per-conv bound of tests/test_ops_gpu.py and tests/test_slab_ops_gpu.py on this data scaling);
the split-bf16 route against the f32 conv_sk2 result of the same pack and grid with the bars of tests/test_bf16x3_gpu.py (relative RMS
in (0, 2e-5), max abs < 1e-3) and against float64 with max abs < 1e-3 -- and, the sharp one, against the float64 sum of the THREE
TERMS the kernel multiplies (tests/slab_ref.py conv_x3: hi = bf16(x), lo = bf16(x - hi), W_hi A_hi + W_hi A_lo + W_lo A_hi) with max abs
< 16 E_case (tests/rounded_cases.py, about 1e-5: float32 accumulation is all that is left), nearer to it than to the four-term sum
and to either two-term sum.
"""
import ctypes as C
import os

import pytest
import torch

from tests import rounded_cases as RC
from tests import slab_ref as R
from test_slab_ops_gpu import (SHORT_256, TOL, ConvPack, P, S, bits, census, lib, out_buf, pack_lens, restore, rnd,  # noqa: F401
                               stop_after_a_gpu_error, took_since)

pytestmark = pytest.mark.gpu

X3_TOL = 1e-3                  # split-bf16: max abs against the f32 kernel and against float64 (tests/test_bf16x3_gpu.py)
X3_REL = 2e-5                  # ... relative RMS against the f32 kernel, and not 0
GUARD = 256                    # guard rows of every buffer: the tallest block, ten times the longest halo

# route -> ss_debug_force_tile (bm, bn), profiler class, block height, k-steps every workgroup keeps (launch_sk: G <= U / 8,
# launch_sk2: G <= U / 4)
ROUTES = {
    "conv_sk": dict(hook=(1, 0), cls="conv_sk<128,BN,32>", bm=128, keep=8),
    "conv_sk_xcd": dict(hook=(1, 8), cls="conv_sk<128,BN,32>", bm=128, keep=8),
    "conv_sk2": dict(hook=(4, 0), cls="conv_sk2<256,128,32>", bm=256, keep=4),
    "conv_sk2_x3": dict(hook=(5, 0), cls="conv_sk2_bf16x3<256,128,32>", bm=256, keep=4),
}
# (Cin, N, taps, dil)
SHAPES = [(64, 64, 7, 3), (128, 128, 3, 1), (32, 192, 3, 1), (128, 512, 7, 1), (64, 320, 3, 1), (128, 256, 3, 1), (256, 256, 11, 5),
          (64, 128, 1, 1)]
SHORT_300 = [1 + (7 * i) % 16 for i in range(300)]      # more utterances than any slab kernel's block table holds
EPILOGUES = (True, False, "up")                         # ConvPack's `on`


def lens_of(pack, bm, d):
    if pack == "edges":        # 1, 2, d - 1, d, d + 1, bm - 1, bm, bm + 1, 2 bm + 3 rows and a long one (d = 1: one of no rows)
        return pack_lens(bm, d, 2600)
    return {"short256": SHORT_256, "short300": SHORT_300}[pack]


def grid_cap(route, shape, M):
    """The largest G the route's launcher keeps for this launch."""
    cin, n, k, _ = shape
    r = ROUTES[route]
    units = -(-M // r["bm"]) * (n // (128 if n % 128 == 0 else 64)) * k * (cin // 32)
    return units // r["keep"]


def grids_of(route, shape, M):
    cap = grid_cap(route, shape, M)
    pair = (3, 7) if cap >= 7 else (3, 5) if cap >= 5 else (2, 3)
    assert cap >= pair[1], f"{route} {shape} M={M}: the launcher would clamp G = {pair[1]} to {cap}"
    return (0, 1) + pair


_packs = {}


def pack_of(shape, lens, seed=0):
    """The pack of (shape, lens) with its float64 references per epilogue, shared by the routes (the two last ones are kept)."""
    key = (shape, tuple(lens), seed)
    if key not in _packs:
        while len(_packs) >= 2:
            del _packs[next(iter(_packs))]
        cin, n, k, d = shape
        p = ConvPack(cin, k, d, lens, guard=GUARD, seed=seed, N=n)
        _packs[key] = (p, {on: p.ref(on, on is not False) for on in EPILOGUES})
    return _packs[key]


_x3 = {}


def x3_of(shape, lens, seed=0):
    """The rounded-operand references of a pack's three epilogues (RC.x3_refs), for the split-bf16 route; the last two are kept."""
    key = (shape, tuple(lens), seed)
    if key not in _x3:
        while len(_x3) >= 2:
            del _x3[next(iter(_x3))]
        _x3[key] = RC.x3_refs(pack_of(shape, lens, seed)[0])
    return _x3[key]


def check_x3(p, out, out2, xr, twin, what):
    """Split-bf16 against the three-term float64 reference: max abs under 16 E (the twin too), and nearer to it than to the four-term
    sum (+ll) and the two-term sums (-hl, -lh) by a factor of two.  The figures are printed before anything is asserted."""
    M = p.M
    e3, near = RC.err(out[:M], xr.ref), RC.nearest(out, xr, M)
    print(f"{what} M={M}: vs three-term float64 {e3:.3e} E {xr.E:.3e} bar {xr.bar:.3e} to the mutants "
          + " ".join(f"[{n}: {dm:.3e}]" for n, (_, dm) in near.items()))
    assert e3 < xr.bar <= TOL, f"{what}: max abs against the three-term reference {e3} (bar {xr.bar})"
    if twin:
        assert RC.err(out2[:M], xr.ref2) < xr.bar, f"{what}: twin against the three-term reference"
    for n, (d0, dm) in near.items():
        assert d0 < 0.5 * dm, f"{what}: {d0} from the three-term reference, {dm} from '{n}'"


def launch(lib, p, route, G, on, twin, segmented=True):
    """One launch on the route at grid G: rc == 0, one launch of the route's class and nothing else, no stream-K time-out."""
    r = ROUTES[route]
    p.grid = r["hook"]
    errs, before = lib.ss_debug_sk_errors(), census(lib)
    rc, out, out2 = p.run(lib, on, twin, segmented=segmented, grid=G)
    what = f"{route} on={on} G={G}"
    assert rc == 0, f"{what}: rc {rc}"
    took = took_since(lib, before)
    assert took == {r["cls"]: 1}, f"{what}: launches by class {took}"
    assert lib.ss_debug_sk_errors() == errs, f"{what}: a stream-K bounded wait timed out / a ticket was out of range"
    return out, out2


def check_output(p, out, out2, ref, ref2, twin, slope, tol, what):
    """Finite over the pack, float64 bound, the twin (bitwise leaky-ReLU of C and within the bound), guard rows, unbound twin."""
    M = p.M
    assert torch.isfinite(out[:M]).all(), f"{what}: not finite over the pack"
    err = (out[:M].double() - ref).abs().max().item()
    assert err < tol, f"{what}: max abs err {err}"
    assert torch.isnan(out[M:]).all(), f"{what}: rows behind the pack were written"
    if twin:
        assert torch.equal(out2[:M], torch.where(out[:M] > 0, out[:M], out[:M] * slope)), f"{what}: twin != leaky_relu(C, c2_slope)"
        assert (out2[:M].double() - ref2).abs().max() < tol, f"{what}: twin"
        assert torch.isnan(out2[M:]).all(), f"{what}: twin rows behind the pack were written"
    else:
        assert torch.isnan(out2).all(), f"{what}: an unbound twin was written"
    return err


def check_sk(lib, route, shape, lens, pack, grids=None):
    """All three epilogues of one (route, shape, pack) at every grid."""
    p, refs = pack_of(shape, lens)
    x3 = route == "conv_sk2_x3"
    xrefs = x3_of(shape, lens) if x3 else None
    tol = X3_TOL if x3 else TOL
    worst = 0.0
    try:
        for on in EPILOGUES:
            twin = on is not False
            slope = 0.3 if on is True else 0.1
            ref, ref2 = refs[on]
            for G in grids or grids_of(route, shape, p.M):
                what = f"{route} {shape} {pack} on={on} G={G}"
                out, out2 = launch(lib, p, route, G, on, twin)
                err = check_output(p, out, out2, ref, ref2, twin, slope, tol, what)
                again, again2 = launch(lib, p, route, G, on, twin)
                assert torch.equal(bits(out), bits(again)) and torch.equal(bits(out2), bits(again2)), f"{what}: two launches, other bits"
                line = f"{what} M={p.M} nseg={len(lens)}: max abs err {err:.3e}"
                if x3:      # against the f32 kernel on the same pack and grid
                    f32, _ = launch(lib, p, "conv_sk2", G, on, twin)
                    check_output(p, f32, _, ref, ref2, twin, slope, TOL, what + " (f32)")
                    diff = (out[:p.M] - f32[:p.M]).double()
                    rel = (diff.pow(2).mean() / f32[:p.M].double().pow(2).mean()).sqrt().item()
                    line += f", vs f32: rel rms {rel:.3e} max abs {diff.abs().max().item():.3e}"
                    print(line)
                    assert 0.0 < rel < X3_REL, f"{what}: relative RMS against the f32 kernel {rel}"
                    assert diff.abs().max().item() < X3_TOL, f"{what}: max abs against the f32 kernel {diff.abs().max().item()}"
                    check_x3(p, out, out2, xrefs[on], twin, what)
                else:
                    print(line)
                worst = max(worst, err)
    finally:
        restore(lib)
    print(f"WORST {route} {shape} {pack}: {worst:.3e}")


CASES = [(route, shape, pack) for shape in SHAPES for pack in ("edges", "short256", "short300")
         for route in ("conv_sk", "conv_sk2", "conv_sk2_x3")]


@pytest.mark.parametrize("route,shape,pack", CASES, ids=[f"{r}-{'x'.join(map(str, s))}-{p}" for r, s, p in CASES])
def test_stream_k_conv_ragged_pack(lib, route, shape, pack):
    check_sk(lib, route, shape, lens_of(pack, ROUTES[route]["bm"], shape[3]), pack)


def test_stream_k_conv_ragged_pack_in_xcd_groups(lib):
    """Tiles dealt to eight groups first (one ticket counter each), stream-K inside a group: only at G >= 64 and >= 64 tiles, so a pack
    of ~4300 rows at N = 256 (34 x 2 tiles of 12 k-steps, 102 workgroups at the most); 72 workgroups: 9 per group on 8.5 tiles."""
    shape = (128, 256, 3, 1)
    lens = pack_lens(128, 1, 4300)
    M = sum(lens)
    assert -(-M // 128) * 2 >= 64 and grid_cap("conv_sk_xcd", shape, M) >= 72
    check_sk(lib, "conv_sk_xcd", shape, lens, "edges4300", grids=(64, 72))


@pytest.mark.parametrize("route", list(ROUTES))
def test_one_utterance_with_and_without_a_segment_table(lib, route):
    """A pack of one utterance: the segment table changes nothing, bit for bit (nseg = 0 bounds every row by in_len)."""
    shape = (128, 256, 3, 1)
    G = 64 if route == "conv_sk_xcd" else 7
    p, refs = pack_of(shape, [4301])
    assert grid_cap(route, shape, p.M) >= G
    try:
        with_table = launch(lib, p, route, G, True, True)
        without = launch(lib, p, route, G, True, True, segmented=False)
    finally:
        restore(lib)
    check_output(p, *with_table, *refs[True], True, 0.3, X3_TOL if route == "conv_sk2_x3" else TOL, f"{route} one utterance")
    if route == "conv_sk2_x3":
        check_x3(p, *with_table, x3_of(shape, [4301])[True], True, f"{route} one utterance G={G}")
    assert torch.equal(bits(with_table[0]), bits(without[0])) and torch.equal(bits(with_table[1]), bits(without[1]))


@pytest.mark.parametrize("route", ["conv_sk", "conv_sk2"])
@pytest.mark.parametrize("cin,cout,k,stride", [(64, 32, 8, 4), (128, 64, 11, 5)])
def test_ragged_polyphase_upsample_against_conv_transpose(lib, route, cin, cout, k, stride):
    """The vocoder's upsampler as it is launched -- leaky-ReLU(0.1) on the input, the ConvTranspose1d as a 3-tap conv with pad 1 and
    N = stride * Cout (weights.convT_polyphase), bias -- over a ragged pack, against torch's own conv_transpose1d in float64 on every
    utterance alone: the polyphase identity at utterance edges."""
    from streamspeech_amd.weights import convT_polyphase
    n = stride * cout
    lens = pack_lens(ROUTES[route]["bm"], 1, 2600)
    p = ConvPack(cin, 3, 1, lens, guard=GUARD, seed=30, N=n)
    wt, b = rnd(cin, cout, k, seed=31, scale=(cin * k / stride) ** -0.5), rnd(cout, seed=32, scale=0.1)
    wp, bp = convT_polyphase(wt, b, stride)
    p.dw.copy_(wp)
    p.db.copy_(bp)
    ref = R.upsample(p.x.double(), wt.double(), b.double(), p.segs, stride, in_slope=0.1)
    M, r = p.M, ROUTES[route]
    assert grid_cap(route, (cin, n, 3, 1), M) >= 7
    try:
        for G in (0, 7):
            out, out2 = out_buf(M, GUARD, n), out_buf(M, GUARD, n)
            a = p.args(False, False, out, out2)
            a.in_act, a.bias = 3, P(p.db)
            assert lib.ss_debug_force_tile(*r["hook"], G) == 0
            errs, before = lib.ss_debug_sk_errors(), census(lib)
            rc = lib.ss_op_conv_gemm_ex(S(), C.byref(a))
            torch.cuda.synchronize()
            assert rc == 0 and took_since(lib, before) == {r["cls"]: 1} and lib.ss_debug_sk_errors() == errs
            out, out2 = out.cpu(), out2.cpu()
            assert torch.isfinite(out[:M]).all() and torch.isnan(out[M:]).all() and torch.isnan(out2).all()
            err = (out[:M].reshape(M * stride, cout).double() - ref).abs().max().item()
            print(f"{route} upsample {cin}->{cout} k={k} s={stride} G={G} M={M} nseg={len(lens)}: max abs err {err:.3e}")
            assert err < TOL, f"{route} G={G}: max abs err {err}"
    finally:
        restore(lib)


def test_default_dispatch_sends_a_packed_conv_pre_to_stream_k(lib):
    """No hook: conv_pre (k = 7, 128 -> 512 channels, bias, the pre-activated twin) over a ragged pack of 20 000 rows.  launch_conv_gemm
    sends it to conv_sk2: 2 M N taps Cin = 1.8e10 flops >= sk_min_flops (4e9) and ceil(M / 128) (N / 128) nk = 157 x 4 x 28 = 17 584
    units >= SS_SK_MIN_UNITS (6144).  One workgroup per CU there: ~35 of the 8848 k-steps each, parts that start and stop mid-tile."""
    for knob in ("SS_SK_MIN_UNITS", "SS_SK_MIN_GFLOP", "SS_NO_SK2"):
        if os.environ.get(knob):
            pytest.skip(f"{knob} is set: the dispatch thresholds are not the defaults")
    shape = (128, 512, 7, 1)
    lens = pack_lens(256, 1, 20000)
    M = sum(lens)
    assert 2.0 * M * 512 * 7 * 128 >= 4e9 and -(-M // 128) * 4 * 28 >= 6144
    p = ConvPack(shape[0], 7, 1, lens, guard=GUARD, seed=50, N=512)
    ref, ref2 = p.ref("up", True)
    errs, before = lib.ss_debug_sk_errors(), census(lib)
    rc, out, out2 = p.run(lib, "up", True)
    assert rc == 0 and took_since(lib, before) == {"conv_sk2<256,128,32>": 1} and lib.ss_debug_sk_errors() == errs
    err = check_output(p, out, out2, ref, ref2, True, 0.1, TOL, "default dispatch")
    print(f"default dispatch conv_pre M={M} nseg={len(lens)}: max abs err {err:.3e}")
