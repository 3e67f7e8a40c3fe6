"""Op-level tests of the FP16 matrix-core conv conv_f16 (csrc/conv_f16.hip, behind ss_vocoder_set_f16) through ss_op_conv_f16, against
the float64 conv of the operands the kernel really multiplies (tests/slab_ref.py conv_f16: input leaky-ReLU in float32, clamp to
+-65504, round to nearest even).  Every product of two FP16 values is exact in float32, so the kernel may differ from that reference
by float32 accumulation only, and the bound is 16 E_case, E_case the distance of the float32-accumulated CPU reference to the float64
one (tests/rounded_cases.py; about 1e-5, where a bound against unrounded operands could not go under 2e-3).  At that bound a wrong
channel of one tap, rounding toward zero and flushed FP16 subnormals all show; tests/test_slab_ref_cpu.py checks that on the
references alone, for every pack used here.

The harness is that of tests/test_slab_ops_gpu.py: rows of 1e4 (an FP16 value) around every input, NaN outputs with a NaN guard block
behind the pack, a census over every profiler class, the default grid against ss_debug_slab(3, 0) bit for bit.
"""
import ctypes as C

import pytest
import torch

from tests import rounded_cases as RC
from tests import slab_ref as R
from test_slab_ops_gpu import (DEV, SHORT_256, SS_ERR_ARG, P, Rows, S, bits, census, lib, out_buf, pack_lens, restore,  # noqa: F401
                               seg_dev, stop_after_a_gpu_error, took_since)

pytestmark = pytest.mark.gpu

assert RC.short_lens(256) == SHORT_256 and RC.pack_lens(128, 5) == pack_lens(128, 5)      # the f32 tests' packs, extended


class F16Pack:
    """One host case (tests/rounded_cases.py) on the device.  on: everything ss_op_conv_f16 exposes (input leaky-ReLU 0.1, bias,
    epilogue leaky-ReLU, R, R2, / 3, the twin) or the plain conv."""

    def __init__(self, h):
        from streamspeech_amd.weights import conv_tap_major
        self.h, self.guard = h, RC.F16_BM[h.C]
        self.dx, self.dR, self.dR2 = Rows(h.x, self.guard), Rows(h.R, self.guard), Rows(h.R2, self.guard)
        self.dw, self.db, self.dsegs = conv_tap_major(h.w).to(DEV), h.b.to(DEV), seg_dev(h.segs)

    def run(self, lib, on, twin, segmented=True, in_act=None):
        h = self.h
        out, out2 = out_buf(h.M, self.guard, h.C), out_buf(h.M, self.guard, h.C)
        rc = lib.ss_op_conv_f16(S(), self.dx.ptr, P(self.dw), P(self.db) if on else None, self.dR.ptr if on else None,
                                self.dR2.ptr if on else None, P(out), P(out2) if twin else None, h.M, h.C, h.k, h.d,
                                (3 if on else 0) if in_act is None else in_act, 0.1, 3 if on else 0, 3.0 if on else 0.0,
                                P(self.dsegs) if segmented else None, len(h.segs) if segmented else 0)
        torch.cuda.synchronize()
        return rc, out.cpu(), out2.cpu()


def two_grids(lib, p, what, launches, **kw):
    """The launch at the default grid and at three workgroups: rc, the census (conv_f16<C> `launches` times, nothing else), the same
    bits.  Returns the first run."""
    runs = []
    for grid in (0, 3):
        assert lib.ss_debug_slab(grid, 0) == 0
        before = census(lib)
        rc, out, out2 = p.run(lib, **kw)
        assert rc == 0, f"{what} grid={grid}: rc {rc}"
        took = took_since(lib, before)
        assert took == {f"conv_f16<{p.h.C}>": launches}, f"{what} grid={grid}: launches by class {took}"
        runs.append((out, out2))
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])), f"{what}: three workgroups give other bits"
    assert torch.equal(bits(runs[0][1]), bits(runs[1][1])), f"{what}: three workgroups give other twin bits"
    return runs[0]


_refs = {}


def refs_of(key, h, on):
    """f16_refs of a case, kept for the test that comes next on the same pack."""
    if (key, on) not in _refs:
        while len(_refs) >= 4:
            del _refs[next(iter(_refs))]
        _refs[(key, on)] = RC.f16_refs(h, on)
    return _refs[(key, on)]


def check_f16(lib, key, h, what, launches=1, segmented=True, edge_segs=()):
    """Both epilogue settings of one pack: census, finite, max abs against R.conv_f16 under 16 E, the twin, guard rows, grid-3 bits."""
    p, M = F16Pack(h), h.M
    try:
        for on in (True, False):
            refs = refs_of(key, h, on)
            out, out2 = two_grids(lib, p, f"{what} on={on}", launches, on=on, twin=on, segmented=segmented)
            assert torch.isfinite(out[:M]).all(), f"{what} on={on}: not finite over the pack"
            err = RC.err(out[:M], refs.ref)
            dist = " ".join(f"[{n}: {RC.err(m, refs.ref):.2e}]" for n, m in refs.mutants.items())
            print(f"{what} on={on} M={M} nseg={len(h.segs) if segmented else 0}: max abs err {err:.3e} E {refs.E:.3e} bar {refs.bar:.3e} "
                  f"mutants {dist}")
            own = {i: RC.err(out[s:s + n], refs.ref[s:s + n]) for i, (s, n) in enumerate(h.segs) if i in edge_segs}
            assert err < refs.bar <= RC.TOL, f"{what} on={on}: max abs err {err} (bar {refs.bar}); segments {own}"
            assert torch.isnan(out[M:]).all(), f"{what} on={on}: rows behind the pack were written"
            if on:
                assert torch.equal(out2[:M], torch.where(out[:M] > 0, out[:M], out[:M] * 0.1)), f"{what}: twin != leaky_relu(C, 0.1)"
                assert RC.err(out2[:M], refs.ref2) < refs.bar
                assert torch.isnan(out2[M:]).all(), f"{what}: twin rows behind the pack were written"
            else:
                assert torch.isnan(out2).all(), f"{what}: an unbound twin was written"
    finally:
        restore(lib)


EDGE_CASES = [(Cc, k, d) for Cc in (64, 128, 256) for (k, d) in RC.KD]


# ---- a. ragged edge packs ------------------------------------------------------------------------
@pytest.mark.parametrize("Cc,k,d", EDGE_CASES, ids=[f"c{c}-k{k}-d{d}" for c, k, d in EDGE_CASES])
def test_conv_f16_ragged_pack(lib, Cc, k, d):
    """Utterances of 1, 2, d - 1, d, d + 1, BM - 1, BM, BM + 1, 2 BM + 3 rows and a long one at the kernel's block height (512 / 256 /
    128): zero padding at every edge, utterances shorter than the halo, blocks that end on an edge."""
    check_f16(lib, ("edge", Cc, k, d), RC.f16_edge_case(Cc, k, d), f"conv_f16 C={Cc} k={k} d={d}")


@pytest.mark.parametrize("Cc", [64, 128, 256])
def test_conv_f16_unsegmented(lib, Cc):
    """nseg = 0, M = 2 BM + 37: the last block is a partial one bounded by M."""
    check_f16(lib, ("unseg", Cc), RC.f16_unsegmented_case(Cc), f"conv_f16 C={Cc} k=7 d=3 unsegmented", segmented=False)


# ---- b. nearest reference, no tolerance ----------------------------------------------------------
@pytest.mark.parametrize("Cc,k,d", [(256, 11, 5), (64, 3, 1)])
def test_conv_f16_is_nearest_to_its_own_rounding(lib, Cc, k, d):
    """The kernel's distance to R.conv_f16 is less than half its distance to each mutant reference: activations / weights rounded
    toward zero, FP16-subnormal weights / activations flushed (the pack holds 96 rows of subnormal activations)."""
    h = RC.f16_edge_case(Cc, k, d)
    p = F16Pack(h)
    try:
        for on in (True, False):
            refs = refs_of(("edge", Cc, k, d), h, on)
            rc, out, _ = p.run(lib, on, on)
            assert rc == 0 and torch.isfinite(out[:h.M]).all()
            near = RC.nearest(out, refs, h.M)
            print(f"conv_f16 C={Cc} k={k} d={d} on={on}: to its reference {next(iter(near.values()))[0]:.3e}, to the mutants "
                  + " ".join(f"[{n}: {dm:.3e}]" for n, (_, dm) in near.items()))
            for n, (d0, dm) in near.items():
                assert d0 < 0.5 * dm, f"on={on}: {d0} from the reference, {dm} from '{n}'"
    finally:
        restore(lib)


# ---- c. exact indexing at zero tolerance ---------------------------------------------------------
LATTICE_CASES = [(Cc, k, d, Cc == 128 and k == 11) for Cc in (64, 128, 256) for (k, d) in ((11, 5), (3, 1))]


@pytest.mark.parametrize("Cc,k,d,sat", LATTICE_CASES, ids=[f"c{c}-k{k}-d{d}" + ("-sat" if s else "") for c, k, d, s in LATTICE_CASES])
def test_conv_f16_selection_weights_bit_for_bit(lib, Cc, k, d, sat):
    """Selection weights (one power of two per output channel, at a seeded (tap, input channel) that covers every tap and channel) on
    inputs from a lattice of FP32 values with known FP16 images -- normals, ties, FP16 subnormals down to 2^-24 and the tie under
    it, +-65504, 65519.9, 65520, +-1e5, +-inf, -0.0; one case with weights of +-1e6 (saturated to +-65504 by the pack kernel).  One
    non-zero exact product per sum: the output equals the reference BIT FOR BIT, input activation off and on.  A mismatch names the
    lattice points behind it (FP16-subnormal points alone would mean the f16 MFMA flushes them)."""
    h = RC.lattice_case(Cc, k, d, saturated_weights=sat)
    p, M = F16Pack(h), h.M
    names = [n for n, _, _ in RC.LATTICE] + ["(outside the utterance)"]
    try:
        for in_act, slope in ((0, None), (3, 0.1)):
            what = f"conv_f16 lattice C={Cc} k={k} d={d} in_act={in_act}"
            ref = R.conv_f16(h.x, h.w, h.segs, d, in_slope=slope).float()
            out, out2 = two_grids(lib, p, what, 1, on=False, twin=False, in_act=in_act)
            assert torch.isfinite(out[:M]).all(), f"{what}: not finite"
            bad = bits(out[:M]) != bits(ref)
            points = {names[i]: int((h.src[bad] == i).sum()) for i in sorted(set(h.src[bad].tolist()))}
            worst = RC.err(out[:M], ref)
            print(f"{what} M={M}: {int(bad.sum())} of {bad.numel()} outputs differ (max abs {worst:.3e}); lattice points behind them: {points}")
            assert not bad.any(), f"{what}: {int(bad.sum())} outputs differ, max abs {worst}, by lattice point {points}"
            assert torch.isnan(out[M:]).all() and torch.isnan(out2).all()
    finally:
        restore(lib)


# ---- d. the segment-table slices -----------------------------------------------------------------
@pytest.mark.parametrize("Cc,k,d,nseg", RC.SLICE_CASES, ids=[f"c{c}-k{k}-d{d}-n{n}" for c, k, d, n in RC.SLICE_CASES])
def test_conv_f16_segment_table_slices(lib, Cc, k, d, nseg):
    """More utterances than one launch takes (F16_MAXSEG = 1024): launch_f16_t issues one launch per slice of the table.  1024 (one
    full slice), 1025 (a slice of one utterance) and 2049 utterances of 1 .. 16 rows; the failure message carries the error over
    the utterances on either side of the first slice edge."""
    launches = -(-nseg // RC.F16_MAXSEG)
    check_f16(lib, ("slice", Cc, k, d, nseg), RC.f16_slice_case(Cc, k, d, nseg), f"conv_f16 C={Cc} k={k} d={d} slices",
              launches=launches, edge_segs=(1023, 1024))


# ---- e. refusals ---------------------------------------------------------------------------------
def test_conv_f16_refusals(lib):
    """What launch_conv_f16 does not take comes back as SS_ERR_ARG with the outputs untouched."""
    M = 300
    x, w, b = torch.zeros(M, 256, device=DEV), torch.zeros(256, 11 * 256, device=DEV), torch.zeros(256, device=DEV)
    out, out2 = out_buf(M, 16, 256), out_buf(M, 16, 256)
    segs = seg_dev(R.seg_table([100, 200]))

    def call(Cc=64, k=3, d=1, in_act=0, in_slope=0.1, act=0, rows=M, table=None, nseg=0):
        return lib.ss_op_conv_f16(S(), P(x), P(w), P(b), None, None, P(out), P(out2), rows, Cc, k, d, in_act, in_slope, act, 0.0,
                                  P(table), nseg)
    try:
        assert call(k=11, d=7) == SS_ERR_ARG                    # halo (taps - 1) dil = 70 > 64
        assert call(Cc=32) == SS_ERR_ARG
        assert call(in_act=1) == SS_ERR_ARG                     # SiLU on the input
        assert call(in_act=3, in_slope=0.0) == SS_ERR_ARG and call(in_act=3, in_slope=1.0) == SS_ERR_ARG      # fmaxf(v, v * slope)
        assert call(act=4) == SS_ERR_ARG                        # tanh in the epilogue
        assert call(rows=0) == SS_ERR_ARG
        assert call(nseg=2) == SS_ERR_ARG                       # a segment count without a table
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(out2).all()
        assert call(k=11, d=5, in_act=3, act=3, table=segs, nseg=2) == 0       # (the same call without a fault is taken)
        torch.cuda.synchronize()
        for o in (out.flatten(), out2.flatten()):               # zeros in, zeros out: [M, 64] at the head of the buffer, nothing behind
            assert not o[:M * 64].any() and torch.isnan(o[M * 64:]).all()
    finally:
        restore(lib)
