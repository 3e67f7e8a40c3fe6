"""The two block shapes of the 256-channel Winograd slab conv (csrc/conv_c64w.hip, Dispatch::c256w_rows): blocks of 128 / 126 / 120 rows
over all 256 output columns in one workgroup (the default) against blocks of 256 / 252 / 240 rows split between two workgroups by column
half.  Op level through ss_op_conv_gemm_ex with a segment table against tests/slab_ref.py (float64), built as tests/test_slab_ops_gpu.py
builds its cases -- the pack here is laid around the 128-row form's block height -- and through HipVocoder.batch_forward.

Both forms give every output element the same products in the same order, so wherever two runs are compared the comparison is of bits:
128 rows against 256 rows, and the 128-row form against itself at the default grid, at three workgroups and at a grid of 17.
"""
import pytest
import torch

from tests import slab_ref as R  # noqa: F401  (ConvPack's reference)
from tests.test_slab_ops_gpu import (KD, TOL, ConvPack, bits, census, lib, pack_lens, restore as restore_slab,  # noqa: F401
                                     took_since)

pytestmark = pytest.mark.gpu

BM128 = {1: 128, 3: 126, 5: 120}        # block heights of the 128-row form (whole pairs)
CLS = "conv_c256w<256,128>"
GRIDS = (0, 3, 17)                      # default, three workgroups, a count co-prime to the pack's block counts


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """A launch that faulted leaves the process without a usable device: end the run there instead of failing every later test."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


def restore(lib):
    restore_slab(lib)
    lib.ss_debug_conv_c256_rows(0)


def run(lib, p, on, rows, grid):
    """One launch of the pack at a block shape and a grid cap: (out, twin), having checked the return code and the census."""
    assert lib.ss_debug_conv_c256_rows(rows) == 0
    assert lib.ss_debug_slab(grid, 0) == 0
    before = census(lib)
    rc, out, out2 = p.run(lib, on, bool(on))
    assert rc == 0, f"rows={rows} on={on} grid={grid}: rc {rc}"
    took = took_since(lib, before)
    assert took == {CLS: 1}, f"rows={rows} on={on} grid={grid}: launches by class {took}"
    return out, out2


def test_hook_values(lib):
    try:
        for bad in (-1, 1, 64, 127, 129, 512):
            assert lib.ss_debug_conv_c256_rows(bad) == 2          # SS_ERR_ARG
        for ok in (128, 256, 0):
            assert lib.ss_debug_conv_c256_rows(ok) == 0
    finally:
        restore(lib)


@pytest.mark.parametrize("k,d", KD, ids=[f"k{k}-d{d}" for k, d in KD])
def test_rows128_ragged_pack(lib, k, d):
    """Both epilogue settings: float64 error, twin, guard rows; the 128-row form bit-equal to the 256-row form and to itself at every grid."""
    bm = BM128[d]
    p = ConvPack(256, k, d, pack_lens(bm, d), guard=bm)
    M = p.M
    try:
        assert lib.ss_debug_conv_c64(9) == 0
        for on in (True, False):
            ref, ref2 = p.ref(on, bool(on))
            runs = [run(lib, p, on, 128, grid) for grid in GRIDS]
            wide = run(lib, p, on, 256, 0)
            out, out2 = runs[0]
            err = (out[:M].double() - ref).abs().max().item()
            print(f"conv_c256w rows=128 k={k} d={d} on={on} M={M} nseg={len(p.segs)}: max abs err {err:.3e}")
            assert torch.isfinite(out[:M]).all() and err < TOL, f"on={on}: max abs err {err}"
            assert torch.isnan(out[M:]).all(), "rows behind the pack were written"
            if on:
                assert torch.equal(out2[:M], torch.where(out[:M] > 0, out[:M], out[:M] * 0.3)), "twin != leaky_relu(C, c2_slope)"
                assert (out2[:M].double() - ref2).abs().max() < TOL
                assert torch.isnan(out2[M:]).all()
            else:
                assert torch.isnan(out2).all(), "an unbound twin was written"
            for grid, (o, o2) in zip(GRIDS[1:], runs[1:]):
                assert torch.equal(bits(out), bits(o)), f"on={on}: grid {grid} gives other bits"
                assert torch.equal(bits(out2), bits(o2)), f"on={on}: grid {grid} gives another twin"
            assert torch.equal(bits(out), bits(wide[0])), f"on={on}: 128-row and 256-row blocks give other bits"
            assert torch.equal(bits(out2), bits(wide[1])), f"on={on}: 128-row and 256-row blocks give another twin"
    finally:
        restore(lib)


def test_vocoder_waveforms_do_not_depend_on_the_block_shape(lib, hip_vocoder):
    """Three utterances through the whole generator with the row thresholds lifted, so that the 256-channel stage of this small pack
    runs on the Winograd slab kernel: the same waveform bits at both block shapes."""
    from streamspeech_amd import synth
    codes = [[int(c) for c in synth.uniform(29, f"c256rows/{i}", (n,), 0, 1000)] for i, n in enumerate((40, 57, 75))]
    durs = [[1 + (j % 3 == 1) for j in range(len(c))] for c in codes]
    wavs = {}
    try:
        assert lib.ss_debug_slab(0, 0) == 0
        for rows in (128, 256):
            assert lib.ss_debug_conv_c256_rows(rows) == 0
            n0 = census(lib)[CLS]
            wavs[rows] = [w.clone() for w in hip_vocoder.batch_forward(codes, True, forced_dur=durs)[0]]
            torch.cuda.synchronize()
            assert census(lib)[CLS] > n0, "the 256-channel stage did not take the Winograd slab kernel"
    finally:
        restore(lib)
    for i, (a, b) in enumerate(zip(wavs[128], wavs[256])):
        assert a.numel() == 320 * sum(durs[i]) and torch.isfinite(a).all()
        assert torch.equal(a, b), f"utterance {i}: max diff {(a - b).abs().max().item()}"
