"""The batched epilogue of the Winograd slab convs (csrc/conv_c64w.hip: conv_c32w / c64w / c128w / c256w) and of the direct conv_c64
(csrc/conv_c64.hip), through ss_op_conv_gemm_ex: slab_epi_batch (csrc/slab_common.hpp) requests every residual of a lane before it
uses one, R2 in a second batch, and stores last.

The check is a composition, bit for bit: one launch with bias, epilogue leaky-ReLU and alpha = 1 gives y; the same launch with R, R2,
div = 3 and (where the route takes one) a twin must give exactly ((y + R) -> R2 + . -> / 3) formed in float32 by torch (on the host, the
divisor a tensor: a true division, as the kernel's), and the twin where(v > 0, v, v * c2_slope).  alpha = 1 makes the kernel's fma(y, alpha, R) the plain sum.  R and R2 may alias the output (the
vocoder passes R == C and R2 == C): a lane must have read an element before it writes it.

Packs, guard rows, NaN outputs and the ss_debug_slab(3, 0) walk are those of tests/test_slab_ops_gpu.py.
"""
import ctypes as C

import pytest
import torch

from tests import test_slab_ops_gpu as T
from tests.test_slab_ops_gpu import lib, stop_after_a_gpu_error  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

EPI_ROUTES = ["conv_c32w", "conv_c64w", "conv_c128w", "conv_c256w", "conv_c64"]
EPI_CASES = [(name, k, d) for name in EPI_ROUTES for (k, d) in T.ROUTES[name].get("kd", T.KD)]
C2_SLOPE = 0.3
# which operands a launch binds: (R, R2) each None / "buf" (its own buffer) / "out" (aliases the output); div and the twin go with
# the full form only
VARIANTS = [("R+R2", "buf", "buf", True), ("R=C", "out", "buf", True), ("R2=C", "buf", "out", True),
            ("R only", "buf", None, False), ("R2 only", None, "buf", False)]


def launch(lib, p, out, out2, R=None, R2=None, div=0.0, twin=False):
    a = p.args(False, False, out, out2)
    a.bias, a.in_act, a.act, a.act_slope, a.alpha = T.P(p.db), 3, 3, 0.2, 1.0
    a.R, a.R2, a.div = R, R2, div
    if twin:
        a.C2, a.c2_slope = T.P(out2), C2_SLOPE
    rc = lib.ss_op_conv_gemm_ex(T.S(), C.byref(a))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name,k,d", EPI_CASES, ids=[f"{n}-k{k}-d{d}" for n, k, d in EPI_CASES])
def test_epilogue_composition(lib, name, k, d):
    r = T.ROUTES[name]
    bm = r["bm"](k, d)
    p = T.ConvPack(r["C"], k, d, T.pack_lens(bm, d, r.get("min_rows", 0)), guard=bm)
    M, Cc = p.M, p.C
    Rd, R2d = p.R.to(T.DEV), p.R2.to(T.DEV)
    three = torch.full((M, Cc), 3.0)
    try:
        for hook in r["hooks"]:
            assert getattr(lib, hook[0])(*hook[1:]) == 0
        plain = {}
        for grid in (0, 3):
            assert lib.ss_debug_slab(grid, 0) == 0
            out, out2 = T.out_buf(M, bm, Cc), T.out_buf(M, bm, Cc)
            n0 = T.launches(lib, r["cls"])
            assert launch(lib, p, out, out2) == 0 and T.launches(lib, r["cls"]) == n0 + 1, f"{name}: not on {r['cls']}"
            assert torch.isfinite(out[:M]).all() and torch.isnan(out[M:]).all() and torch.isnan(out2).all()
            plain[grid] = out
        assert torch.equal(T.bits(plain[0]), T.bits(plain[3])), "neither operand: three workgroups give other bits"
        y = plain[0][:M].cpu()
        for label, Rsrc, R2src, full in VARIANTS:
            twin = full and r["twin"]
            want = y
            if Rsrc:
                want = want + p.R
            if R2src:
                want = p.R2 + want
            if full:
                want = want / three
            runs = []
            for grid in (0, 3):
                assert lib.ss_debug_slab(grid, 0) == 0
                out, out2 = T.out_buf(M, bm, Cc), T.out_buf(M, bm, Cc)
                if Rsrc == "out":
                    out[:M] = Rd
                if R2src == "out":
                    out[:M] = R2d
                ptr = {None: None, "buf": None, "out": T.P(out)}
                Rp = p.dR.ptr if Rsrc == "buf" else ptr[Rsrc]
                R2p = p.dR2.ptr if R2src == "buf" else ptr[R2src]
                n0 = T.launches(lib, r["cls"])
                assert launch(lib, p, out, out2, Rp, R2p, 3.0 if full else 0.0, twin) == 0, f"{name} {label} grid={grid}"
                assert T.launches(lib, r["cls"]) == n0 + 1, f"{name} {label}: not on {r['cls']}"
                runs.append((out, out2))
            out, out2 = runs[0][0].cpu(), runs[0][1].cpu()
            nbad = int((T.bits(out[:M]) != T.bits(want)).sum())
            print(f"{name} k={k} d={d} {label}: M={M}, {nbad} elements differ from the composition")
            assert nbad == 0, f"{name} {label}: {nbad} elements differ from ((y + R) -> R2 + . -> / 3)"
            assert torch.isnan(out[M:]).all(), "rows behind the pack were written"
            if twin:
                assert torch.equal(T.bits(out2[:M]), T.bits(torch.where(out[:M] > 0, out[:M], out[:M] * C2_SLOPE))), "twin"
                assert torch.isnan(out2[M:]).all()
            else:
                assert torch.isnan(out2).all(), "an unbound twin was written"
            assert torch.equal(T.bits(runs[0][0]), T.bits(runs[1][0])), f"{name} {label}: three workgroups give other bits"
            assert torch.equal(T.bits(runs[0][1]), T.bits(runs[1][1]))
    finally:
        T.restore(lib)

