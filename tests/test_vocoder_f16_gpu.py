"""Opt-in FP16 matrix-core ResBlock convs of the vocoder's 64-, 128- and 256-channel stages (ss_vocoder_set_f16, csrc/conv_f16.hip).
Bars: relative RMS against the f32 conv <= 2e-3 per op (and not zero: the FP16 kernel really ran), deterministic, finite under
saturation, output rows pack-invariant; waveform within 1e-3 RMS of the f32 path and of the FP32 oracle with identical durations;
switching it off restores the exact f32 path."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from test_ops_gpu import P, S, lib, rnd, run_conv_gemm  # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu
WAV_RMS_TOL = 1e-3
WIDE_WINOGRAD = ("conv_c64w<256,64>", "conv_c128w<256,128>", "conv_c256w<256,128>")
F16_CLASSES = ("conv_f16<64>", "conv_f16<128>", "conv_f16<256>")


def _launches(lib, name):
    for c in range(lib.ss_prof_num_classes()):
        if lib.ss_prof_class_name(c).decode() == name:
            n = C.c_int64()
            lib.ss_prof_totals(c, None, None, C.byref(n))
            return int(n.value)
    raise KeyError(name)


def _census(lib, names):
    return {n: _launches(lib, n) for n in names}


def run_f16(lib, A, Wp, bias, Cch, taps, dil, in_act=3, R=None, R2=None, div=0.0, segs=None, twin=False):
    from streamspeech_amd import lib as L
    dev = "cuda:0"
    M = A.shape[0]
    dA, dW = A.contiguous().to(dev), Wp.contiguous().to(dev)
    db = None if bias is None else bias.to(dev)
    dR = None if R is None else R.contiguous().to(dev)
    dR2 = None if R2 is None else R2.contiguous().to(dev)
    dC = torch.full((M, Cch), float("nan"), device=dev)
    dC2 = torch.full((M, Cch), float("nan"), device=dev) if twin else None
    dseg = None if segs is None else torch.tensor([v for s in segs for v in s], dtype=torch.int32, device=dev)
    L.check(lib.ss_op_conv_f16(S(), P(dA), P(dW), P(db), P(dR), P(dR2), P(dC), P(dC2), M, Cch, taps, dil, in_act, 0.1, 0, div,
                               P(dseg), 0 if segs is None else len(segs)), "ss_op_conv_f16")
    torch.cuda.synchronize()
    return dC.cpu(), (dC2.cpu() if twin else None)


def _weights(Cch, taps, seed):
    from streamspeech_amd.weights import conv_tap_major
    W = rnd(Cch, Cch, taps, seed=seed, scale=(Cch * taps) ** -0.5)
    return conv_tap_major(W)


def _f32_segments(lib, A, Wp, b, Cch, taps, dil, segs, **kw):
    """The f32 conv of every segment on its own (ss_op_conv_gemm), stitched into the packed rows."""
    out = torch.zeros(A.shape[0], Cch)
    for lo, n, _, _ in segs:
        sub = {k: (v[lo:lo + n] if torch.is_tensor(v) else v) for k, v in kw.items()}
        out[lo:lo + n] = run_conv_gemm(lib, A[lo:lo + n], Wp, b, n, Cch, Cch, taps=taps, dil=dil, pad=dil * (taps - 1) // 2,
                                       in_act=3, slope=0.1, **sub)
    return out


def _rel(got, ref):
    return float(((got.double() - ref.double()).pow(2).mean() / ref.double().pow(2).mean()).sqrt())


@pytest.mark.parametrize("Cch", [64, 128, 256])
@pytest.mark.parametrize("taps,dil", [(3, 1), (7, 3), (11, 5)])
@pytest.mark.parametrize("M", [1, 257, 20011])
def test_conv_f16_close_to_f32(lib, Cch, taps, dil, M):
    """The FP16 conv against the f32 conv on the same launch (input leaky-ReLU, bias, residual): relative RMS in (0, 2e-3],
    two runs bitwise equal, an input scaled to 1e5 (past the FP16 range: saturated while staging) stays finite."""
    A = rnd(M, Cch, seed=31)
    Wp = _weights(Cch, taps, 32)
    b, R = rnd(Cch, seed=33, scale=0.1), rnd(M, Cch, seed=34)
    n0 = _launches(lib, f"conv_f16<{Cch}>")
    got, _ = run_f16(lib, A, Wp, b, Cch, taps, dil, R=R)
    got2, _ = run_f16(lib, A, Wp, b, Cch, taps, dil, R=R)
    assert _launches(lib, f"conv_f16<{Cch}>") == n0 + 2
    ref = run_conv_gemm(lib, A, Wp, b, M, Cch, Cch, taps=taps, dil=dil, pad=dil * (taps - 1) // 2, in_act=3, slope=0.1, R=R)
    assert torch.isfinite(got).all() and torch.equal(got, got2)
    rel = _rel(got - R, ref - R)            # the conv part (the residual is added in f32 and would hide the FP16 error)
    assert 0.0 < rel <= 2e-3, rel
    big, _ = run_f16(lib, A * 1e5, Wp, b, Cch, taps, dil)
    assert torch.isfinite(big).all()


@pytest.mark.parametrize("Cch,taps,dil", [(64, 11, 5), (128, 7, 3), (256, 3, 1), (256, 11, 5)])
def test_conv_f16_ragged_epilogue(lib, Cch, taps, dil):
    """A ragged segment table (lengths 1 .. 700, zero padding at every utterance edge) with the last ResBlock conv's epilogue:
    residual, MRF sum, / n_res and the pre-activated twin C2 = leaky_relu(C, 0.1), against the f32 conv segment by segment."""
    lens = [1, 700, 37, 255, 256, 513, 3, 129]
    segs, off = [], 0
    for n in lens:
        segs.append((off, n, off, n))
        off += n
    M = off
    A = rnd(M, Cch, seed=41)
    Wp = _weights(Cch, taps, 42)
    b, R, R2 = rnd(Cch, seed=43, scale=0.1), rnd(M, Cch, seed=44), rnd(M, Cch, seed=45)
    got, twin = run_f16(lib, A, Wp, b, Cch, taps, dil, R=R, R2=R2, div=3.0, segs=segs, twin=True)
    ref = _f32_segments(lib, A, Wp, b, Cch, taps, dil, segs, R=R, R2=R2, div=3.0)
    assert torch.isfinite(got).all()
    rel = _rel(got - (R + R2) / 3.0, ref - (R + R2) / 3.0)
    assert 0.0 < rel <= 2e-3, rel
    assert torch.equal(twin, torch.where(got > 0, got, got * 0.1))


@pytest.mark.parametrize("Cch,taps,dil", [(64, 7, 3), (128, 11, 5), (256, 3, 1), (256, 11, 1)])
def test_conv_f16_rows_pack_invariant(lib, Cch, taps, dil):
    """One utterance's rows as a segment at different offsets of a ragged launch, alone and among 15 others (and as an unsegmented
    launch): its output rows are bit-identical every time."""
    rng = random.Random(Cch + taps)
    L0 = 601
    U = rnd(L0, Cch, seed=51)
    Wp = _weights(Cch, taps, 52)
    b = rnd(Cch, seed=53, scale=0.1)
    alone, _ = run_f16(lib, U, Wp, b, Cch, taps, dil)
    seg_alone, _ = run_f16(lib, U, Wp, b, Cch, taps, dil, segs=[(0, L0, 0, L0)])
    assert torch.equal(alone, seg_alone)
    for pos in (0, 5, 15):
        parts, segs, off, where = [], [], 0, None
        for k in range(16):
            if k == pos:
                x, where = U, off
            else:
                x = rnd(rng.randrange(1, 900), Cch, seed=100 + k)
            parts.append(x)
            segs.append((off, x.shape[0], off, x.shape[0]))
            off += x.shape[0]
        got, _ = run_f16(lib, torch.cat(parts), Wp, b, Cch, taps, dil, segs=segs)
        assert torch.equal(got[where:where + L0], alone), pos


def _codes(n, seed):
    from streamspeech_amd import synth
    return [int(c) for c in synth.uniform(5, f"f16_codes_{seed}", (n,), 0, 1000)]


def test_f16_vocoder_single_vs_f32_and_oracle(hip_vocoder, synth_weights):
    """Single utterance: FP16 against f32 within 1e-3 RMS (not identical), same durations; against the FP32 oracle within 1e-3;
    FP16 launches counted and no wide Winograd launch; switched off, the handle is bit-identical to a fresh one."""
    from oracle import streamspeech_oracle as O
    _, vcfg, _, vsd = synth_weights
    lib_ = hip_vocoder.lib
    f32 = hip_vocoder.new_context()
    f16 = hip_vocoder.new_context()
    f16.set_fp16(True)
    codes = _codes(90, 1)
    w_ref, d_ref = f32.forward(codes, True)
    c0 = _census(lib_, F16_CLASSES + WIDE_WINOGRAD)
    w16, d16 = f16.forward(codes, True)
    torch.cuda.synchronize()
    c1 = _census(lib_, F16_CLASSES + WIDE_WINOGRAD)
    assert all(c1[n] > c0[n] for n in F16_CLASSES), (c0, c1)
    assert all(c1[n] == c0[n] for n in WIDE_WINOGRAD), (c0, c1)
    assert d16.cpu().tolist() == d_ref.cpu().tolist()
    assert w16.shape == w_ref.shape
    rms = float(torch.sqrt(torch.mean((w16 - w_ref) ** 2)))
    assert 0.0 < rms <= WAV_RMS_TOL, rms
    rw, rd = O.vocoder_forward(vsd, codes, vcfg, True)
    assert d16.cpu().tolist() == rd.tolist()
    assert float(torch.sqrt(torch.mean((w16.cpu() - rw) ** 2))) <= WAV_RMS_TOL
    f16.set_fp16(False)
    w_back, _ = f16.forward(codes, True)
    assert torch.equal(w_back, w_ref), "fp16 off must be the exact f32 path again"
    print(f"fp16 single: rms vs f32 {rms:.2e}")


def test_f16_vocoder_batch_vs_f32_and_oracle(hip_vocoder, synth_weights):
    """Ragged batch (8 utterances): the same bars per utterance; a context made from an FP16 handle inherits the switch."""
    from oracle import streamspeech_oracle as O
    _, vcfg, _, vsd = synth_weights
    lens = [60, 170, 95, 130, 150, 77, 110, 165]
    codes = [_codes(n, 10 + i) for i, n in enumerate(lens)]
    lib_ = hip_vocoder.lib
    f32 = hip_vocoder.new_context()
    f16 = hip_vocoder.new_context()
    f16.set_fp16(True)
    inh = f16.new_context()
    assert inh.fp16
    w_ref, d_ref, _ = f32.batch_forward(codes, True)
    c0 = _census(lib_, F16_CLASSES + WIDE_WINOGRAD)
    w16, d16, _ = inh.batch_forward(codes, True)
    torch.cuda.synchronize()
    c1 = _census(lib_, F16_CLASSES + WIDE_WINOGRAD)
    assert all(c1[n] > c0[n] for n in F16_CLASSES), (c0, c1)
    assert all(c1[n] == c0[n] for n in WIDE_WINOGRAD), (c0, c1)
    assert d16.cpu().tolist() == d_ref.cpu().tolist()
    worst = 0.0
    for a, b in zip(w16, w_ref):
        assert a.shape == b.shape
        rms = float(torch.sqrt(torch.mean((a - b) ** 2)))
        worst = max(worst, rms)
        assert 0.0 < rms <= WAV_RMS_TOL, rms
    for i in (1, 5):
        off = sum(lens[:i])
        rw, rd = O.vocoder_forward(vsd, codes[i], vcfg, True)
        assert d16.cpu().tolist()[off: off + lens[i]] == rd.tolist()
        assert float(torch.sqrt(torch.mean((w16[i].cpu() - rw) ** 2))) <= WAV_RMS_TOL
    f16.set_fp16(False)
    w_back, _, _ = f16.batch_forward(codes, True)
    for a, b in zip(w_back, w_ref):
        assert torch.equal(a, b), "fp16 off must be the exact f32 path again"
    print(f"fp16 batch: worst rms vs f32 {worst:.2e}")


def test_f16_streaming_tails_match_full_synthesis(hip_vocoder):
    """In FP16, the agent's receptive-field tail (synthesize_tail) and the batched tail entry point equal the tail of the full FP16
    synthesis within the f32 tail tests' 1e-5."""
    from streamspeech_amd.agent import synthesize_tail
    from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
    v = hip_vocoder.new_context()
    v.set_fp16(True)

    class Surf:
        hip = v

        def __call__(self, x, dur_prediction=False):
            return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)

    surf = Surf()
    rf = v.cfg.receptive_field_frames()
    rng = random.Random(7)
    rows = [([rng.randrange(0, 1000) for _ in range(K)], n) for K, n in ((120, 5), (90, 3), (150, 8))]
    ctx = rf + 8
    tails, info = v.batch_tail([u for u, _ in rows], [n for _, n in rows], [ctx] * len(rows), [rf] * len(rows))
    for (units, n_new), t, (first, dur) in zip(rows, tails, info):
        full, _ = synthesize_tail(surf, units, n_new, True, 0, rf)
        inc, _ = synthesize_tail(surf, units, n_new, True, ctx, rf)
        assert inc.numel() == full.numel() == t.numel()
        assert float((inc - full).abs().max()) <= 1e-5
        assert float((t - full).abs().max()) <= 1e-5


def test_offline_driver_vocoder_fp16(tmp_path):
    """--vocoder-fp16 on synthetic:0: the text and unit outputs identical to the f32 run, every waveform within the bar."""
    from streamspeech_amd import frontend, offline
    outs = {}
    for tag, extra in (("f32", []), ("f16", ["--vocoder-fp16"])):
        d = tmp_path / tag
        offline.main(["--path", "synthetic:0", "--vocoder", "synthetic:0", "--synthetic", "3", "--results-path", str(d),
                      "--dur-prediction", "--max-len-b-mt", "12"] + extra)
        outs[tag] = d
    files = sorted(str(p.relative_to(outs["f32"])) for p in outs["f32"].rglob("*") if p.is_file())
    assert files == sorted(str(p.relative_to(outs["f16"])) for p in outs["f16"].rglob("*") if p.is_file())
    wavs = [f for f in files if f.endswith(".wav")]
    texts = [f for f in files if not f.endswith(".wav")]
    assert wavs and all(any(f.endswith(e) for f in texts) for e in (".asr", ".tgt", ".unit")), files
    for f in texts:
        if f.endswith(".log"):
            continue                                  # (progress log)
        assert (outs["f32"] / f).read_bytes() == (outs["f16"] / f).read_bytes(), f
    for f in wavs:
        a, _ = frontend.read_wav(str(outs["f32"] / f))
        b, _ = frontend.read_wav(str(outs["f16"] / f))
        assert a.shape == b.shape
        assert float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))) <= WAV_RMS_TOL, f


def test_set_fp16_refuses_a_plan_the_kernel_cannot_take(synth_weights):
    """A ResBlock plan whose (kernel size - 1) x dilation passes 64 (k = 11 at dilation 7) is refused by the switch itself
    (SS_ERR_ARG), and the handle stays on the f32 path and keeps working."""
    import dataclasses
    from streamspeech_amd import lib as L
    from streamspeech_amd import synth
    from streamspeech_amd.engine import HipVocoder
    _, vcfg, _, _ = synth_weights
    dils = [list(d) for d in vcfg.resblock_dilation_sizes]
    dils[-1][-1] = 7
    cfg = dataclasses.replace(vcfg, resblock_dilation_sizes=[tuple(d) if isinstance(vcfg.resblock_dilation_sizes[0], tuple) else d
                                                              for d in dils])
    assert max(k for k in cfg.resblock_kernel_sizes) == 11
    v = HipVocoder(synth.make_vocoder_state_dict(0, cfg), cfg)
    with pytest.raises(L.StreamSpeechHipError) as e:
        v.set_fp16(True)
    assert e.value.code == L.SS_ERR_ARG
    assert not getattr(v, "fp16", False)
    n0 = _census(v.lib, F16_CLASSES)
    wav, dur = v.forward(_codes(20, 3), True)
    torch.cuda.synchronize()
    assert torch.isfinite(wav).all() and wav.numel() == int(dur.sum()) * v.hop
    assert _census(v.lib, F16_CLASSES) == n0
