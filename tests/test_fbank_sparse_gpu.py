"""The fbank kernels on the model's tables (csrc/fbank.hip: the non-zero bin range of every mel row, the FFT twiddles filled once per
model) against the form they replace -- all 257 bins of every mel row, sincospif in the kernel -- which ss_debug_fbank_dense(1) keeps
reachable.  The bins left out are exact zeros, fmaf(0, x, e) == e for a finite power spectrum, the walk keeps its ascending order
and its start value, and the table holds what the same sincospif expression gives: the feature rows must be the same BITS.

Inputs: all-zero PCM, a full-scale 1-kHz sine, seeded noise.  Lengths: 400 samples (one frame), 560 (two frames) and a ragged pack
of 400 / 1999 / 4000 samples.  Through ss_batch_fbank_cmvn, and through the resampling form ss_batch_fbank_frames_sr on the same
signals at 48 kHz (three times the samples).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PACKS = {"one frame": [400], "two frames": [560], "ragged pack": [400, 1999, 4000]}


def _signal(kind, n, sr):
    if kind == "zero":
        x = np.zeros(n, np.float32)
    elif kind == "sine":
        x = np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / sr).astype(np.float32)       # full scale: pcm_scale takes it to +-32768
    else:
        x = np.random.default_rng(77 + n).uniform(-0.5, 0.5, n).astype(np.float32)
    return torch.from_numpy(x).cuda()


@pytest.fixture()
def dense(hip_model):
    lib = hip_model.lib

    def set_dense(on):
        assert lib.ss_debug_fbank_dense(int(on)) == 0
    yield set_dense
    assert lib.ss_debug_fbank_dense(-1) == 0


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("pack", list(PACKS))
@pytest.mark.parametrize("kind", ["zero", "sine", "noise"])
def test_batch_fbank_cmvn_same_bits(hip_model, dense, kind, pack):
    ns = PACKS[pack]
    pcm = torch.cat([_signal(kind, n, 16000) for n in ns])
    dense(0)
    got, T = hip_model.batch_fbank_cmvn(pcm, ns)
    dense(1)
    want, T1 = hip_model.batch_fbank_cmvn(pcm, ns)
    assert T == T1 == [1 + (n - 400) // 160 for n in ns]
    assert torch.isfinite(want).all()
    assert torch.equal(_bits(got), _bits(want)), f"{kind}, {pack}: rows on the tables differ from the dense rows"


@pytest.mark.parametrize("pack", list(PACKS))
@pytest.mark.parametrize("kind", ["zero", "sine", "noise"])
def test_batch_fbank_frames_sr_same_bits(hip_model, dense, kind, pack):
    from streamspeech_amd.engine import fbank_sr_rows, resample_ratio
    sr = 48000
    up, down, half = resample_ratio(sr)
    n_in = [3 * n for n in PACKS[pack]]
    hist = [_signal(kind, n, sr) for n in n_in]
    rows = [fbank_sr_rows(n, up, down, half, hip_model.lib)[0] for n in n_in]
    assert rows == [1 + (n - 400) // 160 for n in PACKS[pack]]

    def run():
        outs = [torch.full((r, 80), float("nan"), device="cuda") for r in rows]
        hip_model.batch_fbank_frames_sr(hist, n_in, [sr] * len(hist), [0] * len(hist), rows, outs)
        return torch.cat(outs)
    dense(0)
    got = run()
    dense(1)
    want = run()
    assert torch.isfinite(want).all()
    assert torch.equal(_bits(got), _bits(want)), f"{kind}, {pack} at 48 kHz: rows on the tables differ from the dense rows"


def test_switch_refuses_other_values(hip_model):
    assert hip_model.lib.ss_debug_fbank_dense(2) == 2 and hip_model.lib.ss_debug_fbank_dense(-2) == 2
