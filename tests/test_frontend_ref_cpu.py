"""tests/frontend_ref.py checked on the host, so that the GPU tests of csrc/fbank.hip (tests/test_frontend_ops_gpu.py) rest on a reference
that is itself pinned: its tables are the kernel's and the oracle's bit for bit, its float64 fbank agrees with oracle/kaldi_fbank.py and the
third-party golden within their bars, its resampler with oracle/resample.py within the derived bound; the float32 twin of the kernel's
algorithm sits inside the intervals on every element of every case, each named mutant of it does not, the intervals are narrow where
they are meant to be, and the constant C_FFT is what a fresh measurement of the twin gives."""
import math
import os

import numpy as np
import pytest

from tests import frontend_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FBANK_MAX_TOL, FBANK_RMS_TOL = 5e-4, 1e-5       # the bars of tests/test_oracle_golden.py on log-mel values
WIDE = 1e-3                                     # an interval wider than this holds nothing to float32 precision
WIDE_CAP = 0.01                                 # largest share of such intervals on a tight case


@pytest.fixture(scope="module")
def stats():
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    return g["mean"].astype(np.float32), g["std"].astype(np.float32)


@pytest.fixture(scope="module")
def refs():
    """{case: (waveform, tight, fbank_ref64, fbank_bounds)}, computed once."""
    out = {}
    for name, (x, tight) in FR.cases().items():
        ref = FR.fbank_ref64(x)
        out[name] = (x, tight, ref, FR.fbank_bounds(ref))
    return out


def test_tables_are_the_kernels_and_the_oracles():
    from oracle import kaldi_fbank as K
    from streamspeech_amd import weights
    window, melw = FR.tables()
    assert window.dtype == melw.dtype == np.float32 and window.shape == (400,) and melw.shape == (80, 257)
    assert np.array_equal(window.view(np.int32), weights.povey_window().numpy().view(np.int32))
    assert np.array_equal(melw.view(np.int32), weights.mel_banks().numpy().view(np.int32))
    assert np.array_equal(window.view(np.int32), K.povey_window().view(np.int32))
    assert np.array_equal(melw.view(np.int32), K.mel_banks().view(np.int32))
    assert FR.FLOOR == float(K.EPS) == float(np.finfo(np.float32).eps) and float(FR.PREEMPH) == float(np.float32(K.PREEMPH))
    assert (melw[:, 256] == 0).all() and window[0] == 0          # the Nyquist bin has no weight; the replicate pad meets a zero


def test_case_list():
    c = FR.cases()
    tight = [n for n, (_, t) in c.items() if t]
    assert tight == ["noise_1s", "noise_short", "noise_ragged", "quiet_1s", "one_frame", "impulse_train"]
    assert [n for n in c if n not in tight] == ["tonal_2s", "dc_offset", "sine_full", "square_440", "alternating", "zeros", "constant"]
    assert all(x.dtype == np.float32 and np.abs(x).max() <= 1.0 for x, _ in c.values())
    assert max(len(x) for x, _ in c.values()) == 48017 == len(c["noise_ragged"][0])


def test_reference_against_oracle_and_golden(refs):
    """log(fbank_ref64) against the float32 oracle and against transformers' Kaldi-compliance values, at test_oracle_golden's bars."""
    from oracle import kaldi_fbank as K
    from oracle import make_golden_fbank as MG
    gold = np.load(os.path.join(ROOT, "tests", "golden", "kaldi_fbank_hf.npz"))
    for name in MG.CASES:
        x, _, ref, _ = refs[name]
        lg = FR.logmel64(ref)
        for what, other in (("oracle", K.fbank(x * np.float32(32768.0))), ("golden", gold[name])):
            assert other.shape == lg.shape == (FR.num_frames(len(x)), 80), (name, what)
            err = np.abs(lg - other.astype(np.float64))
            assert err.max() < FBANK_MAX_TOL and np.sqrt(np.mean(err ** 2)) < FBANK_RMS_TOL, (name, what, err.max())


def test_reference_returns_what_the_bounds_need(refs):
    x, _, ref, _ = refs["noise_short"]
    fr = FR.frames_of(x.astype(np.float64)) * 32768.0
    assert np.allclose(ref["norm"], np.linalg.norm(fr, axis=1), rtol=1e-14) and np.array_equal(ref["absX"], np.abs(ref["X"]))
    assert ref["m"].shape == (23, 80) and ref["X"].shape == (23, 257)
    one = FR.fbank_ref64((x * np.float32(32768.0)).astype(np.float32), 1.0)            # the scale is a power of two: the same frames
    assert np.array_equal(one["m"], ref["m"]) and np.array_equal(one["norm"], ref["norm"])
    assert FR.fbank_ref64(x[:399])["m"].shape == (0, 80)


@pytest.mark.parametrize("sr", [48000, 44100, 8000])
def test_resampler_reference_against_oracle(sr):
    """resample_ref64 (float32 taps, float64 sums) against oracle.resample.resample_poly_ref (float64 taps, float32 result): the two
    differ by one rounding of every tap and one of the result, each at most 2^-24 sum |x h| -- inside the bound wherever the sum has
    three terms, which is everywhere."""
    from oracle.resample import resample_poly_ref
    from streamspeech_amd import synth
    from streamspeech_amd.engine import resample_ratio
    from streamspeech_amd.frontend import design_filter
    up, down, half = resample_ratio(sr)
    taps = design_filter(up, down).astype(np.float32)
    assert len(taps) == 2 * half + 1
    x = synth.synth_pcm(9, 4801)
    n_out = -(-len(x) * up // down)
    y, bound = FR.resample_ref64(x, up, down, taps, half, n_out)
    want = resample_poly_ref(x, 16000, sr)
    assert want.shape == y.shape
    assert (np.abs(y - want) <= bound).all(), float((np.abs(y - want) / bound).max())
    assert bound.max() < 2e-6                                  # no looser than the flat bar of tests/test_stages_gpu.py


def test_resampler_reference_edges():
    """The clamped windows: zero padding at both ends, an impulse returns the taps, one term gives a one-rounding bound."""
    taps = np.arange(1, 8, dtype=np.float32)                  # half = 3
    x = np.array([2.0, 0.0, 0.0, 0.0, 3.0], np.float32)
    y, b = FR.resample_ref64(x, 1, 1, taps, 3, 5)
    full = np.convolve(x.astype(np.float64), taps.astype(np.float64))[3:8]
    assert np.array_equal(y, full)
    y, b = FR.resample_ref64(np.array([1.0], np.float32), 2, 1, taps, 3, 2)           # k = 0: tap 3; k = 1: tap 4
    assert y.tolist() == [4.0, 5.0] and b.tolist() == [4.0 * FR.U, 5.0 * FR.U]
    y, b = FR.resample_ref64(np.zeros(0, np.float32), 1, 3, taps, 3, 0)
    assert y.shape == b.shape == (0,)


def test_cmvn_reference(stats):
    mean, std = stats
    rows = np.linspace(-16, 25, 240, dtype=np.float32).reshape(3, 80)
    assert np.array_equal(FR.cmvn_ref64(rows, mean, std), (rows.astype(np.float64) - mean) / std.astype(np.float64))
    assert np.abs(FR.cmvn32(rows, mean, std) - FR.cmvn_ref64(rows, mean, std)).max() < 2 * FR.U * 8


def test_c_fft_is_the_measured_constant():
    ratios, worst = FR.measure_c_fft()
    print({k: round(v, 2) for k, v in ratios.items()})
    assert max(ratios, key=ratios.get) == "alternating"
    assert abs(worst - FR.TWIN_WORST) < 0.05, worst
    assert FR.C_FFT == math.ceil(2 * worst)


def test_twin_is_inside_the_bounds_everywhere(refs, stats):
    """The unmutated twin, as raw log-mel values and through the float32 CMVN line, on every element of every case; on silence and on
    a constant every value sits on the floor."""
    mean, std = stats
    for name, (x, _, ref, bounds) in refs.items():
        tw = FR.fbank_twin32(x)
        assert tw.dtype == np.float32 and np.isfinite(tw).all(), name
        assert not FR.outside(tw, bounds).any(), (name, int(FR.outside(tw, bounds).sum()))
        with_cmvn = FR.fbank_bounds(ref, mean=mean, std=std)
        assert not FR.outside(FR.cmvn32(tw, mean, std), with_cmvn).any(), name
        if name in FR.FLOOR_CASES:
            assert (tw == np.log(np.float32(FR.FLOOR))).all() and (ref["m"] < FR.FLOOR).all(), name
    # the same intervals for samples that carry the scale already
    x = refs["noise_short"][0]
    assert not FR.outside(FR.fbank_twin32((x * np.float32(32768.0)).astype(np.float32), 1.0), refs["noise_short"][3]).any()


def test_each_mutant_is_caught(refs):
    caught = {m: {} for m in FR.MUTANTS}
    for name, (x, _, _, bounds) in refs.items():
        for m in FR.MUTANTS:
            caught[m][name] = int(FR.outside(FR.fbank_twin32(x, mutant=m), bounds).sum())
    print(caught)
    n = refs["noise_1s"][3][0].size
    assert n == 98 * 80
    for m in FR.MUTANTS:
        assert max(caught[m].values()) > 0, m
        if m != "mean_512":
            assert caught[m]["noise_1s"] > n // 2, (m, caught[m]["noise_1s"])
    assert caught["mean_512"]["noise_1s"] > 0


def test_intervals_are_narrow_where_bins_hold_energy(refs):
    """The non-vacuity cap: on a tight case at most 1 % of the intervals are wider than 1e-3 (one_frame: none), and the median width
    is a few 1e-5.  The other cases' shares are printed (profiles/frontend_accuracy.txt holds a run's)."""
    for name, (_, tight, _, (lo, hi, s, _)) in refs.items():
        share, med = float(((hi - lo) > WIDE).mean()), float(np.median(hi - lo))
        print(f"{name}: {100 * share:.2f} % of the intervals wider than {WIDE:g}, median width {med:.2e}" + ("" if tight else " (reported)"))
        if tight:
            assert share <= WIDE_CAP and med < 5e-5, (name, share, med)
    lo, hi, _, _ = refs["one_frame"][3]
    assert not ((hi - lo) > WIDE).any()
