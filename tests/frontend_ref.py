"""Float64 references of the front-end kernels of csrc/fbank.hip, with the error intervals the op tests hold the kernels to, and a
float32 twin of the fbank kernel's own algorithm that the intervals are measured and proven on.  numpy only; nothing here touches a GPU.

    fbank_ref64     fbank_row in float64, from the float32 samples and the float32 tables the kernel reads
    fbank_bounds    per element an interval [lo, hi] and a slack s around the reference: a kernel value g passes iff lo - s <= g <= hi + s
    fbank_twin32    the kernel's algorithm in float32 numpy (radix-2 FFT with a twiddle table, mel bin by bin), with named mutants
    resample_ref64  resample_sample in float64 with the bound of its fma chain
    cmvn_ref64      (x - mean) / std

The interval.  A float32 FFT of a frame x has a forward error proportional to the frame's norm, not to the bin it lands in:
|X_f32[k] - X[k]| <= delta = C_FFT * 2^-24 * ||x||_2 for every k.  The power of a bin is then off by at most 2 |X[k]| delta + delta^2,
a mel energy m by at most E = melw @ (2 |X| delta + delta^2), and the log-mel value lies in [log(max(m - E, floor)), log(max(m + E,
floor))].  The slack s = 8 * 2^-24 * max(1, |log m|) covers the roundings after the spectrum (the power, the mel sum's 257 fmas of
non-negative terms -- relative, so small next to E wherever E matters -- logf, and the two roundings of the CMVN line).  Where a mel bin
holds real energy the interval is a few 1e-5 wide; where the bin lies below the float32 noise of its frame (tonal inputs, a DC
offset, silence) it opens by itself down to the floor, with no list of exceptions.

C_FFT is measured, never chosen and never calibrated on GPU output: twice the worst max_k |X_twin - X_ref64| / (2^-24 ||x||_2) of the
twin over cases(), rounded up (measure_c_fft; tests/test_frontend_ref_cpu.py checks the constant against a fresh measurement).  The
factor 2 is for what the kernel does and the twin does not: sincospif twiddles, fma contraction, wave-order sums.
"""
import math

import numpy as np

WIN, SHIFT, NFFT, NBIN, NMEL = 400, 160, 512, 257, 80
FLOOR = 1.1920928955078125e-07          # the kernel's log floor, float32 eps
PREEMPH = np.float32(0.97)              # the kernel's 0.97f
U = 2.0 ** -24                          # float32 unit roundoff

# measure_c_fft() on the committed twin: worst ratio 13.29 (case "alternating"; 11.53 on noise_ragged, the worst noise case)
TWIN_WORST = 13.29
C_FFT = 27                              # ceil(2 * 13.29)

MUTANTS = ("mel_edge_lo", "mel_edge_hi", "window_400", "mean_512")


def tables():
    """(window [400], melw [80, 257]) float32: the arrays streamspeech_amd.weights packs into the weight blob for the kernel."""
    from streamspeech_amd import weights
    return weights.povey_window().numpy(), weights.mel_banks().numpy()


def num_frames(n):
    return 0 if n < WIN else 1 + (n - WIN) // SHIFT


def frames_of(x):
    """[n] -> [T, 400], snip_edges."""
    T = num_frames(len(x))
    return x[np.arange(T)[:, None] * SHIFT + np.arange(WIN)[None, :]] if T else np.zeros((0, WIN), x.dtype)


# ---- the float64 statement --------------------------------------------------------------------------------------------------------
def fbank_ref64(pcm_f32, pcm_scale=32768.0):
    """fbank_row in float64: frame (snip_edges), * scale, - the 400-sample mean, pre-emphasis with replicate padding, window,
    zero-pad to 512, rfft, power, mel.  -> dict: m [T, 80] mel energies (before floor and log), X [T, 257] complex spectrum,
    absX = |X|, norm [T] = ||x||_2 of the scaled frame before DC removal."""
    pcm = np.asarray(pcm_f32)
    assert pcm.dtype == np.float32 and pcm.ndim == 1
    window, melw = tables()
    fr = frames_of(pcm.astype(np.float64)) * float(np.float32(pcm_scale))
    norm = np.sqrt((fr * fr).sum(axis=1))
    d = fr - fr.mean(axis=1, keepdims=True)
    prev = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
    y = (d - float(PREEMPH) * prev) * window.astype(np.float64)[None, :]
    X = np.fft.rfft(np.pad(y, ((0, 0), (0, NFFT - WIN))), axis=1)
    power = X.real ** 2 + X.imag ** 2
    return {"m": power @ melw.astype(np.float64).T, "X": X, "absX": np.abs(X), "norm": norm}


def logmel64(ref):
    return np.log(np.maximum(ref["m"], FLOOR))


def fbank_bounds(ref, c_fft=C_FFT, mean=None, std=None):
    """-> (lo, hi, s, mid), each [T, 80] float64 (see the module docstring; mid is the reference's own value, log(max(m, floor))); with
    CMVN vectors lo, hi and mid go through (v - mean) / std and s is scaled by 1 / std."""
    _, melw = tables()
    delta = (c_fft * U * ref["norm"])[:, None]
    E = (2.0 * ref["absX"] * delta + delta * delta) @ melw.astype(np.float64).T
    lo = np.log(np.maximum(ref["m"] - E, FLOOR))
    hi = np.log(np.maximum(ref["m"] + E, FLOOR))
    mid = logmel64(ref)
    s = 8.0 * U * np.maximum(1.0, np.abs(mid))
    if mean is not None:
        mean, std = np.asarray(mean, np.float32).astype(np.float64), np.asarray(std, np.float32).astype(np.float64)
        lo, hi, mid, s = (lo - mean) / std, (hi - mean) / std, (mid - mean) / std, s / std
    return lo, hi, s, mid


def outside(g, bounds):
    """Boolean [T, 80]: where the values g leave their interval (NaN and inf are outside)."""
    lo, hi, s, _ = bounds
    g = np.asarray(g, np.float64)
    return ~((g >= lo - s) & (g <= hi + s))


def excess(g, bounds):
    """The error of g against the reference's value as a fraction of the room the interval leaves on that side (slack included):
    <= 1 inside, NaN or inf for a value that is neither."""
    lo, hi, s, mid = bounds
    g = np.asarray(g, np.float64)
    return np.where(g >= mid, (g - mid) / (hi + s - mid), (mid - g) / (mid - (lo - s)))


# ---- the float32 twin -------------------------------------------------------------------------------------------------------------
def _bitrev9():
    i = np.arange(NFFT)
    r = np.zeros(NFFT, np.int64)
    for b in range(9):
        r |= ((i >> b) & 1) << (8 - b)
    return r


def _mutate_tables(window, melw, mutant):
    if mutant in ("mel_edge_lo", "mel_edge_hi"):
        melw = melw.copy()
        for r in range(NMEL):
            nz = np.flatnonzero(melw[r])
            melw[r, nz[0] if mutant == "mel_edge_lo" else nz[-1]] = 0.0
    if mutant == "window_400":
        i = np.arange(WIN, dtype=np.float64)
        window = ((0.5 - 0.5 * np.cos(2 * math.pi * i / WIN)) ** 0.85).astype(np.float32)
    return window, melw


def mutant_tables(mutant):
    """The tables a mutant of the twin computes with (for a by-hand run of the GPU tests on a mutated weight blob)."""
    assert mutant in ("mel_edge_lo", "mel_edge_hi", "window_400")
    return _mutate_tables(*tables(), mutant)


def fbank_twin32(pcm, pcm_scale=32768.0, mutant=None, spectrum=False):
    """The kernel's algorithm, every operation rounded to float32: frame mean over 400, pre-emphasis, window, bit-reversed load, nine
    radix-2 stages with a 256-entry float32 twiddle table, power, the mel sum accumulated bin by bin, log(max(., floor)).
    -> log-mel [T, 80] float32 (with spectrum=True also the complex128 copy of its float32 spectrum [T, 257])."""
    assert mutant is None or mutant in MUTANTS
    f32 = np.float32
    window, melw = _mutate_tables(*tables(), mutant)
    fr = frames_of(np.asarray(pcm, f32)) * f32(pcm_scale)
    T = fr.shape[0]
    mean = fr.sum(axis=1, keepdims=True, dtype=f32) / f32(NFFT if mutant == "mean_512" else WIN)
    d = fr - mean
    prev = np.concatenate([d[:, :1], d[:, :-1]], axis=1)
    y = (d - PREEMPH * prev) * window[None, :]
    re = np.zeros((T, NFFT), f32)
    im = np.zeros((T, NFFT), f32)
    re[:, _bitrev9()[:WIN]] = y
    k = np.arange(NFFT // 2, dtype=np.float64)
    tw_c, tw_s = np.cos(-2 * math.pi * k / NFFT).astype(f32), np.sin(-2 * math.pi * k / NFFT).astype(f32)
    t = np.arange(NFFT // 2)
    for stg in range(9):
        half = 1 << stg
        pos = t & (half - 1)
        i0 = ((t >> stg) << (stg + 1)) + pos
        i1 = i0 + half
        c, sn = tw_c[pos << (8 - stg)][None, :], tw_s[pos << (8 - stg)][None, :]
        br = re[:, i1] * c - im[:, i1] * sn
        bi = re[:, i1] * sn + im[:, i1] * c
        ar, ai = re[:, i0], im[:, i0]
        re[:, i0], im[:, i0], re[:, i1], im[:, i1] = ar + br, ai + bi, ar - br, ai - bi
    assert re.dtype == f32 and im.dtype == f32
    power = re[:, :NBIN] * re[:, :NBIN] + im[:, :NBIN] * im[:, :NBIN]
    e = np.zeros((T, NMEL), f32)
    for i in range(NBIN):
        e = e + melw[None, :, i] * power[:, i:i + 1]
    lg = np.log(np.maximum(e, f32(FLOOR)))
    assert lg.dtype == f32
    if spectrum:
        return lg, re[:, :NBIN].astype(np.float64) + 1j * im[:, :NBIN].astype(np.float64)
    return lg


def cmvn32(lg, mean, std):
    """The kernel's last line in float32."""
    return (np.asarray(lg, np.float32) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)


def twin_fft_ratio(pcm, pcm_scale=32768.0):
    """max over frames and bins of |X_twin - X_ref64| / (2^-24 ||x||_2); 0 where every frame is silent."""
    ref = fbank_ref64(pcm, pcm_scale)
    _, X = fbank_twin32(pcm, pcm_scale, spectrum=True)
    err = np.abs(X - ref["X"]).max(axis=1)
    ok = ref["norm"] > 0
    assert (err[~ok] == 0).all()
    return float((err[ok] / (U * ref["norm"][ok])).max()) if ok.any() else 0.0


def measure_c_fft():
    """-> ({case: ratio}, the worst ratio): what TWIN_WORST and C_FFT = ceil(2 * worst) are written down from."""
    r = {name: twin_fft_ratio(x) for name, (x, _) in cases().items()}
    return r, max(r.values())


# ---- the cases --------------------------------------------------------------------------------------------------------------------
_CASES = None


def cases():
    """{name: (float32 waveform in [-1, 1], tight)} -- the one list of the CPU and the GPU tests.  tight: every mel bin of every frame
    holds energy above the frame's float32 noise, so the share of wide intervals is capped; the others are held to their intervals
    and their share of wide ones is reported."""
    global _CASES
    if _CASES is None:
        from oracle import make_golden_fbank as MG
        from streamspeech_amd import synth
        c = {name: (MG.waveform(*spec), name != "tonal_2s") for name, spec in MG.CASES.items()}
        n = 16000
        t = np.arange(n) / 16000.0
        imp = np.zeros(n, np.float32)
        imp[::157] = 0.9
        c["impulse_train"] = (imp, True)
        c["dc_offset"] = ((0.5 + 0.01 * synth.normal(21, "frontend_ref/dc", (n,), 1.0)).astype(np.float32), False)
        c["sine_full"] = ((0.999 * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32), False)
        c["square_440"] = ((0.99 * np.sign(np.sin(2 * np.pi * 440.0 * t + 0.1))).astype(np.float32), False)
        c["alternating"] = ((0.5 * (1.0 - 2.0 * (np.arange(n) % 2))).astype(np.float32), False)
        c["zeros"] = (np.zeros(n, np.float32), False)
        c["constant"] = (np.full(n, 0.25, np.float32), False)
        for x, _ in c.values():
            x.setflags(write=False)
        _CASES = c
    return _CASES


FLOOR_CASES = ("zeros", "constant")     # every value is log(floor) before CMVN


# ---- resampler and CMVN -----------------------------------------------------------------------------------------------------------
def resample_ref64(x_f32, up, down, taps_f32, half, n_out):
    """y[k] = sum_m x[m] h[half + k down - m up] in float64 over the clamped window of resample_sample (csrc/fbank.hpp): m from
    max(0, ceil((k down - half) / up)) to min(n_in - 1, (k down + half) / up), zeros outside the history.
    -> (y [n_out], bound [n_out]): bound[k] = n_k * 2^-24 * sum_m |x[m] h[.]| with n_k the number of terms, the bound of a chain of
    n_k fmas (every product exact, one rounding per addition)."""
    x = np.asarray(x_f32)
    h = np.asarray(taps_f32)
    assert x.dtype == np.float32 and h.dtype == np.float32 and len(h) == 2 * half + 1
    n_in = len(x)
    c = np.arange(n_out, dtype=np.int64) * down
    m_lo = np.maximum(0, -(-(c - half) // up))
    m_hi = np.minimum(n_in - 1, (c + half) // up)
    width = 2 * half // up + 1
    m = m_lo[:, None] + np.arange(width, dtype=np.int64)[None, :]
    ok = m <= m_hi[:, None]
    mc = np.where(ok, m, 0)
    tap = np.where(ok, half + c[:, None] - mc * up, 0)
    assert ((tap >= 0) & (tap <= 2 * half)).all()
    prod = np.where(ok, x.astype(np.float64)[mc] * h.astype(np.float64)[tap], 0.0) if n_in else np.zeros((n_out, width))
    n_k = ok.sum(axis=1)
    return prod.sum(axis=1), n_k * U * np.abs(prod).sum(axis=1)


def cmvn_ref64(rows, mean, std):
    return (np.asarray(rows, np.float32).astype(np.float64) - np.asarray(mean, np.float32).astype(np.float64)) \
        / np.asarray(std, np.float32).astype(np.float64)
