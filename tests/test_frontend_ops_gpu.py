"""Op-level tests of the kernels of csrc/fbank.hip -- fbank_cmvn_kernel in its single, packed and per-pointer forms, fbank_cmvn_sr_kernel,
cmvn_rows_kernel and resample_kernel -- form by form against tests/frontend_ref.py (float64), through ss_fbank_cmvn, ss_batch_fbank_cmvn,
ss_batch_fbank_frames, ss_batch_fbank_frames_sr, ss_resample and ss_batch_cmvn.

The bound of an fbank value is no flat tolerance but the interval of frontend_ref.fbank_bounds (the forward error of a float32 FFT carried
through power, mel and log, with the constant measured on the host); a resampled sample has the derived bound of its fma chain; a CMVN value
2 ulp.  The harness is that of tests/test_slab_ops_gpu.py and tests/test_gemm_routes_gpu.py.  Every launch of this file:
  * reads PCM (taps, rows) that sit in a larger device buffer with 1e30 directly before the first and after the last element, so a read
    outside lands far outside every bound (1e30 * 32768 is inf);
  * writes into an output that starts as NaN with guard rows behind it; afterwards the rows the call is defined to write are finite and
    everything else is still NaN.
The worst error of every form as a fraction of its bound is printed as a WORST line when the module ends, the share of wide intervals of
every case as a SHARE line; profiles/frontend_accuracy.txt holds those of a run.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import frontend_ref as FR
from test_slab_ops_gpu import P, S, bits, census, lib, stop_after_a_gpu_error, took_since  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EDGE = 1.0e30                  # what lies directly before and after every input
GUARD = 64                     # guard elements on either side of an input
GROWS = 4                      # guard rows of NaN behind an output
SS_ERR_ARG = 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORM_WORST = {}                # form -> [worst error / bound, values checked]


def book(form, frac, n):
    tot = FORM_WORST.setdefault(form, [0.0, 0])
    tot[0], tot[1] = max(tot[0], float(frac)), tot[1] + int(n)


@pytest.fixture(scope="module", autouse=True)
def worst_table():
    yield
    print()
    for name, (x, tight) in FR.cases().items():
        lo, hi, _, _ = FR.fbank_bounds(FR.fbank_ref64(x))
        print(f"SHARE {name}: {100 * float(((hi - lo) > 1e-3).mean()):.2f} % of the intervals wider than 1e-3, median width "
              f"{float(np.median(hi - lo)):.2e} ({'tight, capped at 1 %' if tight else 'reported'})")
    for form, (frac, n) in FORM_WORST.items():
        print(f"WORST {form}: {frac:.3f} of the bound over {n} values")


@pytest.fixture(scope="module")
def stats():
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    return g["mean"].astype(np.float32), g["std"].astype(np.float32)


@pytest.fixture(scope="module")
def plain_model(synth_weights):
    """The synthetic checkpoint WITHOUT CMVN statistics: its fbank rows are the raw log-mel values, (lg - 0) / 1."""
    from streamspeech_amd.engine import HipModel
    cfg, _, sd, _ = synth_weights
    return HipModel(sd, cfg)


# ---- the harness --------------------------------------------------------------------------------------------------------------------
def guarded(x):
    """A 1-d float32 array -> (the whole device buffer, the view of x inside it): EDGE directly before x[0] and after x[-1]."""
    x = torch.from_numpy(np.array(x, dtype=np.float32)).reshape(-1)          # (a copy: the cases are read-only arrays)
    buf = torch.full((x.numel() + 2 * GUARD,), EDGE, device=DEV)
    buf[GUARD:GUARD + x.numel()] = x.to(DEV)
    return buf, buf[GUARD:GUARD + x.numel()]


def out_rows(T, cols=80):
    """NaN [T + GROWS, cols] on the device; the call gets the first T rows."""
    return torch.full((T + GROWS, cols), float("nan"), device=DEV)


def written_exactly(out, T, what):
    """The host copy of the first T rows, after checking that they are finite and that the guard rows behind them are still NaN."""
    host = out.cpu()
    assert torch.isfinite(host[:T]).all(), f"{what}: not finite where the op writes"
    assert torch.isnan(host[T:]).all(), f"{what}: rows behind the op's own were written"
    return host[:T]


_FORM1 = {}


def form1(model, x, scale=32768.0, key=None):
    """ss_fbank_cmvn on the samples x alone, in the harness -> host float32 [T, 80].  Cached by key (a name of x)."""
    if key is not None and key in _FORM1:
        return _FORM1[key]
    T = FR.num_frames(len(x))
    keep, view = guarded(x)
    out = out_rows(T)
    nf = C.c_int(-1)
    rc = model.lib.ss_fbank_cmvn(model.h, S(), P(view), len(x), scale, P(out), C.byref(nf))
    torch.cuda.synchronize()
    assert rc == 0 and nf.value == T, (key, rc, nf.value)
    got = written_exactly(out, T, f"ss_fbank_cmvn {key}")
    del keep
    if key is not None:
        _FORM1[key] = got
    return got


def hold(form, what, got, x, stats, scale=32768.0):
    """The rows `got` of the fbank of the float32 samples x against fbank_bounds with the model's CMVN vectors."""
    bounds = FR.fbank_bounds(FR.fbank_ref64(x, scale), mean=stats[0], std=stats[1])
    g = got.numpy() if isinstance(got, torch.Tensor) else got
    assert g.shape == bounds[0].shape, (what, g.shape, bounds[0].shape)
    if g.size == 0:
        return
    frac = FR.excess(g, bounds)
    bad = FR.outside(g, bounds)
    print(f"{form} | {what}: worst {np.nanmax(frac):.3f} of the interval, {int(bad.sum())} of {g.size} outside")
    assert not bad.any(), f"{what}: {int(bad.sum())} of {g.size} values outside their interval, the worst at {np.nanmax(frac):.2f} of it"
    book(form, frac.max(), g.size)


# ---- 1. ss_fbank_cmvn ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FR.cases()))
def test_fbank_cmvn_every_case(hip_model, stats, name):
    x, _ = FR.cases()[name]
    got = form1(hip_model, x, key=name)
    hold("ss_fbank_cmvn", name, got, x, stats)
    if name in FR.FLOOR_CASES:           # silence and a constant: every value is the floor's, finite, never NaN or -inf
        want = (np.log(np.float32(FR.FLOOR)) - stats[0]) / stats[1]
        assert np.abs(got.numpy() - want[None, :]).max() <= 8 * FR.U * 16 / stats[1].min()


@pytest.mark.parametrize("n", [399, 400, 559, 560, 48017])
def test_fbank_cmvn_sample_counts(hip_model, stats, n):
    """Frame counts at the snip_edges steps: 399 samples give no frame and nothing is written, 400 and 559 one, 560 two."""
    x = FR.cases()["noise_ragged"][0][48017 - n:]          # the last n samples: another alignment than the case itself
    got = form1(hip_model, x, key=("tail", n))
    assert got.shape[0] == {399: 0, 400: 1, 559: 1, 560: 2, 48017: 298}[n]
    hold("ss_fbank_cmvn", f"{n} samples", got, x, stats)


def test_fbank_cmvn_scale_one_and_repeat(hip_model, stats):
    """pcm_scale = 1 on samples that carry the 2^15 already: the same intervals (and, the scale being a power of two, the same bits);
    two runs of one input are bitwise equal."""
    x = FR.cases()["noise_ragged"][0]
    a = form1(hip_model, x, key="noise_ragged")
    b = form1(hip_model, x)
    assert torch.equal(bits(a), bits(b))
    x1 = (x * np.float32(32768.0)).astype(np.float32)
    c = form1(hip_model, x1, scale=1.0)
    hold("ss_fbank_cmvn", "pcm_scale 1 on scaled samples", c, x1, stats, scale=1.0)
    hold("ss_fbank_cmvn", "pcm_scale 1 against the unscaled reference", c, x, stats)
    assert torch.equal(bits(a), bits(c))


# ---- 2. ss_batch_fbank_cmvn ---------------------------------------------------------------------------------------------------------
def packed(utts, gap=8):
    """Utterances laid out one after another in ONE guarded buffer, `gap` elements of EDGE between neighbours -> (buffer, pointer to
    element 0 of the first, start offsets)."""
    starts, off = [], 0
    for u in utts:
        starts.append(off)
        off += len(u) + gap
    flat = np.full(off, EDGE, np.float32)
    for s, u in zip(starts, utts):
        flat[s:s + len(u)] = u
    keep, view = guarded(flat)
    return keep, view, starts


def batch_fbank(model, view, starts, ns, out, scale=32768.0, hT=None):
    B = len(ns)
    hT = (C.c_int32 * B)(*([-7] * B)) if hT is None else hT
    rc = model.lib.ss_batch_fbank_cmvn(model.h, S(), B, P(view), (C.c_int64 * B)(*starts), (C.c_int32 * B)(*ns), scale, P(out), hT)
    torch.cuda.synchronize()
    return rc, list(hT)


PACK = [("noise_1s", 16000), ("dc_offset", 399), ("one_frame", 400), ("noise_ragged", 48017), ("quiet_1s", 559), ("sine_full", 160),
        ("impulse_train", 560), ("noise_short", 4000), ("tonal_2s", 7777)]


def test_batch_fbank_cmvn_pack(hip_model, stats):
    """Nine utterances of 160 .. 48017 samples, two of them too short for a frame, laid out in memory in another order than the
    batch's: every utterance's rows are the bits of ss_fbank_cmvn on it alone, the pack is inside its intervals, an utterance without
    frames gets h_T = 0 and no row."""
    utts = [FR.cases()[name][0][:n] for name, n in PACK]
    order = [4, 0, 8, 2, 6, 1, 7, 3, 5]                      # memory order of the batch's utterances
    keep, view, mem_starts = packed([utts[i] for i in order])
    starts = [0] * len(utts)
    for pos, i in enumerate(order):
        starts[i] = mem_starts[pos]
    ns = [len(u) for u in utts]
    T = [FR.num_frames(n) for n in ns]
    assert T.count(0) == 2 and max(T) == 298 and min(t for t in T if t) == 1
    out = out_rows(sum(T))
    rc, hT = batch_fbank(hip_model, view, starts, ns, out)
    assert rc == 0 and hT == T
    got = written_exactly(out, sum(T), "ss_batch_fbank_cmvn")
    row = 0
    for (name, n), u, t in zip(PACK, utts, T):
        alone = form1(hip_model, u, key=(name, n))
        assert torch.equal(bits(got[row:row + t]), bits(alone)), f"{name}[:{n}]: rows differ from ss_fbank_cmvn on the utterance alone"
        hold("ss_batch_fbank_cmvn", f"{name}[:{n}]", got[row:row + t], u, stats)
        row += t
    del keep


# ---- D. ss_batch_fbank_cmvn: refusals, and a pack past the grid's y extent ----------------------------------------------------------
def test_batch_fbank_cmvn_refusals(hip_model, lib):
    """Every refusal is decided before the launch: SS_ERR_ARG, the NaN output and h_T stay as they were, no launch is counted.  None
    needs a large buffer -- a start of 2^31 or 161 utterances of 2^31 - 1 samples are refused before anything is read."""
    x = FR.cases()["noise_short"][0]
    keep, view = guarded(x)
    out = out_rows(FR.num_frames(len(x)))
    L = hip_model.lib
    i64, i32 = (lambda v: (C.c_int64 * len(v))(*v)), (lambda v: (C.c_int32 * len(v))(*v))
    big = 2 ** 31 - 1
    assert 160 * FR.num_frames(big) <= big < 161 * FR.num_frames(big)
    calls = {
        "B = 0": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 0, P(view), i64([0]), i32([4000]), 32768.0, P(out), hT),
        "null d_pcm": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 1, None, i64([0]), i32([4000]), 32768.0, P(out), hT),
        "null d_feat": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 1, P(view), i64([0]), i32([4000]), 32768.0, None, hT),
        "null h_pcm_start": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 1, P(view), None, i32([4000]), 32768.0, P(out), hT),
        "null h_n_samples": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 1, P(view), i64([0]), None, 32768.0, P(out), hT),
        "null h_T": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 1, P(view), i64([0]), i32([4000]), 32768.0, P(out), None),
        "negative h_n_samples": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 2, P(view), i64([0, 0]), i32([4000, -1]), 32768.0,
                                                                 P(out), hT),
        "negative h_pcm_start": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 2, P(view), i64([0, -1]), i32([400, 400]), 32768.0,
                                                                 P(out), hT),
        "h_pcm_start = 2^31": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 2, P(view), i64([0, 2 ** 31]), i32([400, 400]), 32768.0,
                                                               P(out), hT),
        "h_pcm_start = 2^31 of an utterance without frames": lambda hT: L.ss_batch_fbank_cmvn(
            hip_model.h, S(), 2, P(view), i64([0, 2 ** 31]), i32([400, 0]), 32768.0, P(out), hT),
        "rows past 2^31 - 1": lambda hT: L.ss_batch_fbank_cmvn(hip_model.h, S(), 161, P(view), i64([0] * 161), i32([big] * 161), 32768.0,
                                                               P(out), hT),
    }
    before = census(lib)
    for what, call in calls.items():
        hT = (C.c_int32 * 161)(*([-7] * 161))
        rc = call(hT)
        torch.cuda.synchronize()
        assert rc == SS_ERR_ARG, f"{what}: rc {rc}"
        assert list(hT) == [-7] * 161, f"{what}: a refused call wrote h_T"
        assert torch.isnan(out).all(), f"{what}: a refused call wrote rows"
    assert took_since(lib, before) == {}
    # the call the refusals were variations of is served
    rc, hT = batch_fbank(hip_model, view, [0], [4000], out)
    assert rc == 0 and hT == [23]
    assert torch.equal(bits(written_exactly(out, 23, "after the refusals")), bits(form1(hip_model, x, key="noise_short")))
    del keep


def test_batch_fbank_cmvn_past_65535_utterances(hip_model):
    """65536 + 3 one-frame utterances (the grid's y extent ends at 65535: the segment table goes out in two slices), cycling through 7
    waveforms: every row is the bits of ss_fbank_cmvn's row of its waveform, the rows behind the pack are untouched."""
    B, K = 65536 + 3, 7
    noise = FR.cases()["noise_ragged"][0]
    waves = np.stack([noise[1000 * k + 3:1000 * k + 403] for k in range(K)])
    want = torch.cat([form1(hip_model, waves[k], key=("wave", k)) for k in range(K)])            # [7, 80]
    which = torch.arange(B, device=DEV) % K
    pcm = torch.full((B * 400 + 2 * GUARD,), EDGE, device=DEV)
    pcm[GUARD:GUARD + B * 400] = torch.from_numpy(waves).to(DEV)[which].reshape(-1)
    out = out_rows(B)
    rc, hT = batch_fbank(hip_model, pcm[GUARD:], [400 * b for b in range(B)], [400] * B, out)
    assert rc == 0 and hT == [1] * B
    assert torch.isnan(out[B:]).all(), "rows behind the pack were written"
    same = (bits(out[:B]) == bits(want.to(DEV)[which])).all(dim=1)
    assert bool(same.all()), f"{int((~same).sum())} of {B} rows differ from the single call's, the first at utterance {int((~same).nonzero()[0])}"
    del pcm


# ---- 3. ss_batch_fbank_frames -------------------------------------------------------------------------------------------------------
def test_batch_fbank_frames(hip_model, stats):
    """Sessions in buffers of their own, some starting at a later frame, some asking for none: rows first .. first + n - 1 are the bits
    of ss_fbank_cmvn's, with EDGE directly after the last sample the last row reads, 160 (first + n - 1) + 399."""
    sess = [("noise_ragged", 0, 298), ("noise_1s", 37, 5), ("tonal_2s", 100, 0), ("quiet_1s", 97, 1), ("one_frame", 0, 1),
            ("noise_short", 3, 0), ("impulse_train", 1, 96)]
    keeps, hist, outs = [], [], []
    for name, first, n in sess:
        x = FR.cases()[name][0]
        keep, view = guarded(x[:160 * (first + n - 1) + 400] if n else x[:400])
        keeps.append(keep); hist.append(view); outs.append(out_rows(n))
    hip_model.batch_fbank_frames(hist, [s[1] for s in sess], [s[2] for s in sess], [o[:s[2]] for o, s in zip(outs, sess)])
    torch.cuda.synchronize()
    for (name, first, n), o in zip(sess, outs):
        got = written_exactly(o, n, f"ss_batch_fbank_frames {name}")
        x = FR.cases()[name][0]
        assert torch.equal(bits(got), bits(form1(hip_model, x, key=name)[first:first + n])), f"{name}: rows {first} .. differ from ss_fbank_cmvn's"
        if n:
            hold("ss_batch_fbank_frames", f"{name} rows {first} .. {first + n - 1}", got, x[160 * first:160 * (first + n - 1) + 400], stats)


# ---- 4. ss_batch_fbank_frames_sr ----------------------------------------------------------------------------------------------------
def test_batch_fbank_frames_sr(hip_model, stats):
    """Sessions at 48 kHz, 44.1 kHz, 8 kHz and 16 kHz (passed through, no taps) in one call, EDGE at pcm[-1] and pcm[n_in]: the rows are
    the bits of ss_fbank_cmvn over ss_resample of the same history, and -- without going through the kernel's own resampling -- inside
    fbank_bounds evaluated on the float32 samples ss_resample returned."""
    from streamspeech_amd import synth
    sess = [(48000, 24017, 0, None), (44100, 22050, 5, None), (8000, 4100, 0, None), (16000, 8013, 2, None), (48000, 24017, 3, 0)]
    keeps, hist, firsts, counts, outs, want = [], [], [], [], [], []
    for i, (sr, n_in, first, n) in enumerate(sess):
        keep, view = guarded(synth.synth_pcm(130 + i, n_in))
        rows = hip_model.fbank_sr_rows(n_in, sr)[0]
        n = rows - first if n is None else n
        assert rows > 40 and n >= 0
        y = hip_model.resample(view, sr)                        # 16 kHz samples, float32 on the device (a view of the history at 16 kHz)
        want.append((y.cpu().numpy(), rows))
        keeps.append(keep); hist.append(view); firsts.append(first); counts.append(n); outs.append(out_rows(n))
    hip_model.batch_fbank_frames_sr(hist, [s[1] for s in sess], [s[0] for s in sess], firsts, counts, [o[:n] for o, n in zip(outs, counts)])
    torch.cuda.synchronize()
    for (sr, n_in, _, _), first, n, o, (y, rows) in zip(sess, firsts, counts, outs, want):
        got = written_exactly(o, n, f"ss_batch_fbank_frames_sr {sr}")
        assert FR.num_frames(len(y)) == rows
        alone = form1(hip_model, y)
        assert torch.equal(bits(got), bits(alone[first:first + n])), f"{sr} Hz: rows differ from ss_fbank_cmvn(ss_resample(.))"
        if n:
            hold("ss_batch_fbank_frames_sr", f"{sr} Hz rows {first} .. {first + n - 1}", got, y[160 * first:160 * (first + n - 1) + 400], stats)


# ---- 5. ss_resample -----------------------------------------------------------------------------------------------------------------
RATES = [48000, 44100, 8000, 22050, 32000]


def resample_case(model, form, what, x, sr):
    """ss_resample of x (float32, at sr) in the harness against resample_ref64 and its bound -> (host result, taps, up, down, half)."""
    from streamspeech_amd.engine import resample_ratio
    from streamspeech_amd.frontend import design_filter
    up, down, half = resample_ratio(sr)
    taps = design_filter(up, down).astype(np.float32)
    n_in = len(x)
    n_out = -(-n_in * up // down)
    kx, vx = guarded(x)
    kt, vt = guarded(taps)
    out = out_rows(n_out, 1)
    rc = model.lib.ss_resample(S(), P(vx), n_in, up, down, P(vt), half, P(out), n_out)
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    got = written_exactly(out, n_out, what)[:, 0].numpy()
    y, bound = FR.resample_ref64(x, up, down, taps, half, n_out)
    err = np.abs(got.astype(np.float64) - y)
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} of {n_out} samples outside the bound, worst {np.max(err / np.maximum(bound, 1e-300)):.2f} of it"
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    edge = min(n_out, -(-half // down))                       # the outputs whose window is clamped, at either end
    ends = np.concatenate([frac[:edge], frac[n_out - edge:]])
    print(f"{form} | {what}: {n_in} -> {n_out} samples, worst {frac.max():.3f} of the bound, {ends.max():.3f} on the {edge} clamped at each end")
    book(form, frac.max(), n_out)
    book(form + ", clamped windows", ends.max(), len(ends))
    del kx, kt
    return got, taps, up, down, half


@pytest.mark.parametrize("sr", RATES)
def test_resample_lengths(hip_model, sr):
    """1, 2, half / up, 255, 256 and 257 output samples (a block is 256: the last is a second block of one thread) and 3 s."""
    from streamspeech_amd import synth
    from streamspeech_amd.engine import resample_ratio
    up, down, half = resample_ratio(sr)
    x = synth.synth_pcm(140, 3 * sr)
    seen = set()
    for t in (1, 2, max(1, half // up), 255, 256, 257):
        n_in = max(1, t * down // up if down > up else -(-t * down // up))
        got = resample_case(hip_model, "ss_resample", f"{sr} Hz, {n_in} in", x[:n_in], sr)[0]
        seen.add(len(got))
    assert {256, 257} & seen and min(seen) <= 2, seen
    resample_case(hip_model, "ss_resample", f"{sr} Hz, 3 s", x, sr)


@pytest.mark.parametrize("sr", RATES)
def test_resample_impulses_return_the_taps(hip_model, sr):
    """An impulse at sample 0 and one at sample n_in - 1: y[k] is the tap half + k down - m up wherever that is a tap, 0 elsewhere."""
    n_in = 700
    for m in (0, n_in - 1):
        x = np.zeros(n_in, np.float32)
        x[m] = 1.0
        got, taps, up, down, half = resample_case(hip_model, "ss_resample", f"{sr} Hz, impulse at {m}", x, sr)
        idx = half + np.arange(len(got), dtype=np.int64) * down - m * up
        ok = (idx >= 0) & (idx <= 2 * half)
        assert ok.sum() >= half // down - 1                 # one side of the table: the other lies outside the output
        want = np.where(ok, taps[np.clip(idx, 0, 2 * half)], np.float32(0.0))
        assert np.abs(got - want).max() <= FR.U * np.abs(taps).max() and (got[~ok] == 0).all()


# ---- 6. ss_batch_cmvn ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [0, 1, 3, 4, 1000])
def test_batch_cmvn_rows(hip_model, stats, rows):
    """(x - mean) / std within 2 ulp of float64, out of place and in place (a 256-thread block covers 3.2 rows)."""
    rng = np.random.default_rng(rows)
    x = (rng.standard_normal((rows, 80)) * 6.0 + 4.0).astype(np.float32)
    if rows:
        x[0, :3] = [np.log(np.float32(FR.FLOOR)), 0.0, 25.0]
    ref = FR.cmvn_ref64(x, *stats)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    keep, view = guarded(x)
    out = out_rows(rows)
    rc = hip_model.lib.ss_batch_cmvn(hip_model.h, S(), P(view), rows, P(out))
    torch.cuda.synchronize()
    assert rc == 0
    got = written_exactly(out, rows, f"ss_batch_cmvn {rows} rows")
    rc = hip_model.lib.ss_batch_cmvn(hip_model.h, S(), P(view), rows, P(view))              # d_out == d_in
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(bits(view.cpu().reshape(rows, 80)), bits(got)), "in place differs from out of place"
    assert bool((keep[:GUARD] == EDGE).all()) and bool((keep[GUARD + rows * 80:] == EDGE).all()), "in place wrote outside its rows"
    if rows:
        frac = np.abs(got.numpy().astype(np.float64) - ref) / (2 * ulp)
        print(f"ss_batch_cmvn | {rows} rows: worst {frac.max():.3f} of 2 ulp")
        assert frac.max() <= 1.0
        book("ss_batch_cmvn", frac.max(), ref.size)


def test_batch_cmvn_of_raw_rows_is_the_fused_kernel(hip_model, plain_model, stats):
    """The header's promise, "written exactly as the last line of the fbank kernel": the raw log-mel rows of a model packed without
    stats (mean 0, std 1), through ss_batch_cmvn of the model with stats, are the bits of that model's ss_fbank_cmvn -- and the raw
    rows themselves sit inside the intervals without CMVN."""
    for name in ("noise_short", "tonal_2s", "zeros"):
        x = FR.cases()[name][0]
        raw = form1(plain_model, x)
        T = raw.shape[0]
        hold("ss_fbank_cmvn, no stats", name, raw, x, (np.zeros(80, np.float32), np.ones(80, np.float32)))
        keep, view = guarded(raw.numpy())
        out = out_rows(T)
        assert hip_model.lib.ss_batch_cmvn(hip_model.h, S(), P(view), T, P(out)) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits(written_exactly(out, T, name)), bits(form1(hip_model, x, key=name)))
        del keep
