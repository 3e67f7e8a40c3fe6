"""The incremental front-end for sources at any sample rate, on the host: the two C-ABI additions are exported and prototyped, and
ss_fbank_sr_rows -- where the Python layer reads which fbank rows of a growing source-rate history are final -- against a brute-force
index model of the resampler's zero-padded edge, with the refusals it shares with ss_batch_fbank_frames_sr.  (The library loads without
a GPU; the entry point's own refusals need a model handle and are a GPU test, tests/test_frontend_sr_gpu.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (48000, 44100, 32000, 24000, 22050, 11025, 8000)


def _lib():
    from streamspeech_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _rows(lib, n_in, up, down, half):
    rows, fin = C.c_int32(-1), C.c_int32(-1)
    rc = lib.ss_fbank_sr_rows(n_in, up, down, half, C.byref(rows), C.byref(fin))
    return rc, rows.value, fin.value


def test_exported_and_prototyped():
    from streamspeech_amd import lib as L
    header = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    lib = _lib()
    for name, args in (("ss_batch_fbank_frames_sr", 13), ("ss_fbank_sr_rows", 6)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == args, name
        assert hasattr(lib, name)
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", header) and lib.ss_abi_version() == 2


@pytest.mark.parametrize("sr", RATES)
def test_rows_and_final_rows_against_the_index_model(sr):
    """16-kHz sample k is settled iff the last input of its FIR window exists, (k * down + half) // up <= n_in - 1; a row is final iff
    its last sample 160 f + 399 is.  Identical counts for growing histories (every sample count up to ~0.2 s, then the agent's 160-,
    320- and 640-ms segment boundaries and odd strides up to 12 s); the final count never goes back; the rows still open are within
    what frontend.unsettled_fbank_frames tells the encoder."""
    from streamspeech_amd.engine import resample_ratio
    from streamspeech_amd.frontend import design_filter, unsettled_fbank_frames
    lib = _lib()
    up, down, half = resample_ratio(sr)
    assert half == (len(design_filter(up, down)) - 1) // 2
    counts = set(range(0, sr // 5))
    for ms in (160, 320, 640):
        counts |= set(range(0, 12 * sr + 1, sr * ms // 1000))
    counts |= set(range(0, 12 * sr, 7919))
    tail, prev = unsettled_fbank_frames(sr), 0
    k = np.arange(12 * 16000 + 1, dtype=np.int64)
    last_in = (k * down + half) // up                    # the kernel's m_hi before its clamp
    for n_in in sorted(counts):
        n16 = -(-n_in * up // down)
        rows = 0 if n16 < 400 else 1 + (n16 - 400) // 160
        settled = last_in[:n16] <= n_in - 1
        fin = 0
        while fin < rows and settled[160 * fin + 399]:
            fin += 1
        assert not settled[1:][~settled[:-1]].any()          # the settled samples are a prefix, so are the final rows
        assert _rows(lib, n_in, up, down, half) == (0, rows, fin), (sr, n_in)
        assert fin >= prev and rows - fin <= tail, (sr, n_in, rows, fin, prev)
        prev = fin


def test_pass_through_rows_are_all_final():
    lib = _lib()
    for n_in in (0, 399, 400, 559, 560, 16000, 123457):
        rows = 0 if n_in < 400 else 1 + (n_in - 400) // 160
        assert _rows(lib, n_in, 1, 1, 0) == (0, rows, rows)


def test_refusals_about_a_ratio():
    """What ss_batch_fbank_frames_sr refuses about a ratio (the same code): up or down below 1, a negative half_len, taps that do not
    fit the 64 KB of a workgroup beside the row's 6160 bytes (2 * half_len + 1 floats)."""
    from streamspeech_amd import lib as L
    lib = _lib()
    ok = (1000, 1, 3, 30)
    assert _rows(lib, *ok)[0] == 0
    for bad in ((1000, 0, 3, 30), (1000, -1, 3, 30), (1000, 1, 0, 30), (1000, 1, -2, 30), (1000, 1, 3, -1), (-1, 1, 3, 30)):
        rc, rows, fin = _rows(lib, *bad)
        assert rc == L.SS_ERR_ARG and (rows, fin) == (-1, -1), bad            # nothing written on a refusal
    fit = ((65536 - 6160) // 4 - 1) // 2                                       # the most taps on either side that fit
    assert _rows(lib, 100000, 1, fit // 10, fit)[0] == 0
    assert _rows(lib, 100000, 1, fit // 10, fit + 1)[0] == L.SS_ERR_ARG
    assert _rows(lib, 100000, 1, 800, 8000)[0] == L.SS_ERR_ARG                 # a 1:800 ratio's filter
    assert lib.ss_fbank_sr_rows(1000, 1, 3, 30, None, None) == 0               # either output may be left out


def test_every_rate_of_the_tests_fits():
    from streamspeech_amd.engine import fbank_sr_rows, resample_ratio
    for sr in RATES + (16000,):
        assert fbank_sr_rows(sr, *resample_ratio(sr), lib=_lib()) is not None, sr
    assert fbank_sr_rows(16000, 1, 800, 8000, lib=_lib()) is None              # the Python layer's sign to resample the old way
