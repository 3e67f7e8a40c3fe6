"""ss_fbank_mel_ranges (host only; the library loads without a GPU): the non-zero bin range of every mel row, which a new model computes
once so that the fbank kernel walks bins [lo, hi) of a row only.  On the product's matrix weights.mel_banks() ([80][257]) every
non-zero must lie inside its row's range -- that is what keeps the kernel's sums bit-identical -- and the ranges are tight: each row is
one contiguous run, 501 non-zeros in all, the widest row 16 bins.  Hand-made rows pin the edges.
"""
import ctypes as C

import numpy as np
import pytest

from streamspeech_amd import lib as L
from streamspeech_amd import weights


@pytest.fixture(scope="module")
def lib():
    return L.load()


def ranges(lib, w):
    w = np.ascontiguousarray(w, np.float32)
    out = (C.c_int32 * (2 * w.shape[0]))()
    assert lib.ss_fbank_mel_ranges(w.ctypes.data, w.shape[0], w.shape[1], out) == 0
    return np.array(out, np.int64).reshape(w.shape[0], 2)


def test_mel_banks_ranges(lib):
    w = np.asarray(weights.mel_banks(), np.float32)
    assert w.shape == (80, 257)
    r = ranges(lib, w)
    lo, hi = r[:, 0], r[:, 1]
    assert (0 <= lo).all() and (lo < hi).all() and (hi <= 257).all()            # no empty row
    inside = (np.arange(257)[None, :] >= lo[:, None]) & (np.arange(257)[None, :] < hi[:, None])
    assert not (w[~inside] != 0).any(), "a non-zero weight outside its row's range"
    assert (w[inside] != 0).all(), "an interior zero: the rows are contiguous runs"
    assert not (w < 0).any()
    width = hi - lo
    assert int(width.sum()) == 501 == int((w != 0).sum())
    assert int(width.max()) == 16 and int(width.min()) == 1


def test_hand_made_rows(lib):
    w = np.zeros((7, 257), np.float32)
    w[0, 5:9] = 1.0                     # leading and trailing zeros
    w[1, 0:3] = 2.0                     # no leading zeros
    w[2, 250:257] = 3.0                 # no trailing zeros
    # row 3: all zeros
    w[4, 0] = 1e-30                     # a single non-zero at index 0
    w[5, 256] = -1.0                    # a single non-zero at the last index
    w[6, 10] = 1.0; w[6, 20] = 1.0      # interior zeros stay inside the range
    assert ranges(lib, w).tolist() == [[5, 9], [0, 3], [250, 257], [0, 0], [0, 1], [256, 257], [10, 21]]


def test_shapes_and_refusals(lib):
    assert ranges(lib, np.ones((2, 1), np.float32)).tolist() == [[0, 1], [0, 1]]
    assert ranges(lib, np.zeros((3, 0), np.float32)).tolist() == [[0, 0]] * 3
    out = (C.c_int32 * 2)()
    one = np.ones((1, 4), np.float32)
    assert lib.ss_fbank_mel_ranges(None, 1, 4, out) == L.SS_ERR_ARG
    assert lib.ss_fbank_mel_ranges(one.ctypes.data, 1, 4, None) == L.SS_ERR_ARG
    assert lib.ss_fbank_mel_ranges(one.ctypes.data, -1, 4, out) == L.SS_ERR_ARG
    assert lib.ss_fbank_mel_ranges(one.ctypes.data, 1, -4, out) == L.SS_ERR_ARG
