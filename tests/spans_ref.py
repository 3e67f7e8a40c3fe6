"""Unit spans, restated in plain numpy and integers: which CTC units of a row of the unit decoder's arg-max belong to which
text-decoder state, and where their speech lies on the clock of the emitted frames (include/streamspeech_hip.h, "Unit spans").
The reference for ss_unit_spans_host, ss_op_unit_spans and ss_batch_unit_spans, plus the seeded rows the tests share."""
import numpy as np

BOS = 0
FRAME_MS = 20            # one vocoder frame: 320 samples at 16 kHz


def unit_mask(raw, blank, pad, bos, eos):
    """unit(f): raw[f] is none of {blank, pad, bos, eos} and starts a run of equal ids (f counts from the row's start)."""
    raw = np.asarray(raw, dtype=np.int64).reshape(-1)
    keep = (raw != blank) & (raw != pad) & (raw != bos) & (raw != eos)
    keep[1:] &= raw[1:] != raw[:-1]
    return keep


def unit_spans(raw, up, blank, pad, bos, eos, dur, d0=0, u0=0):
    """raw [up * n] arg-max ids of n states; dur[j - d0] the frames of unit ordinal j (j >= d0); u0 >= d0 the first NEW unit.
    -> (int32 [n, 4] = {first_unit, n_units, start_frame, n_frames} per state over the new units, K = all units of the row)."""
    raw = np.asarray(raw, dtype=np.int64).reshape(-1)
    up, d0, u0 = int(up), int(d0), int(u0)
    if up < 1 or raw.size == 0 or raw.size % up:
        raise ValueError("raw holds up * n ids, n >= 1")
    if not 0 <= d0 <= u0:
        raise ValueError("0 <= d0 <= u0")
    n = raw.size // up
    keep = unit_mask(raw, blank, pad, bos, eos)
    K = int(keep.sum())
    if u0 > K:
        raise ValueError("u0 > K")
    dur = np.asarray(dur, dtype=np.int64).reshape(-1)
    if dur.size < K - d0:
        raise ValueError("a duration per unit from d0 on")
    spans = np.zeros((n, 4), dtype=np.int64)
    ordinal, units, clock = 0, u0, 0
    frames = np.flatnonzero(keep)
    at = 0
    for s in range(n):
        spans[s, 0], spans[s, 2] = units, clock
        while at < frames.size and frames[at] // up == s:
            if ordinal >= u0:
                units += 1
                clock += int(dur[ordinal - d0])
            ordinal += 1
            at += 1
        spans[s, 1], spans[s, 3] = units - spans[s, 0], clock - spans[s, 2]
    return spans.astype(np.int32), K


def check_tiling(spans, u0, K, total_frames):
    """The spans of a row tile its new units and the emitted frames."""
    spans = np.asarray(spans, dtype=np.int64)
    assert spans[0, 0] == u0 and spans[0, 2] == 0
    assert (spans[1:, 0] == spans[:-1, 0] + spans[:-1, 1]).all()
    assert (spans[1:, 2] == spans[:-1, 2] + spans[:-1, 3]).all()
    assert spans[-1, 0] + spans[-1, 1] == K
    assert spans[-1, 2] + spans[-1, 3] == total_frames
    assert (spans[:, 1] >= 0).all() and (spans[:, 3] >= 0).all()


def random_row(rng, n, up, blank, pad, eos, p_blank=0.6):
    """A seeded row over {blank, pad, 0, eos, 4, 5, 6}: mostly blanks, so repeats and runs that cross a state boundary are common."""
    others = np.array([pad, BOS, eos, 4, 5, 6], dtype=np.int32)
    pick = rng.random(n * up) < p_blank
    return np.where(pick, np.int32(blank), others[rng.integers(0, others.size, n * up)]).astype(np.int32)


def random_dur(rng, count):
    return rng.integers(1, 9, max(int(count), 1)).astype(np.int32)


# ---- the op cases of tests/test_unit_spans_cpu.py (host twin) and tests/test_unit_spans_gpu.py (kernel) ----------------------------
BLANK, PAD, EOS = 1004, 1, 2


def _row(ids, n, up=25):
    r = np.full(n * up, BLANK, dtype=np.int32)
    for f, v in ids.items():
        r[f] = v
    return r


def op_cases():
    """name -> (up, [row, ...]) with row = dict(raw, d0, u0, dur): every case of the issue's list that is about one call's rows."""
    rng = np.random.default_rng(20240607)
    cases = {}

    def finish(up, raws, windows=None):
        rows = []
        for i, raw in enumerate(raws):
            K = int(unit_mask(raw, BLANK, PAD, BOS, EOS).sum())
            d0, u0 = windows[i](K) if windows else (0, 0)
            rows.append({"raw": raw, "d0": d0, "u0": u0, "dur": random_dur(rng, K - d0), "K": K})
        return up, rows

    cases["one_state_all_blank"] = finish(25, [_row({}, 1)])
    cases["run_crosses_boundary"] = finish(25, [_row({24: 7, 25: 7}, 2)])
    cases["blank_between"] = finish(25, [_row({23: 7, 25: 7}, 2)])
    cases["bos_eos"] = finish(25, [_row({3: 5, 10: BOS, 11: 6, 30: EOS, 31: EOS, 40: 9, 60: 8, 74: EOS}, 3)])
    busy = random_row(rng, 6, 25, BLANK, PAD, EOS, p_blank=0.5)
    cases["u0_inside_state"] = finish(25, [busy], [lambda K: (K // 4, K // 2)])
    cases["u0_is_K"] = finish(25, [busy], [lambda K: (K // 3, K)])
    cases["ragged_1_65_3"] = finish(25, [random_row(rng, n, 25, BLANK, PAD, EOS) for n in (1, 65, 3)],
                                    [lambda K: (0, 0), lambda K: (K // 5, K // 3), lambda K: (0, min(1, K))])
    cases["row_of_1030"] = finish(25, [random_row(rng, n, 25, BLANK, PAD, EOS) for n in (2, 1030, 4)],
                                  [lambda K: (0, 0), lambda K: (K // 7, K // 2), lambda K: (0, 0)])
    cases["up_1"] = finish(1, [random_row(rng, n, 1, BLANK, PAD, EOS, 0.3) for n in (1, 2100, 7)],
                           [lambda K: (0, 0), lambda K: (3, 11), lambda K: (0, 0)])
    cases["up_3"] = finish(3, [random_row(rng, n, 3, BLANK, PAD, EOS, 0.4) for n in (5, 700, 1)],
                           [lambda K: (0, min(2, K)), lambda K: (K // 2, K // 2), lambda K: (0, 0)])
    return cases


def pack_rows(rows):
    """-> (raw packed, K, d0, u0, dur packed in the tail's layout: row b at the prefix sum of K, K_b - d0_b values)."""
    raw = np.concatenate([r["raw"] for r in rows]).astype(np.int32)
    K = [int(r["K"]) for r in rows]
    dur = np.zeros(max(sum(K), 1), dtype=np.int32)
    off = 0
    for r in rows:
        m = r["K"] - r["d0"]
        dur[off: off + m] = r["dur"][:m]
        off += r["K"]
    return raw, K, [r["d0"] for r in rows], [r["u0"] for r in rows], dur
