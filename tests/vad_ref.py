"""The endpoint scan of include/streamspeech_hip.h ("Endpointing") restated in NumPy float64, the seeded test streams, and the
wrappers the CPU and GPU suites share for the library's host twin.  Thresholds come from the same dB parameters as the library's
(endpoint.Endpoint.params), kept in float64 here."""
import numpy as np

from streamspeech_amd import endpoint as EP
from streamspeech_amd import lib as L

RATES = (8000, 11025, 16000, 48000)
NOISE_DB, BURST_DB, DC = -70.0, -25.0, 0.25
# (start, end) of the speech bursts in ms: one shorter than min_speech, two separated by a pause shorter than end_silence, then
# silence longer than it; another pair behind
BURSTS_MS = ((300, 350), (600, 1400), (1700, 2200), (3200, 3700))
STREAM_MS = 4600


def make_stream(sr: int, seed: int, bursts_ms=BURSTS_MS, total_ms=STREAM_MS, dc=DC) -> np.ndarray:
    """Seeded noise at -70 dBFS with bursts at -25 dBFS and a DC offset throughout, float32.  Burst edges lie on multiples of the
    shift, so no frame holds only a sample or two of a burst (such a frame would sit at the threshold)."""
    H = int(10 * sr / 1000)
    rng = np.random.default_rng(seed)
    n = total_ms // 10 * H
    x = rng.standard_normal(n) * 10.0 ** (NOISE_DB / 20.0)
    for a, b in bursts_ms:
        i, j = a // 10 * H, b // 10 * H
        x[i:j] += rng.standard_normal(j - i) * 10.0 ** (BURST_DB / 20.0)
    return (x + dc).astype(np.float32)


def ref_thresholds(ep: EP.Endpoint, shift_ms=10):
    """(p_abs, p_min, snr, rise) in float64, from the dB parameters."""
    r = lambda db: 10.0 ** (db / 10.0)                                                                        # noqa: E731
    return r(ep.threshold_db), r(EP.FLOOR_MIN_DB), r(ep.snr_db), r(ep.floor_rise_db_per_s * shift_ms / 1000.0)


def ref_powers(x, H: int, W: int, hist_first: int, first: int, n: int) -> np.ndarray:
    """P_j = mean((x - mean(x))^2) over [j H, j H + W), float64, two passes."""
    out = np.empty(n, np.float64)
    x = np.asarray(x, np.float64)
    for k in range(n):
        f = x[(first + k) * H - hist_first:(first + k) * H - hist_first + W]
        m = f.sum() / W
        out[k] = ((f - m) ** 2).sum() / W
    return out


def fresh_state() -> dict:
    return {"onset": 0, "last_speech": 0, "utt_first_frame": 0, "floor": 0.0, "mode": EP.IDLE, "run": 0}


def ref_scan(P, p: EP.EndpointParams, thr, st: dict, first: int, margins=None) -> dict:
    """The noise floor, the decisions and the state machine over the powers P of frames first, first + 1, ...; `st` is advanced.
    margins: a list that receives |10 log10(P / threshold)| of every decision."""
    p_abs, p_min, snr, rise = thr
    r = {"consumed": first, "start_frame": -1, "cut_sample": -1, "events": 0}
    for k, Pj in enumerate(P):
        j = first + k
        speech = False
        if j == 0:
            st["floor"] = max(p_min, Pj)
        else:
            t = max(p_abs, st["floor"] * snr)
            speech = Pj > t
            if margins is not None:
                margins.append(abs(10.0 * np.log10(max(Pj, 1e-300) / t)))
            st["floor"] = max(p_min, min(Pj, st["floor"] * (1.0 if speech else rise)))
        stop = False
        if st["mode"] == EP.IDLE:
            if speech:
                if st["run"] == 0:
                    st["onset"] = j
                st["run"] += 1
                if st["run"] >= p.min_speech:
                    r["events"] |= EP.START
                    r["start_frame"] = st["onset"]
                    st.update(mode=EP.SPEECH, utt_first_frame=st["onset"], last_speech=j, run=0)
            else:
                st["run"] = 0
        elif speech:
            st.update(last_speech=j, run=0)
        else:
            st["run"] += 1
        if st["mode"] == EP.SPEECH:
            if st["run"] >= p.end_silence:
                r["events"] |= EP.END
                r["cut_sample"] = (st["last_speech"] + 1 + p.post_roll) * p.H + (p.W - p.H)
                st.update(mode=EP.IDLE, run=0)
                stop = True
            elif j + 1 - st["utt_first_frame"] >= p.max_frames:
                r["events"] |= EP.FORCED
                r["cut_sample"] = (j + 1) * p.H + (p.W - p.H)
                st.update(utt_first_frame=j + 1, last_speech=j, run=0)
                stop = True
        r["consumed"] = j + 1
        if stop:
            break
    r["last_speech"], r["mode"] = st["last_speech"], st["mode"]
    return r


def result_dict(r: L.SSVadResult) -> dict:
    return {k: int(getattr(r, k)) for k in ("consumed", "start_frame", "cut_sample", "events", "last_speech", "mode")}


def state_dict(raw: np.ndarray) -> dict:
    s = L.SSVadState.from_buffer_copy(raw.tobytes())
    return {"onset": int(s.onset), "last_speech": int(s.last_speech), "utt_first_frame": int(s.utt_first_frame),
            "floor": float(s.floor), "mode": int(s.mode), "run": int(s.run)}


def host_scan(x: np.ndarray, p: EP.EndpointParams, state: np.ndarray, hist_first: int, first: int, n: int, powers=None) -> dict:
    """One ss_vad_scan_host call over one segment: x (float32) is the history from stream sample hist_first on, `state` the 40-byte
    record (uint8 array, rewritten), powers an optional float32 array of n."""
    seg = p.seg(x.ctypes.data, state.ctypes.data, powers.ctypes.data if powers is not None else 0, hist_first, x.size, first, n)
    return result_dict(EP.scan_host([seg])[0])


def scan_all(scan_one, total_frames: int, chunk: int):
    """Drive a scanner over frames [0, total_frames) in calls of at most `chunk` frames, going on behind every stop.  scan_one(first,
    n) -> result dict.  -> the list of (events, start_frame, cut_sample) of the calls that raised something."""
    events, nxt = [], 0
    while nxt < total_frames:
        r = scan_one(nxt, min(chunk, total_frames - nxt))
        assert nxt < r["consumed"] <= nxt + chunk
        if r["events"]:
            events.append((r["events"], r["start_frame"], r["cut_sample"]))
        nxt = r["consumed"]
    return events


def merge(events):
    """Event lists of different chunkings compare as the sequence of single events."""
    out = []
    for ev, s, c in events:
        if ev & EP.START:
            out.append(("start", s))
        if ev & EP.END:
            out.append(("end", c))
        if ev & EP.FORCED:
            out.append(("forced", c))
    return out
