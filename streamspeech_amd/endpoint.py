"""Endpointing of live PCM streams in the session pools: a phone call or a browser microphone never says
"finished", so a session opened with ``endpoint=Endpoint(...)`` has its continuous stream cut into utterances by the pool.  The scan
is energy-based and runs on the device where the decoded samples already lie: ONE ss_vad_scan launch (csrc/vad.hip) over the new
frames of every endpointed session of a step, one small download of the result records, and the host decides what each session
commits.  :class:`Endpoint` holds the caller's parameters in dB and milliseconds; :meth:`Endpoint.params` converts them ONCE to the
float32 power ratios and frame counts the scan takes (there is no logarithm in the scan itself, so kernel and host twin agree bit
for bit); :class:`EndpointState` is one session's side: the device state record and the host's bookkeeping of the stream."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import lib as L

IDLE, SPEECH = 0, 1
START, END, FORCED = 1, 2, 4
FLOOR_MIN_DB = -100.0                       # P_min: the noise floor never falls below this (digital silence would make it 0)
STATE_BYTES, RESULT_BYTES = 40, 40          # sizeof(ss_vad_state), sizeof(ss_vad_result)


def _number(name, v, lo=None, strict=False):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise ValueError(f"Endpoint.{name} = {v!r}: a finite number")
    if lo is not None and (v <= lo if strict else v < lo):
        raise ValueError(f"Endpoint.{name} = {v!r}: {'above' if strict else 'at least'} {lo}")


@dataclass(frozen=True)
class EndpointParams:
    """An :class:`Endpoint` at one sample rate and framing: what a ss_vad_seg carries, and the host's sample counts."""
    H: int
    W: int
    p_abs: float
    p_min: float
    snr: float
    rise: float
    min_speech: int
    end_silence: int
    post_roll: int
    max_frames: int
    pre_roll_samples: int
    max_utterance_samples: int

    def seg(self, hist_ptr, state_ptr, powers_ptr, hist_first, n_hist, first_frame, n_frames):
        """The segment tuple of :func:`scan` / :func:`scan_host` (ss_vad_seg field for field, without `reserved`)."""
        return (hist_ptr, state_ptr, powers_ptr, hist_first, n_hist, first_frame, n_frames, self.H, self.W, self.p_abs, self.p_min,
                self.snr, self.rise, self.min_speech, self.end_silence, self.post_roll, self.max_frames)

    def frames_present(self, n_samples: int) -> int:
        """Whole frames [j H, j H + W) inside the first n_samples samples of the stream."""
        return 0 if n_samples < self.W else (n_samples - self.W) // self.H + 1

    @property
    def idle_keep(self) -> int:
        """Samples an idle session keeps behind its next frame: pre-roll, the onset run, one window."""
        return self.pre_roll_samples + self.min_speech * self.H + self.W


@dataclass(frozen=True)
class Endpoint:
    """How a session's stream is cut.  A frame (the session's own fbank framing) is speech when its power, mean removed, lies above
    `threshold_db` (dB re full scale) AND `snr_db` above the tracked noise floor; the floor follows the power down at once and up by
    `floor_rise_db_per_s`, and stands still during speech.  `min_speech_ms` of speech in a row start an utterance, which then begins
    `pre_roll_ms` before that run; `end_silence_ms` without speech end it, `post_roll_ms` (at most end_silence_ms) behind its last
    speech frame.  `max_utterance_ms` forces a cut; None: the longest utterance whose encoder rows fit the pool's max_rows."""
    threshold_db: float = -50.0
    snr_db: float = 9.0
    floor_rise_db_per_s: float = 2.0
    min_speech_ms: float = 100
    end_silence_ms: float = 600
    pre_roll_ms: float = 200
    post_roll_ms: float = 200
    max_utterance_ms: Optional[float] = None

    def __post_init__(self):
        _number("threshold_db", self.threshold_db)
        if self.threshold_db > 0 or self.threshold_db < FLOOR_MIN_DB:
            raise ValueError(f"Endpoint.threshold_db = {self.threshold_db!r}: between {FLOOR_MIN_DB} and 0 dB re full scale")
        _number("snr_db", self.snr_db, 0)
        _number("floor_rise_db_per_s", self.floor_rise_db_per_s, 0)
        _number("min_speech_ms", self.min_speech_ms, 0, strict=True)
        _number("end_silence_ms", self.end_silence_ms, 0, strict=True)
        _number("pre_roll_ms", self.pre_roll_ms, 0)
        _number("post_roll_ms", self.post_roll_ms, 0)
        if self.post_roll_ms > self.end_silence_ms:
            raise ValueError(f"Endpoint.post_roll_ms = {self.post_roll_ms!r} is more than end_silence_ms = {self.end_silence_ms!r}: "
                             "a cut would lie past the frame that finds it")
        if self.max_utterance_ms is not None:
            _number("max_utterance_ms", self.max_utterance_ms, 0, strict=True)

    def params(self, sr: int, shift_ms=10, window_ms=25, fit_samples: Optional[int] = None) -> EndpointParams:
        """The scan's parameters at `sr` Hz: thresholds as float32 linear power ratios, times as frame counts (starts and ends rounded
        up to whole frames, the post-roll down).  fit_samples: the longest utterance the pool holds, which bounds max_utterance_ms
        and stands in for it when it is None.  ValueError when the utterance limit leaves no room for an utterance."""
        H, W = int(shift_ms * sr / 1000), int(window_ms * sr / 1000)
        if H < 1 or W < H:
            raise ValueError(f"framing of {shift_ms} / {window_ms} ms at {sr} Hz: shift {H}, window {W} samples")
        ratio = lambda db: float(np.float32(10.0 ** (db / 10.0)))                                            # noqa: E731
        min_speech = max(1, math.ceil(self.min_speech_ms / shift_ms))
        end_silence = max(1, math.ceil(self.end_silence_ms / shift_ms))
        post_roll = min(end_silence, int(self.post_roll_ms // shift_ms))
        pre = int(self.pre_roll_ms * sr / 1000)
        if self.max_utterance_ms is None:
            if fit_samples is None:
                raise ValueError("Endpoint.max_utterance_ms is None and there is no pool to take the limit from")
            max_samples = int(fit_samples)
        else:
            max_samples = int(self.max_utterance_ms * sr / 1000)
            if fit_samples is not None and max_samples > fit_samples:
                raise ValueError(f"Endpoint.max_utterance_ms = {self.max_utterance_ms!r}: {max_samples} samples at {sr} Hz, the pool's "
                                 f"max_rows holds utterances of {fit_samples}")
        # an utterance is at most pre-roll + max_frames H + (W - H) samples long (FORCED fires max_frames behind the onset)
        max_frames = (max_samples - (W - H) - pre) // H
        if max_frames <= min_speech:
            raise ValueError(f"an utterance limit of {max_samples} samples at {sr} Hz leaves {max_frames} frames behind the pre-roll: "
                             f"more than min_speech ({min_speech} frames) are needed")
        return EndpointParams(H, W, ratio(self.threshold_db), ratio(FLOOR_MIN_DB), ratio(self.snr_db),
                              ratio(self.floor_rise_db_per_s * shift_ms / 1000.0), min_speech, end_silence, post_roll,
                              int(min(max_frames, 2 ** 31 - 1)), pre, max_samples)


def seg_table(segs):
    tab = (L.SSVadSeg * max(len(segs), 1))()
    for i, sg in enumerate(segs):
        tab[i] = L.SSVadSeg(*sg, 0)
    return tab


def scan(lib, stream, segs, results: torch.Tensor):
    """ss_vad_scan: the segment tuples of EndpointParams.seg (device pointers) -> row i of the uint8 device tensor `results` [n, 40]."""
    if results.dtype != torch.uint8 or not results.is_contiguous() or results.numel() < RESULT_BYTES * len(segs):
        raise ValueError("scan: a contiguous uint8 result tensor of 40 bytes per segment")
    L.check(lib.ss_vad_scan(stream, seg_table(segs), len(segs), C.c_void_p(results.data_ptr() if len(segs) else 0)), "ss_vad_scan")


def scan_host(segs, lib=None) -> List[L.SSVadResult]:
    """ss_vad_scan_host: the same call with host pointers (NumPy arrays, CPU tensors) -> the result records."""
    res = (L.SSVadResult * max(len(segs), 1))()
    L.check((lib or L.load()).ss_vad_scan_host(seg_table(segs), len(segs), res), "ss_vad_scan_host")
    return [res[i] for i in range(len(segs))]


def read_results(buf: np.ndarray, n: int) -> List[L.SSVadResult]:
    """n result records out of a host byte buffer (the pinned copy of a step's results)."""
    return [L.SSVadResult.from_buffer_copy(buf[RESULT_BYTES * i: RESULT_BYTES * (i + 1)].tobytes()) for i in range(n)]


class EndpointState:
    """One endpointed session: the 40-byte device state record of the scan, and what the host knows of the stream.  The session's
    device history (OnlineFeatureExtractor._dev) holds the stream from sample `base` on: the `fe.n_pcm` samples the current utterance
    has committed, then `held` samples that are received and not committed (all of them while the session is idle); up to a window
    of samples before `base` stays in front of it, for the frames that straddle a cut."""

    def __init__(self, endpoint: Endpoint, params: EndpointParams, device):
        self.endpoint, self.p = endpoint, params
        self.dev_state = torch.zeros((STATE_BYTES,), dtype=torch.uint8, device=device)
        self.buf = None                        # the buffer the session's device history is a view into
        self.reset()

    def reset(self):
        self.dev_state.zero_()
        self.base = 0                          # stream index of the history's first sample
        self.held = 0
        self.next_frame = 0                    # first frame not scanned
        self.mode, self.last_speech = IDLE, 0  # the device state's, as of the last result
        self.in_utt = False                    # an utterance is open (between START / FORCED and its END / FORCED / stream end)
        self.utt_start = 0
        self.prev_cut = 0
        self.stream_finished = False           # push_pcm(finished=True) was seen
        self.done = False                      # ... and has taken effect
        self.deferred = None                   # (result, samples at scan time) of a scan whose START found no free slot
        self.final = False                     # the utterance ended in the step under way: the pool resets the session behind it
        self.lead = 0                          # valid samples in front of the history's first (text_pool._ep_room), at most a window
        self.utterances: List[dict] = []
