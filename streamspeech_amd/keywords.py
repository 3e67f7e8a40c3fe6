"""Keyword lists for the spotter on the CTC heads (csrc/ctc_spot.hpp: the recursion and the emission rule; the rule itself is in
include/streamspeech_hip.h at ss_batch_ctc_spot): a text file of phrases in, the library's own table on the device.

read_keywords maps a keyword file -- the hotword file format -- onto a Dictionary and gives the phrases and thresholds
ss_ctc_spot_set_create takes; CtcKeywords is the handle on the set the library builds from them -- HipModel.batch_ctc_spot,
CTCDecoder.spot, engine.CtcSpotStream, text_pool.TextSessionPool(spot=...), the ASR agent's --ctc-keywords and the offline driver's
--ctc-keywords-asr / --ctc-keywords-st take it.  CtcHit is what they all report."""
import ctypes as C
import math
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

from . import lib as L
from .hotwords import read_hotwords

DEFAULT_THRESHOLD = 1.0     # tau, natural-log units per label: a stated starting point, not tuned on a trained checkpoint

HIT_DTYPE = np.dtype([("keyword", "<i4"), ("start", "<i4"), ("end", "<i4"), ("n_labels", "<i4"), ("score", "<f8")])
COUNT_DTYPE = np.dtype([("n_hits", "<i4"), ("status", "<i4"), ("overflow", "<i4"), ("frames", "<i4")])


class CtcHit(NamedTuple):
    """One occurrence of a keyword: encoder rows [start, end] of its utterance, both inclusive."""
    keyword: int     # index into the set
    start: int
    end: int
    score: float     # the path's log-likelihood ratio against the arg-max path over the same frames, <= 0
    norm: float      # score / n_labels: what the keyword's threshold bounds (norm >= -tau)


class KeywordHit(NamedTuple):
    """A hit on a session's or an utterance's clock, as the pools, the agent and the driver report it: [start_ms, end_ms)."""
    keyword: int
    phrase: str
    start_ms: int
    end_ms: int
    score: float
    norm: float


def hits_from_records(rec) -> List[CtcHit]:
    """The tuples of a slice of ss_ctc_hit records (a numpy array of HIT_DTYPE)."""
    cols = [rec[name].tolist() for name in ("keyword", "start", "end", "score", "n_labels")]     # (field-wise: one pass per column)
    return [CtcHit(k, a, z, x, x / n) for k, a, z, x, n in zip(*cols)]


def read_keywords(path, dictionary, threshold: float = DEFAULT_THRESHOLD) -> Tuple[List[List[int]], List[float]]:
    """The hotword file format (hotwords.read_hotwords, whose parser this is): one phrase of `dictionary` pieces per line,
    optionally a tab and that phrase's threshold tau; `threshold` where a line gives none.  -> (phrases as id lists, thresholds).
    ValueError also for a negative threshold."""
    phrases, taus = read_hotwords(path, dictionary, boost=threshold)
    for p, t in zip(phrases, taus):
        if not (t >= 0.0) or not math.isfinite(t):
            raise ValueError(f"{path}: threshold {t!r} of phrase {p} is negative")
    return phrases, taus


class CtcKeywords:
    """The library's keyword set (ss_ctc_spot_set): phrases as id lists of a head's vocabulary, one threshold each (a float, or one
    float for all), the head's vocabulary size and its pad / unk ids (-1: none).  Read-only, so one object serves every model,
    context and stream of one device: the one that is current at its first device call (make a set per device).  `texts` (optional): the phrases as the caller wrote them, for reports.  A context manager; close() frees it."""

    def __init__(self, phrases: Sequence[Sequence[int]], thresholds=DEFAULT_THRESHOLD, vocab: int = 0, pad: int = -1, unk: int = -1,
                 texts: Sequence[str] = None):
        self.lib = L.load()
        self.h = None
        self.phrases = [[int(t) for t in p] for p in phrases]
        if isinstance(thresholds, (int, float)):
            thresholds = [float(thresholds)] * len(self.phrases)
        if len(thresholds) != len(self.phrases):
            raise ValueError("one threshold per phrase")
        self.thresholds = [float(t) for t in thresholds]
        self.texts = list(texts) if texts is not None else [" ".join(str(t) for t in p) for p in self.phrases]
        self.V, self.pad, self.unk = int(vocab), int(pad), int(unk)
        tok = np.asarray([t for p in self.phrases for t in p] or [0], np.int32)
        off = np.cumsum([0] + [len(p) for p in self.phrases]).astype(np.int32)
        tau = np.asarray(self.thresholds or [0.0], np.float32)
        h = C.c_void_p()
        L.check(self.lib.ss_ctc_spot_set_create(len(self.phrases), tok.ctypes.data, off.ctypes.data, tau.ctypes.data, self.V, self.pad,
                                                self.unk, C.byref(h)), "ss_ctc_spot_set_create")
        self.h = h
        k, u, g, s, d = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        L.check(self.lib.ss_ctc_spot_set_info(self.h, C.byref(k), C.byref(u), C.byref(s), C.byref(g), C.byref(d)), "ss_ctc_spot_set_info")
        self.n_keywords, self.n_labels, self.states, self.workgroups, self.device_bytes = k.value, u.value, s.value, g.value, d.value

    @classmethod
    def from_file(cls, path, dictionary, threshold: float = DEFAULT_THRESHOLD) -> "CtcKeywords":
        """The set of a keyword file over `dictionary` (a head's own): its size, pad and unk are the dictionary's."""
        phrases, taus = read_keywords(path, dictionary, threshold)
        return cls(phrases, taus, len(dictionary), dictionary.pad(), dictionary.unk(),
                   texts=[" ".join(dictionary[i] for i in p) for p in phrases])

    def spot_host(self, logits: np.ndarray, T: Sequence[int], max_hits: int = 256):
        """The plain-C++ twin on host logits [sum T][>= V] (ss_ctc_spot_host) -> (hit records [B][max_hits], count records [B])."""
        logits = np.ascontiguousarray(logits, np.float32)
        B = len(T)
        hits = np.zeros((max(B, 1), max(int(max_hits), 1)), HIT_DTYPE)
        counts = np.zeros((max(B, 1),), COUNT_DTYPE)
        L.check(self.lib.ss_ctc_spot_host(logits.ctypes.data, logits.shape[1] if logits.ndim == 2 else 0, B,
                                          (C.c_int32 * max(B, 1))(*[int(t) for t in T]), self.h, int(max_hits), hits.ctypes.data,
                                          counts.ctypes.data), "ss_ctc_spot_host")
        return hits, counts

    def close(self):
        if getattr(self, "h", None):
            self.lib.ss_ctc_spot_set_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
