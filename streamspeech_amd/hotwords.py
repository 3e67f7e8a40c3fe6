"""Hotword lists for the CTC prefix beam search (csrc/ctc_bias.hpp: the phrase automaton and its scoring rule): a text file of
phrases in, the library's own table on the device.

read_hotwords maps a hotword file onto a Dictionary and gives the phrases and boosts ss_ctc_bias_create takes; CtcBias is the
handle on the set the library builds from them -- HipModel.batch_ctc_beam(bias=...), CTCDecoder.beam_search(bias=...),
engine.CtcStream(bias=...), text_pool.CtcBeamOptions(bias=...), the ASR agent's --ctc-hotwords and the offline driver's
--ctc-hotwords-asr / --ctc-hotwords-st take it."""
import ctypes as C
import math
from typing import List, Sequence, Tuple

import numpy as np

from . import lib as L


def read_hotwords(path, dictionary, boost: float = 1.5) -> Tuple[List[List[int]], List[float]]:
    """One phrase per line: space-separated pieces of `dictionary` (the head's own pieces: nothing is tokenised here), optionally a
    tab and the phrase's per-token boost (natural-log units; `boost` where a line gives none).  Blank lines and lines that start
    with `#` are skipped.  -> (phrases as id lists, boosts).  ValueError, naming the line: a piece the dictionary lacks, a boost
    that is not a finite number, a phrase without pieces."""
    unk = dictionary.unk()
    phrases, boosts = [], []
    with open(path, "rt", encoding="utf-8") as f:
        for no, raw in enumerate(f, 1):
            ln = raw.rstrip("\r\n")
            if not ln.strip() or ln.lstrip().startswith("#"):
                continue
            text, tab, b = ln.partition("\t")
            value = float(boost)
            if tab:
                try:
                    value = float(b.strip())
                except ValueError:
                    raise ValueError(f"{path}:{no}: boost {b.strip()!r} is not a number") from None
            if not math.isfinite(value):
                raise ValueError(f"{path}:{no}: boost {value!r} is not finite")
            pieces = text.split()
            if not pieces:
                raise ValueError(f"{path}:{no}: a boost without a phrase")
            ids = [dictionary.index(p) for p in pieces]
            for p, i in zip(pieces, ids):
                if i == unk:
                    raise ValueError(f"{path}:{no}: the dictionary has no piece {p!r}")
            phrases.append(ids)
            boosts.append(value)
    return phrases, boosts


class CtcBias:
    """The library's hotword set (ss_ctc_bias): phrases as id lists of a head's vocabulary, one per-token boost each (a float, or
    one float for all), the head's vocabulary size and its pad / unk ids (-1: none).  Read-only, so one object serves every
    model, context and stream.  A context manager; close() frees it."""

    def __init__(self, phrases: Sequence[Sequence[int]], boosts, vocab: int, pad: int = -1, unk: int = -1):
        self.lib = L.load()
        self.h = None
        phrases = [[int(t) for t in p] for p in phrases]
        if isinstance(boosts, (int, float)):
            boosts = [float(boosts)] * len(phrases)
        if len(boosts) != len(phrases):
            raise ValueError("one boost per phrase")
        self.V, self.pad, self.unk = int(vocab), int(pad), int(unk)
        tok = np.asarray([t for p in phrases for t in p] or [0], np.int32)
        off = np.cumsum([0] + [len(p) for p in phrases]).astype(np.int32)
        bo = np.asarray(list(boosts) or [0.0], np.float32)
        h = C.c_void_p()
        L.check(self.lib.ss_ctc_bias_create(len(phrases), tok.ctypes.data, off.ctypes.data, bo.ctypes.data, self.V, self.pad, self.unk,
                                            C.byref(h)), "ss_ctc_bias_create")
        self.h = h
        p, n, s, d = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.lib.ss_ctc_bias_info(self.h, C.byref(p), C.byref(n), C.byref(s), C.byref(d)), "ss_ctc_bias_info")
        self.n_phrases, self.states, self.slots, self.device_bytes = p.value, n.value, s.value, d.value

    def score(self, token_lists: Sequence[Sequence[int]], finish: bool = True) -> List[float]:
        """Per sequence its bias under the scoring rule, from the root: the sum of its tokens' deltas, minus what an unfinished
        phrase at its end holds when `finish` is set -- the device step (ss_op_ctc_bias_score)."""
        import torch
        B = len(token_lists)
        if B == 0:
            return []
        n = [len(s) for s in token_lists]
        tok = torch.tensor([int(t) for s in token_lists for t in s] or [0], dtype=torch.int32, device="cuda")
        delta = torch.empty((max(sum(n), 1),), dtype=torch.float64, device="cuda")
        out = torch.empty((B,), dtype=torch.float64, device="cuda")
        L.check(self.lib.ss_op_ctc_bias_score(C.c_void_p(torch.cuda.current_stream().cuda_stream), self.h, B, C.c_void_p(tok.data_ptr()),
                                              (C.c_int32 * B)(*n), int(bool(finish)), C.c_void_p(delta.data_ptr()), None,
                                              C.c_void_p(out.data_ptr())), "ss_op_ctc_bias_score")
        return out.cpu().tolist()

    def close(self):
        if getattr(self, "h", None):
            self.lib.ss_ctc_bias_destroy(self.h)
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
