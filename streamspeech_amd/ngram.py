"""Back-off n-gram language models for the CTC prefix beam search (csrc/ngram_lm.hpp: the table and the scoring rule): ARPA text in,
the library's own table on the device.

read_arpa maps an ARPA file onto a Dictionary and gives the arrays ss_ngram_lm_create takes; NgramLM is the handle on the model
the library builds from them -- HipModel.batch_ctc_beam(lm=...), CTCDecoder.beam_search(lm=...) and the offline driver's
--ctc-lm-asr / --ctc-lm-st take it."""
import ctypes as C
import gzip
import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import lib as L

LN10 = math.log(10)
NO_OOV = np.float32(np.float64(-99.0) * LN10)        # ARPA's conventional "never" (-99 in log10), where no oov_logp is given


def to_ln(x) -> np.float32:
    """An ARPA log10 value as the library's float32 natural logarithm."""
    return np.float32(np.float64(x) * LN10)


def read_arpa(path, dictionary, oov_logp: Optional[float] = None) -> Dict:
    """Reads `.arpa` / `.arpa.gz` -> the arrays of a model over `dictionary`: order, counts [order], tokens (the n-grams' ids, order
    by order), logp / backoff (float32 natural logarithms, np.float32(np.float64(x) * ln 10); backoff 0 where the file gives none),
    V, bos / eos / unk (the dictionary's), oov_logp, and `dropped`, the number of n-grams left out because they hold a symbol
    the dictionary lacks.  Raises ValueError when the model has neither a unigram for every ordinary symbol of the dictionary nor
    one for <unk>, unless oov_logp (a natural logarithm) is given: the search could propose a token the model cannot score."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt", encoding="utf-8") as f:
        lines = f.read().splitlines()
    unk = dictionary.unk()
    declared, grams, k = {}, {}, 0
    dropped = 0
    for ln in lines:
        ln = ln.strip()
        if not ln or ln == "\\data\\":
            continue
        if ln == "\\end\\":
            break
        if ln.startswith("ngram ") and "=" in ln and k == 0:
            a, b = ln[6:].split("=")
            declared[int(a)] = int(b)
            continue
        if ln.startswith("\\") and ln.endswith("-grams:"):
            k = int(ln[1:-7])
            grams[k] = []
            continue
        if k == 0:
            continue
        f_ = ln.split()
        if len(f_) not in (k + 1, k + 2):
            raise ValueError(f"{path}: not a {k}-gram line: {ln!r}")
        ids = [dictionary.index(s) for s in f_[1:k + 1]]
        if any(i == unk and s != dictionary[unk] for i, s in zip(ids, f_[1:k + 1])):
            dropped += 1
            continue
        grams[k].append((ids, to_ln(f_[0]), to_ln(f_[k + 1]) if len(f_) == k + 2 else np.float32(0)))
    order = max(grams) if grams else 0
    if order < 1 or sorted(grams) != list(range(1, order + 1)):
        raise ValueError(f"{path}: no n-gram sections, or an order is missing")
    for n, want in declared.items():
        if len(grams.get(n, ())) > want:
            raise ValueError(f"{path}: more {n}-grams than the header declares")
    have = {g[0][0] for g in grams[1]}
    if oov_logp is None and unk not in have:
        for i in range(4, len(dictionary)):
            if i not in have:
                raise ValueError(f"{path}: no unigram for {dictionary[i]!r} and none for <unk>: give oov_logp")
    return {"order": order, "counts": [len(grams[n]) for n in range(1, order + 1)],
            "tokens": np.asarray([i for n in range(1, order + 1) for g in grams[n] for i in g[0]], np.int32),
            "logp": np.asarray([g[1] for n in range(1, order + 1) for g in grams[n]], np.float32),
            "backoff": np.asarray([g[2] for n in range(1, order + 1) for g in grams[n]], np.float32),
            "V": len(dictionary), "bos": dictionary.bos(), "eos": dictionary.eos(), "unk": unk,
            "oov_logp": float(NO_OOV if oov_logp is None else oov_logp), "dropped": dropped}


class NgramLM:
    """The library's model object (ss_ngram_lm), built from read_arpa's arrays (or the same keys made any other way): read-only,
    so one object serves every model, context and stream.  A context manager; close() frees it."""

    def __init__(self, arrays: Dict):
        self.lib = L.load()
        a = arrays
        self.V, self.bos, self.eos, self.unk = int(a["V"]), int(a["bos"]), int(a["eos"]), int(a["unk"])
        self.dropped = int(a.get("dropped", 0))
        counts = (C.c_int64 * max(len(a["counts"]), 1))(*[int(c) for c in a["counts"]])
        tok = np.ascontiguousarray(a["tokens"], np.int32)
        lp = np.ascontiguousarray(a["logp"], np.float32)
        bo = np.ascontiguousarray(a["backoff"], np.float32)
        n = sum(int(c) for c in a["counts"])
        if lp.size != n or bo.size != n or tok.size != sum((k + 1) * int(c) for k, c in enumerate(a["counts"])):
            raise ValueError("counts, tokens, logp and backoff do not describe the same n-grams")
        h = C.c_void_p()
        L.check(self.lib.ss_ngram_lm_create(int(a["order"]), counts, tok.ctypes.data, lp.ctypes.data, bo.ctypes.data, self.V, self.bos,
                                            self.eos, self.unk, float(a.get("oov_logp", NO_OOV)), C.byref(h)), "ss_ngram_lm_create")
        self.h = h
        o, e, s, d = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(self.lib.ss_ngram_lm_info(self.h, C.byref(o), C.byref(e), C.byref(s), C.byref(d)), "ss_ngram_lm_info")
        self.order, self.entries, self.slots, self.device_bytes = o.value, e.value, s.value, d.value

    def score(self, seqs: Sequence[Sequence[int]], eos: bool = True) -> List[np.ndarray]:
        """Per sequence the float64 lp of each of its tokens under the scoring rule, from the start state, and with `eos` one
        more, lp(eos | final state): the device lookup (ss_op_ngram_score)."""
        import torch
        B = len(seqs)
        if B == 0:
            return []
        n = [len(s) for s in seqs]
        total = sum(n) + (B if eos else 0)
        tok = torch.tensor([int(t) for s in seqs for t in s] or [0], dtype=torch.int32, device="cuda")
        out = torch.empty((max(total, 1),), dtype=torch.float64, device="cuda")
        L.check(self.lib.ss_op_ngram_score(C.c_void_p(torch.cuda.current_stream().cuda_stream), self.h, B, C.c_void_p(tok.data_ptr()),
                                           (C.c_int32 * B)(*n), int(bool(eos)), C.c_void_p(out.data_ptr()), None), "ss_op_ngram_score")
        host = out.cpu().numpy()
        res, o = [], 0
        for k in n:
            res.append(host[o:o + k + (1 if eos else 0)].copy())
            o += k + (1 if eos else 0)
        return res

    def close(self):
        if getattr(self, "h", None):
            self.lib.ss_ngram_lm_destroy(self.h)
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
