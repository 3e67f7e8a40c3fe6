"""Python host side of the HIP library: owns device memory (torch tensors), hands raw pointers
to the C ABI.  Torch is plumbing here (allocation, streams, H2D/D2H copies) -- every FLOP of the
S2ST path runs in libstreamspeech_hip.so.
"""
import ctypes as C
import os
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import lib as L
from .config import ModelConfig, VocoderConfig
from .weights import pack_model, pack_vocoder


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise L.StreamSpeechHipError(
            "streamspeech_amd needs an AMD GPU (torch.cuda.is_available() is False); "
            "there is no CPU fallback for the product path")
    return torch.device(device)


def _slots(names, offsets, numels):  # noqa: E302
    n = len(names)
    c_names = (C.c_char_p * n)(*[s.encode() for s in names])
    c_off = (C.c_int64 * n)(*offsets)
    c_num = (C.c_int64 * n)(*numels)
    return c_names, c_off, c_num, n


def _i32(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def _unpack_scored(host, T: List[int], return_raw: bool = False):
    """One head's scored CTC answer on the host: int32 [6 tot + n] = raw | tokens | index | last | lprob bits | tok_lprob bits | counts
    (the float bits ride in the int32 buffer: one device-to-host copy).  -> per session (tokens, index, last, tok_lprob, lprob rows)."""
    tot, fl = sum(T), host.view(np.float32)
    out, off = [], 0
    for b, t in enumerate(T):
        n = int(host[6 * tot + b])
        rec = (host[tot + off: tot + off + n].tolist(), host[2 * tot + off: 2 * tot + off + n].tolist(),
               host[3 * tot + off: 3 * tot + off + n].tolist(), fl[5 * tot + off: 5 * tot + off + n].copy(),
               fl[4 * tot + off: 4 * tot + off + t].copy())
        out.append(rec + (host[off: off + t].tolist(),) if return_raw else rec)
        off += t
    return out


class CtcAlignment(NamedTuple):
    """One utterance of batch_ctc_align (ss_ctc_align_result and the spans behind it)."""
    score: float            # log p(labels | audio): the CTC forward sum
    viterbi_score: float    # the log-probability of the best path, the one path / first / last describe
    status: int             # 0 aligned, 1 infeasible, 2 a NaN in a row of the utterance
    path: Optional[List[int]]      # token id per frame, 0 = blank (-1 where there is no path); None without want_path
    first: List[int]        # per label, the first ...
    last: List[int]         # ... and the last frame of its run on the path (-1 where there is no path)
    tok_lprob: np.ndarray   # per label, the float32 sum of the per-frame log-probability over that run (NaN where there is no path)


class CtcHypothesis(NamedTuple):
    """One hypothesis of batch_ctc_beam."""
    tokens: List[int]       # the labels (never blank, pad or unk)
    score: float            # log of the summed probability of its alignments: the scale of CtcAlignment.score
    # with an n-gram model (batch_ctc_beam(lm=...)): score is the fused one, log p_ctc + lm_weight * lm_score + word_score * n
    ctc_score: Optional[float] = None   # log p_ctc alone, the scale above
    lm_score: Optional[float] = None    # the model's log-probability of the tokens (and </s>, with lm_eos): natural log, unweighted

    @property
    def bias_score(self) -> Optional[float]:
        """None: a search without a hotword set (with one the hypotheses are CtcBiasHypothesis, which carry it)."""
        return None


class CtcBiasHypothesis(NamedTuple):
    """One hypothesis of batch_ctc_beam(bias=...): CtcHypothesis with a trailing bias_score.  score is the fused one, log p_ctc
    [+ lm_weight * lm_score + word_score * n] + bias_scale * bias_score."""
    tokens: List[int]
    score: float
    ctc_score: float
    lm_score: Optional[float]           # None without a model
    bias_score: float                   # the hotword set's credit for the tokens, natural log, unscaled; with bias_finish an
    #                                     unfinished phrase at the end has earned nothing


_BIAS_HYP = np.dtype([("score", "<f8"), ("ctc_score", "<f8"), ("lm_score", "<f8"), ("bias_score", "<f8"), ("n_tokens", "<i4"),
                      ("status", "<i4")])


def ctc_beam_default_cand(beam: int) -> int:
    """Candidates per frame when the caller names none: beam + 1, up to the library's cap.  A new string enters the beam only past
    the extensions of its own parent by better tokens, and at most one of those is the parent's last label (the one token whose
    extension weighs less), so no token below place beam + 1 of a frame can bring a new string into a beam of `beam`."""
    return min(L.CTC_BEAM_MAX_CAND, int(beam) + 1)


def resample_ratio(sr_in: int, sr_out: int = 16000) -> Tuple[int, int, int]:
    """(up, down, half_len) of the resampler from sr_in to sr_out: the ratio in lowest terms and the taps on either side of the
    centre of frontend.design_filter's low-pass (0 when nothing is resampled)."""
    import math
    from .frontend import filter_half_len
    g = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    return up, down, (0 if up == down else filter_half_len(up, down))


def fbank_sr_rows(n_in: int, up: int, down: int, half_len: int, lib=None) -> Optional[Tuple[int, int]]:
    """The library's own count (ss_fbank_sr_rows, host only): (fbank rows n_in source samples resample to, how many of them are final
    -- no later sample changes them); None for a ratio ss_batch_fbank_frames_sr refuses."""
    lib = lib or L.load()
    rows, fin = C.c_int32(0), C.c_int32(0)
    rc = lib.ss_fbank_sr_rows(int(n_in), int(up), int(down), int(half_len), C.byref(rows), C.byref(fin))
    if rc == L.SS_ERR_ARG:
        return None
    L.check(rc, "ss_fbank_sr_rows")
    return rows.value, fin.value


def _as_i64(x: int) -> int:
    """A 64-bit key as the signed value ctypes takes (keys are bit patterns: 2**64 - 1 and -1 are the same key)."""
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x - (1 << 64) if x >= 1 << 63 else x


MT_BEAM_MAX_ROWS = 256     # B * beam hypothesis rows of one ss_batch_mt_beam call
MT_BEAM_MAX = 32


def check_search_options(len_penalty: float = 1.0, temperature: float = 1.0, no_repeat_ngram_size: int = 0):
    """The library's refusals of the three search controls, raised as ValueError before anything is booked -> the ss_mt_search_opts
    to pass (None at the defaults).  n = 1 is refused: the reference's Python path bans nothing there and its compiled extension
    bans every seen token."""
    n, p, t = int(no_repeat_ngram_size), float(len_penalty), float(temperature)
    if n != no_repeat_ngram_size or (n != 0 and not 2 <= n <= 32):
        raise ValueError(f"no_repeat_ngram_size {no_repeat_ngram_size} outside {{0, 2..32}}")
    if not np.isfinite(p):
        raise ValueError(f"len_penalty {len_penalty} is not finite")
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"temperature {temperature} is not a finite positive number")
    return L.search_opts(p, t, n)


def check_sampling_options(topk: int = 0, topp: float = 0.0, seed: int = 1, vocab: Optional[int] = None):
    """The library's refusals of the sampling controls (ss_mt_sample_opts), raised as ValueError before anything is booked -> the
    ss_mt_sample_opts to pass.  topk 0 / topp 0 switch the control off; both set is refused (the reference silently prefers
    top-p)."""
    k, p = int(topk), float(topp)
    if k != topk or k < 0 or (vocab is not None and k > vocab):
        raise ValueError(f"sampling top-k {topk} outside [0, vocabulary]")
    if not np.isfinite(p) or p < 0.0 or p > 1.0:
        raise ValueError(f"sampling top-p {topp} outside {{0}} u (0, 1]")
    if k > 0 and p > 0.0:
        raise ValueError("sampling top-k and top-p are both set")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed {seed} is not a 64-bit unsigned integer")
    return L.sample_opts(k, p, int(seed))


def sampling_stream_key(session_id: int, n_writes: int) -> int:
    """The stream key of a streaming session's write: the session id and the count of writes so far.  A replayed session samples
    the same, and two sessions never share a stream."""
    return ((int(session_id) & 0xFFFFFFFFFF) << 24) | (int(n_writes) & 0xFFFFFF)


class SamplingOptions:
    """Sampling of the first-pass text search as one object (the session pools' ``search=`` takes it in place of a SearchOptions,
    which it may carry as ``search``): the reference generator's sampling_topk / sampling_topp (fairseq's -1 = off is 0 here) and
    seed."""

    def __init__(self, topk: int = 0, topp: float = 0.0, seed: int = 1, search=None):
        check_sampling_options(topk, topp, seed)
        self.topk, self.topp, self.seed = int(topk), float(topp), int(seed)
        self.search = search

    def kwargs(self) -> dict:
        return {"topk": self.topk, "topp": self.topp, "seed": self.seed}

    def __repr__(self):
        return f"SamplingOptions(topk={self.topk}, topp={self.topp}, seed={self.seed})"


def sampling_from_fairseq(sampling: bool, sampling_topk: int = -1, sampling_topp: float = -1.0, seed: int = 1):
    """fairseq's generator arguments (build_generator: -1 = off) -> SamplingOptions, or None without sampling.  As there, top-k or
    top-p without --sampling is an error."""
    k, p = int(sampling_topk), float(sampling_topp)
    if not sampling:
        if k > 0 or p > 0:
            raise ValueError("--sampling-topk / --sampling-topp require --sampling")
        return None
    return SamplingOptions(k if k > 0 else 0, p if p > 0 else 0.0, seed)


class SearchOptions:
    """The three controls of the first-pass text search as one object (the session pools' ``search=``): the reference generator's
    len_penalty, temperature and no_repeat_ngram_size.  Refused values raise ValueError here (check_search_options)."""

    def __init__(self, len_penalty: float = 1.0, temperature: float = 1.0, no_repeat_ngram_size: int = 0):
        check_search_options(len_penalty, temperature, no_repeat_ngram_size)
        self.len_penalty, self.temperature = float(len_penalty), float(temperature)
        self.no_repeat_ngram_size = int(no_repeat_ngram_size)

    def kwargs(self) -> dict:
        """The keywords batch_mt_beam / batch_mt_beam_continue take; empty when every control is at its default."""
        if (self.len_penalty, self.temperature, self.no_repeat_ngram_size) == (1.0, 1.0, 0):
            return {}
        return {"len_penalty": self.len_penalty, "temperature": self.temperature, "no_repeat_ngram_size": self.no_repeat_ngram_size}

    def __repr__(self):
        return (f"SearchOptions(len_penalty={self.len_penalty}, temperature={self.temperature}, "
                f"no_repeat_ngram_size={self.no_repeat_ngram_size})")


def plan_beam_groups(B: int, beam: int, max_rows: int = MT_BEAM_MAX_ROWS) -> List[Tuple[int, int]]:
    """Consecutive [start, end) utterance ranges, in order, with (end - start) * beam <= max_rows."""
    if not 1 <= beam <= max_rows:
        raise ValueError(f"beam {beam} outside [1, {max_rows}]")
    per = max_rows // beam
    return [(b, min(b + per, B)) for b in range(0, B, per)]


class BatchMixin:
    """Ragged-batch calls on a HipModel (B utterances packed along the row axis, no padding)."""

    def batch_fbank_cmvn(self, pcm_packed: torch.Tensor, n_samples: List[int], pcm_scale: float = 32768.0):
        B = len(n_samples)
        starts = np.concatenate([[0], np.cumsum(n_samples)[:-1]]).astype(np.int64)
        T = [self.lib.ss_fbank_num_frames(int(n)) for n in n_samples]
        feat = torch.empty((sum(T), 80), dtype=torch.float32, device=self.device)
        hT = (C.c_int32 * B)()
        L.check(self.lib.ss_batch_fbank_cmvn(self.h, _stream(), B, _ptr(pcm_packed), (C.c_int64 * B)(*starts.tolist()),
                                             _i32(n_samples), pcm_scale, _ptr(feat), hT), "ss_batch_fbank_cmvn")
        return feat, list(hT)

    def batch_cmvn(self, feats_packed: torch.Tensor) -> torch.Tensor:
        """Precomputed raw fbank rows [rows, 80] -> (x - mean) / std with the model's CMVN vectors, fbank_row's last line (one launch)."""
        if feats_packed.dtype != torch.float32 or feats_packed.dim() != 2 or feats_packed.shape[1] != 80 or not feats_packed.is_contiguous():
            raise ValueError("batch_cmvn takes a contiguous float32 [rows, 80] tensor")
        out = torch.empty_like(feats_packed)
        L.check(self.lib.ss_batch_cmvn(self.h, _stream(), _ptr(feats_packed), feats_packed.shape[0], _ptr(out)), "ss_batch_cmvn")
        return out

    def batch_encoder_forward(self, fbank_packed: torch.Tensor, T: List[int], attn_chunk=999999, conv_chunk=999999):
        B = len(T)
        Tp = [self.lib.ss_encoder_out_len(int(t)) for t in T]
        out = torch.empty((sum(Tp), self.cfg.enc_dim), dtype=torch.float32, device=self.device)
        hTp = (C.c_int32 * B)()
        L.check(self.lib.ss_batch_encoder_forward(self.h, _stream(), B, _ptr(fbank_packed), _i32(T),
                                                  int(min(attn_chunk, 1 << 30)), int(min(conv_chunk, 1 << 30)),
                                                  _ptr(out), hTp), "ss_batch_encoder_forward")
        return out, list(hTp)

    def batch_ctc_greedy(self, head: int, enc_packed: torch.Tensor, Tp: List[int], return_raw: bool = False,
                         return_scores: bool = False):
        """-> per-utterance (tokens, frame index) lists (+ the raw per-frame argmax with return_raw).  With return_scores each
        record is (tokens, index, last frame per token, summed log-probability per token [float32], log-probability per frame
        [float32 Tp]) (+ raw): the reference's `positional_scores` (agent/ctc_decoder.py:61) and the spans they are summed over."""
        B, tot = len(Tp), sum(Tp)
        if return_scores:
            ibuf = torch.empty((6 * tot + B,), dtype=torch.int32, device=self.device)
            fbuf = ibuf.view(torch.float32)
            p = [_ptr(ibuf[k * tot:(k + 1) * tot]) for k in range(4)] + [_ptr(fbuf[k * tot:(k + 1) * tot]) for k in (4, 5)]
            L.check(self.lib.ss_batch_ctc_greedy_scored(self.h, _stream(), head, B, _ptr(enc_packed), _i32(Tp), p[0], p[1], p[2],
                                                        _ptr(ibuf[6 * tot:]), p[4], p[3], p[5]), "ss_batch_ctc_greedy_scored")
            return _unpack_scored(ibuf.cpu().numpy(), Tp, return_raw)
        ibuf = torch.empty((3 * tot + B,), dtype=torch.int32, device=self.device)
        raw, toks, idx, cnt = ibuf[:tot], ibuf[tot:2 * tot], ibuf[2 * tot:3 * tot], ibuf[3 * tot:]
        L.check(self.lib.ss_batch_ctc_greedy(self.h, _stream(), head, B, _ptr(enc_packed), _i32(Tp), _ptr(raw),
                                             _ptr(toks), _ptr(idx), _ptr(cnt)), "ss_batch_ctc_greedy")
        host = ibuf.cpu().numpy()
        out, off = [], 0
        for b in range(B):
            n = int(host[3 * tot + b])
            rec = (host[tot + off: tot + off + n].tolist(), host[2 * tot + off: 2 * tot + off + n].tolist())
            out.append(rec + (host[off: off + Tp[b]].tolist(),) if return_raw else rec)
            off += Tp[b]
        return out

    def batch_ctc_align(self, head: int, enc_packed: torch.Tensor, Tp: List[int], targets: List[List[int]],
                        want_path: bool = True) -> List[CtcAlignment]:
        """Forced alignment and score of the given label ids on a text head (ss_batch_ctc_align): per utterance where its labels lie
        in its frames and log p(labels | audio).  The rows are packed as batch_ctc_greedy takes them; an empty label list is legal.
        One buffer, one device-to-host copy.  The library refuses (SS_ERR_ARG, nothing launched) a label that is blank, pad, negative
        or outside the vocabulary and more than L.CTC_ALIGN_MAX_LABELS labels or L.CTC_ALIGN_MAX_FRAMES frames per utterance."""
        B, tot = len(Tp), sum(int(t) for t in Tp)
        if len(targets) != B:
            raise ValueError("one label list per utterance")
        n = [len(t) for t in targets]
        flat = [int(v) for t in targets for v in t]
        nl = len(flat)
        # int32 words: results [6 B] (two doubles and two ints each, first: 8-byte aligned) | path [tot] | first | last | tok_lprob [nl]
        ibuf = torch.empty((6 * B + tot + 3 * nl,), dtype=torch.int32, device=self.device)
        o_path, o_first = 6 * B, 6 * B + tot
        L.check(self.lib.ss_batch_ctc_align(self.h, _stream(), head, B, _ptr(enc_packed), _i32(Tp), _i32(flat or [0]), _i32(n),
                                            _ptr(ibuf), _ptr(ibuf[o_path:]) if want_path else None, _ptr(ibuf[o_first:]),
                                            _ptr(ibuf[o_first + nl:]), _ptr(ibuf[o_first + 2 * nl:])), "ss_batch_ctc_align")
        host = ibuf.cpu().numpy()
        res = host[:6 * B].view(np.dtype([("score", "<f8"), ("viterbi", "<f8"), ("status", "<i4"), ("n_tokens", "<i4")]))
        fl = host.view(np.float32)
        out, r0, l0 = [], 0, 0
        for b in range(B):
            a, z = o_first + l0, o_first + l0 + n[b]
            out.append(CtcAlignment(float(res["score"][b]), float(res["viterbi"][b]), int(res["status"][b]),
                                    host[o_path + r0: o_path + r0 + int(Tp[b])].tolist() if want_path else None,
                                    host[a:z].tolist(), host[a + nl:z + nl].tolist(), fl[a + 2 * nl:z + 2 * nl].copy()))
            r0 += int(Tp[b])
            l0 += n[b]
        return out

    def batch_ctc_spot(self, head: int, enc_packed: torch.Tensor, Tp: List[int], keywords, max_hits: int = 256,
                       return_counts: bool = False):
        """Keyword spotting on a text head (ss_batch_ctc_spot): per utterance the occurrences of the set's phrases (a
        keywords.CtcKeywords over this head's dictionary) as CtcHit tuples, sorted by (end, keyword, start); start and end are
        encoder rows of the utterance, both inclusive.  The rows are packed as batch_ctc_greedy takes them.  No hits for an
        utterance with a NaN row.  At most max_hits per utterance come back (which, past that, is unspecified);
        return_counts: also the count records (n_hits the true number, status, overflow, frames) as a numpy array.  One buffer,
        one device-to-host copy.  The library refuses (SS_ERR_ARG, nothing launched) a set that is not of this head's vocabulary,
        pad and unk, more than L.CTC_ALIGN_MAX_FRAMES frames per utterance and a max_hits outside [1, L.CTC_SPOT_MAX_HITS]."""
        from .keywords import COUNT_DTYPE, HIT_DTYPE, hits_from_records
        B, mh = len(Tp), int(max_hits)
        # int32 words: hits [6 B mh] (four ints and a double each, first: 8-byte aligned) | counts [4 B]
        ibuf = torch.empty((6 * B * max(mh, 0) + 4 * B + 2,), dtype=torch.int32, device=self.device)
        L.check(self.lib.ss_batch_ctc_spot(self.h, _stream(), head, B, _ptr(enc_packed), _i32(Tp), keywords.h, mh, _ptr(ibuf),
                                           _ptr(ibuf[6 * B * max(mh, 0):])), "ss_batch_ctc_spot")
        host = ibuf.cpu().numpy()
        rec = host[:6 * B * mh].view(HIT_DTYPE).reshape(B, mh)
        cnt = host[6 * B * mh: 6 * B * mh + 4 * B].view(COUNT_DTYPE)
        out = [hits_from_records(rec[b, :min(int(cnt["n_hits"][b]), mh)]) for b in range(B)]
        return (out, cnt.copy()) if return_counts else out

    def batch_ctc_beam(self, head: int, enc_packed: torch.Tensor, Tp: List[int], beam: int, cand: Optional[int] = None,
                       nbest: Optional[int] = None, lm=None, lm_weight: float = 0.0, word_score: float = 0.0,
                       lm_eos: bool = True, bias=None, bias_scale: float = 1.0, bias_finish: bool = True) -> List[List[CtcHypothesis]]:
        """CTC prefix beam search on a text head (ss_batch_ctc_beam): per utterance its `nbest` (default: beam) most likely label
        strings, best first, each with the log of the summed probability of its alignments.  The rows are packed as
        batch_ctc_greedy takes them.  Fewer than nbest come back where fewer prefixes are alive, none for an utterance with a NaN
        in a row.  cand: candidates per frame (default ctc_beam_default_cand).  One buffer, one device-to-host copy.  The library
        refuses (SS_ERR_ARG, nothing launched) a beam / cand above L.CTC_BEAM_MAX_BEAM / _CAND, an nbest outside [1, beam] and
        more than L.CTC_BEAM_MAX_FRAMES frames per utterance.
        lm (an ngram.NgramLM over this head's dictionary): shallow fusion (ss_batch_ctc_beam_lm) -- the hypotheses are ranked by
        log p_ctc + lm_weight * log p_lm + word_score * n_tokens, the lm term with the model's </s> when lm_eos, and each carries
        ctc_score and lm_score besides the fused score.  Without lm the call and its tuples are the plain ones.
        bias (a hotwords.CtcBias over this head's dictionary): hotword biasing (ss_batch_ctc_beam_bias), with lm or without --
        bias_scale * (the set's credit for the string) joins the fused score, an unfinished phrase at the end earns nothing when
        bias_finish, and the hypotheses are CtcBiasHypothesis.  Without bias the call and its tuples are what they were."""
        B = len(Tp)
        cand = ctc_beam_default_cand(beam) if cand is None else int(cand)
        nbest = int(beam) if nbest is None else int(nbest)
        stride = max([int(t) for t in Tp] + [1])
        n = B * max(nbest, 0)
        if bias is not None:
            # int32 words: hyps [10 n] (four doubles and two ints each) | tokens [n][stride]
            ibuf = torch.empty((10 * n + n * stride + 1,), dtype=torch.int32, device=self.device)
            opts = C.byref(L.SSCtcLmOpts(float(lm_weight), float(word_score), int(bool(lm_eos)))) if lm is not None else None
            bopts = L.SSCtcBiasOpts(float(bias_scale), int(bool(bias_finish)), 0)
            L.check(self.lib.ss_batch_ctc_beam_bias(self.h, _stream(), head, B, _ptr(enc_packed), _i32(Tp), int(beam), cand, nbest,
                                                    _ptr(ibuf), _ptr(ibuf[10 * n:]), stride, lm.h if lm is not None else None, opts,
                                                    bias.h, C.byref(bopts)), "ss_batch_ctc_beam_bias")
            host = ibuf.cpu().numpy()
            hyp = host[:10 * n].view(_BIAS_HYP)
            return [[CtcBiasHypothesis(host[10 * n + k * stride: 10 * n + k * stride + int(hyp["n_tokens"][k])].tolist(),
                                       float(hyp["score"][k]), float(hyp["ctc_score"][k]),
                                       float(hyp["lm_score"][k]) if lm is not None else None, float(hyp["bias_score"][k]))
                     for k in range(b * nbest, (b + 1) * nbest) if hyp["status"][k] == 0] for b in range(B)]
        if lm is not None:
            # int32 words: hyps [8 n] (three doubles and two ints each) | tokens [n][stride]
            ibuf = torch.empty((8 * n + n * stride + 1,), dtype=torch.int32, device=self.device)
            opts = L.SSCtcLmOpts(float(lm_weight), float(word_score), int(bool(lm_eos)))
            L.check(self.lib.ss_batch_ctc_beam_lm(self.h, _stream(), head, B, _ptr(enc_packed), _i32(Tp), int(beam), cand, nbest,
                                                  _ptr(ibuf), _ptr(ibuf[8 * n:]), stride, lm.h, C.byref(opts)), "ss_batch_ctc_beam_lm")
            host = ibuf.cpu().numpy()
            hyp = host[:8 * n].view(np.dtype([("score", "<f8"), ("ctc_score", "<f8"), ("lm_score", "<f8"), ("n_tokens", "<i4"),
                                              ("status", "<i4")]))
            return [[CtcHypothesis(host[8 * n + k * stride: 8 * n + k * stride + int(hyp["n_tokens"][k])].tolist(),
                                   float(hyp["score"][k]), float(hyp["ctc_score"][k]), float(hyp["lm_score"][k]))
                     for k in range(b * nbest, (b + 1) * nbest) if hyp["status"][k] == 0] for b in range(B)]
        # int32 words: hyps [4 n] (a double and two ints each, first: 8-byte aligned) | tokens [n][stride]
        ibuf = torch.empty((4 * n + n * stride + 1,), dtype=torch.int32, device=self.device)
        L.check(self.lib.ss_batch_ctc_beam(self.h, _stream(), head, B, _ptr(enc_packed), _i32(Tp), int(beam), cand, nbest, _ptr(ibuf),
                                           _ptr(ibuf[4 * n:]), stride), "ss_batch_ctc_beam")
        host = ibuf.cpu().numpy()
        hyp = host[:4 * n].view(np.dtype([("score", "<f8"), ("n_tokens", "<i4"), ("status", "<i4")]))
        out = []
        for b in range(B):
            out.append([CtcHypothesis(host[4 * n + k * stride: 4 * n + k * stride + int(hyp["n_tokens"][k])].tolist(),
                                      float(hyp["score"][k]))
                        for k in range(b * nbest, (b + 1) * nbest) if hyp["status"][k] == 0])
        return out

    def batch_mt_greedy(self, enc_packed: torch.Tensor, Tp: List[int], max_len: List[int], min_len: int = 1):
        """-> (list of token lists incl. final eos, feats [B, Lcap, D], n_feats list)."""
        B = len(Tp)
        Lmax = max(max_len)
        rows, stride = Lmax + 2, Lmax + 1
        feats = torch.empty((B, rows, self.cfg.dec_dim), dtype=torch.float32, device=self.device)
        out = (C.c_int32 * (B * stride))()
        n_out = (C.c_int32 * B)()
        L.check(self.lib.ss_batch_mt_greedy(self.h, _stream(), B, _ptr(enc_packed), _i32(Tp), _i32(max_len), min_len, out,
                                            stride, n_out, _ptr(feats), rows), "ss_batch_mt_greedy")
        toks = [list(out[b * stride: b * stride + n_out[b]]) for b in range(B)]
        return toks, feats, list(n_out)

    def batch_mt_continue(self, enc_packed: torch.Tensor, Tp: List[int], prefixes: List[List[int]], max_len: List[int],
                          min_len: int = 1) -> List[Tuple[List[int], torch.Tensor]]:
        """B independent greedy continuations in one call (ss_batch_mt_continue): row b feeds [</s>, prefixes[b]...] over its
        encoder rows (packed as batch_mt_greedy takes them) and generates up to position max_len[b].  -> per row (tokens after the
        prefix incl. the final eos, decoder states [n_prefix + n_out, D] of the fed positions), as :meth:`HipModel.mt_greedy`."""
        B = len(Tp)
        if not (len(prefixes) == len(max_len) == B):
            raise ValueError("one prefix and one max_len per row")
        plan = plan_mt_continue(Tp, [len(p) for p in prefixes], max_len, min_len, max_tgt_pos=self.max_tgt_pos,
                                prefix_ids=[int(t) for p in prefixes for t in p], vocab=self.cfg.tgt_vocab, eos=self.cfg.eos)
        rows, stride = plan["feat_rows"], plan["out_stride"]
        feats = torch.empty((B, rows, self.cfg.dec_dim), dtype=torch.float32, device=self.device)
        flat = [int(t) for p in prefixes for t in p]
        out = (C.c_int32 * (B * stride))()
        n_out, n_feats = (C.c_int32 * B)(), (C.c_int32 * B)()
        L.check(self.lib.ss_batch_mt_continue(self.h, _stream(), B, _ptr(enc_packed), _i32(Tp), _i32(flat or [0]),
                                              _i32([len(p) for p in prefixes]), _i32(max_len), int(min_len), out, stride, n_out,
                                              _ptr(feats), rows, n_feats), "ss_batch_mt_continue")
        return [(list(out[b * stride: b * stride + n_out[b]]), feats[b, :n_feats[b]]) for b in range(B)]

    def batch_fbank_frames(self, histories: List[torch.Tensor], first: List[int], counts: List[int], outs: List[torch.Tensor],
                           pcm_scale: float = 32768.0):
        """New fbank rows of many 16-kHz streams in one launch (ss_batch_fbank_frames): rows first[i] .. first[i] + counts[i] - 1 of
        the sample history histories[i] (device) into outs[i] ([counts[i], 80] contiguous, device)."""
        B = len(histories)
        if not (len(first) == len(counts) == len(outs) == B) or B == 0:
            raise ValueError("one history, first frame, count and output per session")
        for h, f, n, o in zip(histories, first, counts, outs):
            if n and (h.numel() < (int(f) + int(n) - 1) * 160 + 400 or tuple(o.shape) != (int(n), 80) or not o.is_contiguous()):
                raise ValueError("history shorter than the frames asked for, or a wrong output view")
        pp = (C.c_void_p * B)(*[h.data_ptr() for h in histories])
        fp = (C.c_void_p * B)(*[o.data_ptr() if n else 0 for o, n in zip(outs, counts)])
        L.check(self.lib.ss_batch_fbank_frames(self.h, _stream(), B, pp, _i32(first), _i32(counts), pcm_scale, fp),
                "ss_batch_fbank_frames")

    def batch_fbank_frames_sr(self, histories: List[torch.Tensor], n_in: List[int], rates: List[int], first: List[int],
                              counts: List[int], outs: List[torch.Tensor], pcm_scale: float = 32768.0):
        """batch_fbank_frames for streams at any source rate, each at its own, in one launch (ss_batch_fbank_frames_sr): rows
        first[i] .. first[i] + counts[i] - 1 of fbank_cmvn(resample(histories[i][:n_in[i]], rates[i])) into outs[i] ([counts[i], 80]
        contiguous, device), computed from the source-rate history.  A 16-kHz stream passes through (batch_fbank_frames' bits)."""
        B = len(histories)
        if not (len(n_in) == len(rates) == len(first) == len(counts) == len(outs) == B) or B == 0:
            raise ValueError("one history, sample count, rate, first frame, count and output per session")
        up, down, half, taps = [], [], [], []
        for h, n, sr, c, o in zip(histories, n_in, rates, counts, outs):
            if c and (h.numel() < int(n) or tuple(o.shape) != (int(c), 80) or not o.is_contiguous()):
                raise ValueError("history shorter than the samples named, or a wrong output view")
            u, d, hl = resample_ratio(sr)
            t = self._taps(u, d) if c and u != d else None
            up.append(u); down.append(d); half.append(hl); taps.append(t)
        pp = (C.c_void_p * B)(*[h.data_ptr() for h in histories])
        tp = (C.c_void_p * B)(*[t.data_ptr() if t is not None else 0 for t in taps])
        fp = (C.c_void_p * B)(*[o.data_ptr() if n else 0 for o, n in zip(outs, counts)])
        L.check(self.lib.ss_batch_fbank_frames_sr(self.h, _stream(), B, pp, _i32(n_in), _i32(up), _i32(down), tp, _i32(half),
                                                  _i32(first), _i32(counts), pcm_scale, fp), "ss_batch_fbank_frames_sr")

    def pcm_scatter(self, stage: torch.Tensor, stage_bytes: int, segs, dsts: List[torch.Tensor]):
        """Every raw PCM chunk of a step, lying in the device staging tensor `stage`, decoded into the float32 histories `dsts` in
        one launch (ss_pcm_scatter; pcm.scatter names the segment tuple)."""
        from . import pcm
        pcm.scatter(self.lib, _stream(), stage, stage_bytes, segs, dsts)

    def mp3_stream_decode(self, arena, items):
        """The new granules of every MP3-fed session of a step (mp3.decode_stream_batch names the item tuple): one upload of the
        arena, one ss_mp3_stream_synthesize, mono.  -> (granule-channels decoded, bytes uploaded)."""
        from . import mp3
        return mp3.decode_stream_batch(arena, items, True, self.lib)

    def pcm_pack_s16(self, src: torch.Tensor, out: torch.Tensor):
        """float32 device samples -> 16-bit PCM on the device, one launch (ss_pcm_pack_s16)."""
        from . import pcm
        pcm.pack_s16(self.lib, _stream(), src, out)

    def pcm_taps(self, up: int, down: int) -> torch.Tensor:
        """The device tap table of the ratio up / down, made once and shared with resample()."""
        return self._taps(up, down)

    def pcm_emit(self, segs, out: torch.Tensor):
        """The speech of every session of a step that answers at its own rate and format: resampled from each one's carried history
        and new tail, encoded, into the uint8 device tensor `out` (ss_pcm_emit; pcm.emit_plan names the segment tuple)."""
        from . import pcm
        pcm.emit(self.lib, _stream(), segs, out)

    def vad_scan(self, segs, results: torch.Tensor):
        """The endpoint scan of every endpointed session of a step, one launch (ss_vad_scan; endpoint.seg_table names the segment
        tuple): each session's device state record is rewritten and its result record goes to row i of the uint8 device tensor
        `results` [n, 40]."""
        from . import endpoint
        endpoint.scan(self.lib, _stream(), segs, results)

    def fbank_sr_rows(self, n_in: int, sr_in: int) -> Optional[Tuple[int, int]]:
        """(fbank rows, final fbank rows) of n_in samples at sr_in Hz (fbank_sr_rows); None for a rate batch_fbank_frames_sr refuses."""
        return fbank_sr_rows(n_in, *resample_ratio(sr_in), lib=self.lib)

    def _mt_beam(self, entry: str, enc_packed: torch.Tensor, Tp: List[int], prefixes: Optional[List[List[int]]], max_len: List[int],
                 beam: int, spare_rows: int, min_len: int, unk_penalty: float, normalize: bool, search: tuple, sample=None,
                 constraints=None):
        """The calls behind batch_mt_beam (prefixes None: `entry` takes none) and batch_mt_beam_continue -> (nbest, feats [B, rows, D]),
        rows = the longest max_len + 1 + spare_rows.  A pack with B * beam > 256 rows runs as consecutive sub-calls (plan_beam_groups).
        search = (len_penalty, temperature, no_repeat_ngram_size): at the defaults the call is `entry` itself, otherwise `entry`_opts.
        A hypothesis is its row's prefix + the generated tokens, and its positional scores cover both.
        sample = (keys, ss_mt_sample_opts): the sampling twin of `entry` (ss_batch_mt_sample / _continue), `beam` chains per row.
        constraints = per-row phrase lists: ss_batch_mt_beam_cons (the search options always travel with it, NULL at the defaults)."""
        B = len(Tp)
        if constraints is not None and (prefixes is not None or sample is not None):
            raise ValueError("constraints go with the offline beam search only, not behind a forced prefix and not with sampling")
        if not 1 <= beam <= MT_BEAM_MAX:
            raise ValueError(f"beam {beam} outside [1, {MT_BEAM_MAX}]")
        opts = check_search_options(*search)
        name, tail = (entry, ()) if opts is None else (entry + "_opts", (C.byref(opts),))
        if sample is not None:
            name = entry.replace("_beam", "_sample")
            if len(sample[0]) != B:
                raise ValueError("one key per row")
        if constraints is not None:
            L.pack_constraints(constraints, B)       # an empty phrase or a wrong count is refused before anything is booked
            name = "ss_batch_mt_beam_cons"
        stride = max(max_len) + 1
        rows = stride + spare_rows
        feats = torch.empty((B, rows, self.cfg.dec_dim), dtype=torch.float32, device=self.device)
        nbest: List[List[dict]] = []
        off = np.concatenate([[0], np.cumsum(Tp)]).astype(np.int64)
        for b0, b1 in plan_beam_groups(B, beam):
            n = b1 - b0
            enc = enc_packed[int(off[b0]):int(off[b1])]
            pre = [[int(t) for t in p] for p in prefixes[b0:b1]] if prefixes is not None else [[]] * n
            forced = () if prefixes is None else (_i32([t for p in pre for t in p] or [0]), _i32([len(p) for p in pre]))
            out = (C.c_int32 * (n * beam * stride))()
            n_out = (C.c_int32 * (n * beam))()
            sc = (C.c_float * (n * beam))()
            pos = (C.c_float * (n * beam * stride))()
            if sample is not None:
                keys = (C.c_int64 * n)(*[_as_i64(x) for x in sample[0][b0:b1]])
                tail = (C.byref(opts) if opts is not None else None, keys, C.byref(sample[1]))
            if constraints is not None:
                tail = (C.byref(opts) if opts is not None else None,) + tuple(_i32(a) for a in L.pack_constraints(constraints[b0:b1], n))
            L.check(getattr(self.lib, name)(self.h, _stream(), n, beam, _ptr(enc), _i32(Tp[b0:b1]), *forced, _i32(max_len[b0:b1]),
                                            int(min_len), float(unk_penalty), 1 if normalize else 0, out, stride, n_out, sc, pos,
                                            _ptr(feats[b0:b1]), rows, *tail), name)
            for b in range(n):
                hyps = []
                for i in range(beam):
                    o = b * beam + i
                    k = n_out[o]
                    if k <= 0:
                        continue
                    hyps.append({"tokens": pre[b] + list(out[o * stride: o * stride + k]), "score": float(sc[o]),
                                 "positional_scores": list(pos[o * stride: o * stride + len(pre[b]) + k])})
                nbest.append(hyps)
        return nbest, feats

    def batch_mt_beam(self, enc_packed: torch.Tensor, Tp: List[int], max_len: List[int], beam: int, min_len: int = 1,
                      unk_penalty: float = 0.0, normalize: bool = True, len_penalty: float = 1.0, temperature: float = 1.0,
                      no_repeat_ngram_size: int = 0, constraints: Optional[List[List[List[int]]]] = None):
        """Beam search of the first-pass text decoder (ss_batch_mt_beam) -> (n-best lists, feats [B, Lcap, D], n_feats list).
        nbest[b] holds up to `beam` dicts {"tokens" (incl. final eos), "score", "positional_scores"} in the reference's final order;
        feats / n_feats are the decoder states of hypothesis 0, as batch_mt_greedy returns them.  A pack with B * beam > 256 rows
        runs as consecutive sub-calls (plan_beam_groups); pack-invariant arithmetic makes the split invisible.  len_penalty,
        temperature and no_repeat_ngram_size are the reference's --lenpen, --temperature and --no-repeat-ngram-size
        (ss_mt_search_opts); at their defaults the call is ss_batch_mt_beam itself.  constraints[b] is a list of phrases (token id
        lists) that every hypothesis of row b must contain in that order (the reference's --constraints, ordered;
        ss_batch_mt_beam_cons); None, or no phrase anywhere, is exactly the call without them."""
        if constraints is not None and not any(len(c or []) for c in constraints):
            if len(constraints) != len(Tp):
                raise ValueError("one constraint list per row")
            constraints = None
        nbest, feats = self._mt_beam("ss_batch_mt_beam", enc_packed, Tp, None, max_len, beam, 1, min_len, unk_penalty, normalize,
                                     (len_penalty, temperature, no_repeat_ngram_size), constraints=constraints)
        return nbest, feats, [len(h[0]["tokens"]) if h else 0 for h in nbest]

    def batch_mt_beam_continue(self, enc_packed: torch.Tensor, Tp: List[int], prefixes: List[List[int]], max_len: List[int], beam: int,
                               min_len: int = 1, unk_penalty: float = 0.0, normalize: bool = True, len_penalty: float = 1.0,
                               temperature: float = 1.0, no_repeat_ngram_size: int = 0):
        """Beam search behind a forced prefix per row (ss_batch_mt_beam_continue; fairseq's ``prefix_tokens`` of the offline generator)
        -> (nbest, feats).  nbest[b] holds up to `beam` dicts, best first: "tokens" is the FULL hypothesis (prefixes[b] + generated,
        incl. the final eos), "score" and "positional_scores" cover it whole.  feats[b] = decoder states [n_prefix_b + n_generated_b, D]
        of hypothesis 0's fed positions, as batch_mt_continue returns them.  A pack with B * beam > 256 rows runs as consecutive
        sub-calls (plan_beam_groups); pack-invariant arithmetic makes the split invisible.  len_penalty, temperature and
        no_repeat_ngram_size as in batch_mt_beam (ss_batch_mt_beam_continue_opts); a prefix that itself repeats an n-gram is refused."""
        if not (len(prefixes) == len(max_len) == len(Tp)):
            raise ValueError("one prefix and one max_len per row")
        nbest, feats = self._mt_beam("ss_batch_mt_beam_continue", enc_packed, Tp, prefixes, max_len, beam, 0, min_len, unk_penalty,
                                     normalize, (len_penalty, temperature, no_repeat_ngram_size))
        return nbest, [feats[b, :len(h[0]["tokens"]) if h else 0] for b, h in enumerate(nbest)]

    def batch_mt_sample(self, enc_packed: torch.Tensor, Tp: List[int], max_len: List[int], n_samples: int, keys: List[int],
                        topk: int = 0, topp: float = 0.0, seed: int = 1, min_len: int = 1, unk_penalty: float = 0.0,
                        normalize: bool = True, len_penalty: float = 1.0, temperature: float = 1.0, no_repeat_ngram_size: int = 0):
        """n_samples independent ancestral samples per row from the first-pass text decoder (ss_batch_mt_sample; the rule stands in
        the header at ss_mt_sample_opts) -> what batch_mt_beam returns, every list holding exactly n_samples entries ordered by
        score.  keys[b] is the row's 64-bit stream key: with `seed` it fixes the row's samples whatever else is in the pack."""
        so = check_sampling_options(topk, topp, seed, self.cfg.tgt_vocab)
        nbest, feats = self._mt_beam("ss_batch_mt_beam", enc_packed, Tp, None, max_len, n_samples, 1, min_len, unk_penalty, normalize,
                                     (len_penalty, temperature, no_repeat_ngram_size), sample=(list(keys), so))
        return nbest, feats, [len(h[0]["tokens"]) if h else 0 for h in nbest]

    def batch_mt_sample_continue(self, enc_packed: torch.Tensor, Tp: List[int], prefixes: List[List[int]], max_len: List[int],
                                 n_samples: int, keys: List[int], topk: int = 0, topp: float = 0.0, seed: int = 1, min_len: int = 1,
                                 unk_penalty: float = 0.0, normalize: bool = True, len_penalty: float = 1.0, temperature: float = 1.0,
                                 no_repeat_ngram_size: int = 0):
        """batch_mt_sample behind a forced prefix per row (ss_batch_mt_sample_continue) -> what batch_mt_beam_continue returns."""
        if not (len(prefixes) == len(max_len) == len(Tp)):
            raise ValueError("one prefix and one max_len per row")
        so = check_sampling_options(topk, topp, seed, self.cfg.tgt_vocab)
        nbest, feats = self._mt_beam("ss_batch_mt_beam_continue", enc_packed, Tp, prefixes, max_len, n_samples, 0, min_len,
                                     unk_penalty, normalize, (len_penalty, temperature, no_repeat_ngram_size),
                                     sample=(list(keys), so))
        return nbest, [feats[b, :len(h[0]["tokens"]) if h else 0] for b, h in enumerate(nbest)]

    def last_logits(self) -> torch.Tensor:
        """Dense logits [rows, cols] of this context's last batch_ctc_greedy / batch_t2u_units call (test hook: arg-max margins)."""
        rows, cols = C.c_int(0), C.c_int(0)
        L.check(self.lib.ss_debug_last_logits(self.h, _stream(), None, 0, C.byref(rows), C.byref(cols)), "ss_debug_last_logits")
        out = torch.empty((rows.value, cols.value), dtype=torch.float32, device=self.device)
        L.check(self.lib.ss_debug_last_logits(self.h, _stream(), _ptr(out), out.numel(), C.byref(rows), C.byref(cols)), "ss_debug_last_logits")
        return out

    def batch_t2u_units(self, feats: torch.Tensor, n_rows: List[int], t2u_causal=False, mask_eos=False,
                        return_raw: bool = False, keep_raw: bool = False):
        """feats [B, rows, D] (rows of utterance b used: n_rows[b]) -> list of collapsed unit-vocab token lists
        (with return_raw: (collapsed lists, raw per-position argmax lists)).  keep_raw: the packed DEVICE arg-max ids (int32
        [ctc_upsample * sum n_rows], what :meth:`batch_unit_spans` reads) follow as one more element of the answer."""
        B, rows = feats.shape[0], feats.shape[1]
        up = self.cfg.ctc_upsample
        U = sum(n_rows) * up
        ibuf = torch.empty((2 * U + B,), dtype=torch.int32, device=self.device)
        raw, toks, cnt = ibuf[:U], ibuf[U:2 * U], ibuf[2 * U:]
        L.check(self.lib.ss_batch_t2u_units(self.h, _stream(), B, _ptr(feats), rows, _i32(n_rows), int(t2u_causal),
                                            int(mask_eos), _ptr(raw), _ptr(toks), _ptr(cnt)), "ss_batch_t2u_units")
        host = ibuf.cpu().numpy()
        out, raws, off = [], [], 0
        for b in range(B):
            k = int(host[2 * U + b])
            out.append(host[U + off: U + off + k].tolist())
            raws.append(host[off: off + n_rows[b] * up].tolist())
            off += n_rows[b] * up
        if keep_raw:
            return (out, raws, raw) if return_raw else (out, raw)
        return (out, raws) if return_raw else out

    def batch_t2u_units_pad(self, feats: torch.Tensor, n_rows: List[int], n_tail_pad: List[int], t2u_causal=False, mask_eos=False,
                            return_raw: bool = False, keep_raw: bool = False):
        """:meth:`batch_t2u_units` with trailing <pad> states (ss_batch_t2u_units_pad): the last n_tail_pad[b] of row b's n_rows[b]
        states are masked as keys, as :meth:`HipModel.t2u_units` (..., n_tail_pad) masks them; they are still decoded.  keep_raw as
        there."""
        B, rows = feats.shape[0], feats.shape[1]
        if len(n_rows) != B or len(n_tail_pad) != B:
            raise ValueError("one row count and one tail pad per row")
        up = self.cfg.ctc_upsample
        U = sum(n_rows) * up
        ibuf = torch.empty((2 * U + B,), dtype=torch.int32, device=self.device)
        raw, toks, cnt = ibuf[:U], ibuf[U:2 * U], ibuf[2 * U:]
        L.check(self.lib.ss_batch_t2u_units_pad(self.h, _stream(), B, _ptr(feats), rows, _i32(n_rows), _i32(n_tail_pad),
                                                int(t2u_causal), int(mask_eos), _ptr(raw), _ptr(toks), _ptr(cnt)),
                "ss_batch_t2u_units_pad")
        host = ibuf.cpu().numpy()
        out, raws, off = [], [], 0
        for b in range(B):
            k = int(host[2 * U + b])
            out.append(host[U + off: U + off + k].tolist())
            raws.append(host[off: off + n_rows[b] * up].tolist())
            off += n_rows[b] * up
        if keep_raw:
            return (out, raws, raw) if return_raw else (out, raw)
        return (out, raws) if return_raw else out

    def batch_unit_spans(self, raw: torch.Tensor, n_states: List[int], K: List[int], dur, dur_first: Optional[List[int]] = None,
                         unit0: Optional[List[int]] = None) -> List[np.ndarray]:
        """Where each text-decoder state is spoken (ss_batch_unit_spans): raw = the device arg-max ids a t2u call kept (keep_raw),
        n_states[b] / K[b] the states and the units of row b, dur the durations of the vocoder call that spoke them -- a DEVICE
        int32 tensor packed [sum K] (HipVocoder.forward / batch_forward) or per row a host sequence of the durations of units
        dur_first[b] .. K[b] (HipVocoder.batch_tail's info) -- and unit0[b] the first NEW unit (both default to 0).  -> per row an
        int32 [n, 4] array {first_unit, n_units, start_frame, n_frames} over the new units; one launch, one download.  A row whose
        units the kernel counts differently from K[b] raises with the row's number."""
        B = len(n_states)
        d0 = [0] * B if dur_first is None else [int(x) for x in dur_first]
        u0 = [0] * B if unit0 is None else [int(x) for x in unit0]
        if not (len(K) == len(d0) == len(u0) == B):
            raise ValueError("one state count, unit count, first duration and first new unit per row")
        if raw.dtype != torch.int32 or not raw.is_contiguous() or raw.numel() < self.cfg.ctc_upsample * sum(int(n) for n in n_states):
            raise ValueError("raw: the contiguous int32 arg-max ids of all rows")
        d_dur = h_dur = None
        if torch.is_tensor(dur):
            if dur.dtype != torch.int32 or not dur.is_contiguous() or dur.numel() < sum(int(k) for k in K):
                raise ValueError("dur: a contiguous int32 tensor with one duration per unit")
            d_dur = dur if dur.numel() else torch.zeros((1,), dtype=torch.int32, device=raw.device)
        else:
            if len(dur) != B:
                raise ValueError("dur: one sequence of durations per row")
            h_dur = np.zeros((max(sum(int(k) for k in K), 1),), dtype=np.int32)
            off = 0
            for b in range(B):
                m = int(K[b]) - d0[b]
                if len(dur[b]) < m:
                    raise ValueError(f"row {b}: {len(dur[b])} durations for units {d0[b]} .. {int(K[b])}")
                h_dur[off: off + m] = np.asarray(dur[b][:m], dtype=np.int32) if m > 0 else 0
                off += int(K[b])
        spans = np.empty((sum(int(n) for n in n_states), 4), dtype=np.int32)
        counted = np.empty((B,), dtype=np.int32)
        L.check(self.lib.ss_batch_unit_spans(self.h, _stream(), B, _ptr(raw), _i32(n_states), _i32(K), _i32(d0), _i32(u0), _ptr(d_dur),
                                             None if h_dur is None else h_dur.ctypes.data_as(C.c_void_p),
                                             spans.ctypes.data_as(C.c_void_p), counted.ctypes.data_as(C.c_void_p)),
                "ss_batch_unit_spans")
        out, off = [], 0
        for b in range(B):
            if int(counted[b]) != int(K[b]):
                raise L.StreamSpeechHipError(f"ss_batch_unit_spans: row {b} holds {int(counted[b])} units, the caller counted {int(K[b])}")
            out.append(spans[off: off + int(n_states[b])])
            off += int(n_states[b])
        return out

    def batch_mt_features(self, enc_packed: torch.Tensor, Tp: List[int], tokens: List[List[int]], n_tail_pad: List[int]) -> List[torch.Tensor]:
        """Decoder states of B fed rows in one ragged pass (ss_batch_mt_features): row b feeds [</s>, tokens[b]..., <pad> x
        n_tail_pad[b]] over its encoder rows (packed as batch_mt_continue takes them).  -> per row the post-LN states [n_b, D] of every
        fed position, as mt_truncate + mt_append(..., n_tail_pad) give them."""
        B = len(Tp)
        if not (len(tokens) == len(n_tail_pad) == B) or B == 0:
            raise ValueError("one token list and one tail pad per row")
        n = [1 + len(t) + int(p) for t, p in zip(tokens, n_tail_pad)]
        rows = max(n)
        feats = torch.empty((B, rows, self.cfg.dec_dim), dtype=torch.float32, device=self.device)
        flat = [int(t) for ts in tokens for t in ts]
        L.check(self.lib.ss_batch_mt_features(self.h, _stream(), B, _ptr(enc_packed), _i32(Tp), _i32(flat or [0]),
                                              _i32([len(t) for t in tokens]), _i32(n_tail_pad), _ptr(feats), rows),
                "ss_batch_mt_features")
        return [feats[b, :n[b]] for b in range(B)]

    def batch_mt_attention(self, enc_packed: torch.Tensor, Tp: List[int], tokens: List[List[int]], first: Optional[List[int]] = None,
                           want_matrix: bool = True, want_feats: bool = False):
        """Head-averaged cross-attention of the last MT decoder layer in one ragged teacher-forced pass (ss_batch_mt_attention): row b
        feeds [</s>, tokens[b]...] over its encoder rows (packed as batch_mt_continue takes them) and answers the fed positions
        first[b] .. len(tokens[b]) (position p is the decoder input that predicts token p; first None: every position).
        -> per row ``(attn, peak, peak_prob, mean_pos, feats)``: attn float32 [rows, Tp[b]] on the host (None without want_matrix:
        nothing of that size is written or copied), peak int32 [rows] the arg-max source frame of every position, peak_prob float32
        [rows] its probability, mean_pos float32 [rows] = sum_j j * attn[., j]; feats (want_feats) the post-LN decoder states
        [1 + len(tokens[b]), D] on the device, the bits batch_mt_features(..., n_tail_pad = 0) gives, else None.  One device-to-host
        copy per call.  Rewrites the scratch set's MT cross-attention K/V and workspace, as batch_mt_features does."""
        B = len(Tp)
        if len(tokens) != B or B == 0 or (first is not None and len(first) != B):
            raise ValueError("one token list (and one first position) per row")
        first = [0] * B if first is None else [int(f) for f in first]
        n_tok = [len(t) for t in tokens]
        rows = [n_tok[b] + 1 - first[b] for b in range(B)]
        if any(r <= 0 for r in rows) or any(f < 0 for f in first):
            raise ValueError("first[b] must lie in [0, len(tokens[b])]")
        R = sum(rows)
        n_attn = sum(r * int(t) for r, t in zip(rows, Tp)) if want_matrix else 0
        # one buffer, one copy: attn | stat [R][2] | peak [R] (int32 bits)
        buf = torch.empty((n_attn + 3 * R,), dtype=torch.float32, device=self.device)
        d_attn, d_stat, d_peak = buf[:n_attn], buf[n_attn:n_attn + 2 * R], buf[n_attn + 2 * R:]
        feats, frows = None, 0
        if want_feats:
            frows = max(n_tok) + 1
            feats = torch.empty((B, frows, self.cfg.dec_dim), dtype=torch.float32, device=self.device)
        off = (C.c_int64 * B)()
        flat = [int(t) for ts in tokens for t in ts]
        L.check(self.lib.ss_batch_mt_attention(self.h, _stream(), B, _ptr(enc_packed), _i32(Tp), _i32(flat or [0]), _i32(n_tok),
                                               _i32(first), _ptr(feats) if want_feats else None, frows,
                                               _ptr(d_attn) if want_matrix else None, off, n_attn, _ptr(d_peak), _ptr(d_stat)),
                "ss_batch_mt_attention")
        host = buf.cpu()
        stat = host[n_attn:n_attn + 2 * R].view(R, 2)
        peak = host[n_attn + 2 * R:].view(torch.int32)
        out, r0 = [], 0
        for b in range(B):
            n = rows[b]
            attn = host[int(off[b]):int(off[b]) + n * int(Tp[b])].view(n, int(Tp[b])) if want_matrix else None
            out.append((attn, peak[r0:r0 + n], stat[r0:r0 + n, 0], stat[r0:r0 + n, 1],
                        feats[b, :n_tok[b] + 1] if want_feats else None))
            r0 += n
        return out

    def batch_mt_score(self, enc_packed: torch.Tensor, Tp: List[int], tokens: List[List[int]], src: Optional[List[int]] = None,
                       want_feats: bool = False) -> List[dict]:
        """How likely the first-pass text decoder finds each GIVEN text, in one ragged teacher-forced pass (ss_batch_mt_score;
        fairseq's SequenceScorer): row b feeds [</s>, tokens[b]...] (tokens without </s>) over the encoder rows of utterance src[b]
        of the U = len(Tp) packed utterances (src None: one text per utterance, in order; several rows may name one utterance).
        -> per row a dict: ``positional_scores`` float32 [n + 1] -- the natural-log probability of tokens[b][p] at position p and of
        </s> at the last one, under the plain log_softmax (no pad / unk masking) -- ``score`` = their sum / (n + 1) (</s> counted, as
        SequenceScorer forms it), ``best`` int32 [n + 1] the decoder's own arg-max at every position, ``best_lprob`` float32 [n + 1]
        its log-probability, ``rank`` int32 [n + 1] the given token's rank (0: the decoder would have chosen it), ``feats``
        (want_feats) the post-LN decoder states [n + 1, D] on the device, the bits batch_mt_features(..., n_tail_pad = 0) gives, else
        None.  One device-to-host copy per call.  Rewrites the scratch set's MT cross-attention K/V and workspace, as
        batch_mt_features does."""
        U, B = len(Tp), len(tokens)
        if U == 0 or B == 0 or (src is None and B != U) or (src is not None and len(src) != B):
            raise ValueError("one text per utterance, or one utterance index per text")
        n_tok = [len(t) for t in tokens]
        R = sum(n_tok) + B
        buf = torch.empty((4 * R,), dtype=torch.float32, device=self.device)      # stat [R][2] | idx [R][2] (int32 bits): one copy
        d_stat, d_idx = buf[:2 * R], buf[2 * R:]
        feats, frows = None, 0
        if want_feats:
            frows = max(n_tok) + 1
            feats = torch.empty((B, frows, self.cfg.dec_dim), dtype=torch.float32, device=self.device)
        flat = [int(t) for ts in tokens for t in ts]
        L.check(self.lib.ss_batch_mt_score(self.h, _stream(), U, _ptr(enc_packed), _i32(Tp), B,
                                           _i32([int(s) for s in src]) if src is not None else None, _i32(flat or [0]), _i32(n_tok),
                                           _ptr(feats) if want_feats else None, frows, _ptr(d_stat), _ptr(d_idx)),
                "ss_batch_mt_score")
        host = buf.cpu()
        stat, idx = host[:2 * R].view(R, 2), host[2 * R:].view(torch.int32).view(R, 2)
        out, r0 = [], 0
        for b in range(B):
            n = n_tok[b] + 1
            pos = stat[r0:r0 + n, 0].contiguous()
            out.append({"positional_scores": pos, "score": float(pos.double().sum()) / n, "best": idx[r0:r0 + n, 0].contiguous(),
                        "best_lprob": stat[r0:r0 + n, 1].contiguous(), "rank": idx[r0:r0 + n, 1].contiguous(),
                        "feats": feats[b, :n] if want_feats else None})
            r0 += n
        return out


class Scratch:
    """One scratch set (ss_scratch: activations, KV caches, stream-K hand-off state, streaming-encoder state) -- everything a call
    mutates.  One per concurrent stream; weight handles of any language (HipModel / HipVocoder) are bound to it with
    `handle.bind_scratch(scratch)` or at construction (`scratch=`).  Driven by one host thread at a time."""

    def __init__(self, device="cuda:0", cap_bytes: int = 0):
        self.lib = L.load()
        self.device = _require_gpu(device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_scratch_create(C.byref(h)), "ss_scratch_create")
        self.h = h
        if cap_bytes:
            self.set_cap(cap_bytes)

    def set_cap(self, max_bytes: int):
        L.check(self.lib.ss_scratch_set_cap(self.h, int(max_bytes)), "ss_scratch_set_cap")

    def trim(self, keep_bytes: int = 0):
        """Synchronises the device and releases the re-sizable buffers, largest first, until at most keep_bytes are held.  A streaming
        sequence on the set starts over (a deferred time-out check still outstanding is settled first)."""
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_scratch_trim(self.h, int(keep_bytes)), "ss_scratch_trim")

    def bytes(self) -> int:
        return int(self.lib.ss_scratch_bytes(self.h))

    def audit(self) -> Tuple[int, int]:
        """Test hook: (bytes booked, bytes the set's buffers hold) -- equal when the set keeps its books; raises if a buffer of the
        set is booked under another account (ss_debug_scratch_audit)."""
        booked, held = C.c_size_t(0), C.c_size_t(0)
        L.check(self.lib.ss_debug_scratch_audit(self.h, C.byref(booked), C.byref(held)), "ss_debug_scratch_audit")
        return int(booked.value), int(held.value)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ss_scratch_destroy(self.h)
                self.h = None
        except Exception:
            pass


class HipModel(BatchMixin):
    """ss_model handle + packed weights (StreamSpeechModel replacement)."""

    def __init__(self, state_dict, cfg: ModelConfig = None, device="cuda:0", cmvn_mean=None, cmvn_std=None,
                 max_rel_pos: int = 2048, max_tgt_pos: int = 1026, _share=None, scratch: "Scratch" = None):
        self.lib = L.load()
        self.cfg = cfg or ModelConfig()
        self.device = _require_gpu(device)
        if _share is not None:      # another execution context over the same (read-only) weight blob
            names, offsets, numels, self.blob = _share
        else:
            names, offsets, numels, blob = pack_model(state_dict, self.cfg, cmvn_mean, cmvn_std, max_rel_pos, max_tgt_pos)
            self.blob = blob.to(self.device)
        self._packed = (names, offsets, numels, self.blob)
        self._dims = (max_rel_pos, max_tgt_pos)
        c = self.cfg
        self.c_cfg = L.SSConfig(
            c.input_feat, c.conv_channels, c.conv_kernel, c.enc_dim, c.enc_ffn, c.enc_heads, c.enc_layers,
            c.dw_kernel, c.src_vocab, c.tgt_vocab, c.mt_layers, c.dec_dim, c.dec_ffn, c.dec_heads, c.t2u_layers,
            c.unit_layers, c.unit_vocab, c.ctc_upsample, c.pad, c.eos, c.unk, max_rel_pos, max_tgt_pos)
        cn, co, cm, n = _slots(names, offsets, numels)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_model_create(C.byref(self.c_cfg), _ptr(self.blob), self.blob.numel(), cn, co, cm, n,
                                             C.byref(h)), "ss_model_create")
        self.h = h
        self.scratch = None                 # None: the handle's own scratch set (made by ss_model_create)
        if scratch is not None:
            self.bind_scratch(scratch)
        self.max_tgt_pos = max_tgt_pos
        # MT decode step of single-utterance searches (ss_mt_greedy / ss_mt_append with one token): the C ABI's default is the
        # launch-per-op form (SS_MT_PERSISTENT overrides it); a PRIMARY context -- the one an agent / the offline driver / a
        # one-utterance-at-a-time caller decodes on, alone on its device -- uses the persistent one-launch step (mt_step.hip:
        # 125 vs 189 us per token).  Contexts made by new_context() exist for concurrency and keep the launch-per-op form; a
        # time-out of the persistent step (its workgroups were not all resident) falls back to it for good and says so.
        self.persistent_mt = int(self.lib.ss_mt_get_persistent(self.h))
        if _share is None and scratch is None and "SS_MT_PERSISTENT" not in os.environ:     # (a handle made ON a shared scratch set is a concurrent one)
            self.set_persistent_mt_step(64)

    def new_context(self, scratch: "Scratch" = None) -> "HipModel":
        """Another ss_model handle borrowing the same weights -- on its own scratch set, or on `scratch` (a set shared with the
        handles of other languages on the same stream): one per concurrent utterance stream.  (Concurrent contexts start with the
        launch-per-op MT decode step: the persistent step's workgroups must all be resident, which only a context that decodes
        alone on the device can count on.)"""
        return HipModel(None, self.cfg, device=str(self.device), max_rel_pos=self._dims[0],
                        max_tgt_pos=self._dims[1], _share=self._packed, scratch=scratch)

    def bind_scratch(self, scratch: "Scratch"):
        """Run this handle on `scratch` from now on (between stateful sequences only: mt_begin ... mt_append and the streaming
        encoder keep their state in the scratch set; a streaming sequence on the set the handle leaves ends here)."""
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_model_bind_scratch(self.h, scratch.h), "ss_model_bind_scratch")
        self.scratch = scratch
        if hasattr(self, "persistent_mt"):      # the MT decode-step form is a setting of the scratch set (its granule region lives there)
            self.persistent_mt = int(self.lib.ss_mt_get_persistent(self.h))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ss_model_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ---- waveform front-end (§8f-3) --------------------------------------------------------
    def _taps(self, up: int, down: int) -> torch.Tensor:
        """design_filter(up, down) on the device, float32, made once per ratio."""
        from .frontend import design_filter
        cache = self.__dict__.setdefault("_resample_taps", {})
        if (up, down) not in cache:
            cache[(up, down)] = torch.from_numpy(design_filter(up, down).astype(np.float32)).to(self.device)
        return cache[(up, down)]

    def resample(self, pcm: torch.Tensor, sr_in: int, sr_out: int = 16000) -> torch.Tensor:
        """float32 [n] on the device at sr_in -> [ceil(n*sr_out/sr_in)] at sr_out (polyphase FIR kernel)."""
        up, down, _ = resample_ratio(sr_in, sr_out)
        if up == down:
            return pcm
        taps = self._taps(up, down)
        n_in = pcm.numel()
        n_out = -(-n_in * up // down)
        out = torch.empty((n_out,), dtype=torch.float32, device=self.device)
        L.check(self.lib.ss_resample(_stream(), _ptr(pcm), n_in, up, down, _ptr(taps), (taps.numel() - 1) // 2,
                                     _ptr(out), n_out), "ss_resample")
        return out

    # ---- a1 -------------------------------------------------------------------------------
    def fbank_cmvn(self, pcm16k: torch.Tensor, pcm_scale: float = 32768.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pcm16k: float32 [n] on the device -> [T, 80] (into ``out`` -- T contiguous rows -- when given)."""
        n = pcm16k.numel()
        T = self.lib.ss_fbank_num_frames(n)
        if out is not None:
            assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (T, 80)
        feat = out if out is not None else torch.empty((T, 80), dtype=torch.float32, device=self.device)
        nf = C.c_int(0)
        L.check(self.lib.ss_fbank_cmvn(self.h, _stream(), _ptr(pcm16k), n, pcm_scale, _ptr(feat), C.byref(nf)),
                "ss_fbank_cmvn")
        return feat

    # ---- a2-a7 ----------------------------------------------------------------------------
    def encoder_out_len(self, T: int) -> int:
        return self.lib.ss_encoder_out_len(T)

    def encoder_forward(self, fbank: torch.Tensor, attn_chunk: int = 999999, conv_chunk: int = 999999) -> torch.Tensor:
        """fbank [T,80] (device, contiguous) -> [T',256]."""
        assert fbank.is_cuda and fbank.dtype == torch.float32 and fbank.is_contiguous()
        T = fbank.shape[0]
        Tp = self.lib.ss_encoder_out_len(T)
        out = torch.empty((Tp, self.cfg.enc_dim), dtype=torch.float32, device=self.device)
        L.check(self.lib.ss_encoder_forward(self.h, _stream(), _ptr(fbank), T, int(min(attn_chunk, 1 << 30)),
                                            int(min(conv_chunk, 1 << 30)), _ptr(out)), "ss_encoder_forward")
        self._last_enc, self._ctc_stash, self._ctc_both = (out.data_ptr(), Tp), None, None
        return out

    def encoder_stream_reset(self):
        """Forget the incremental-encoder cache (new utterance)."""
        L.check(self.lib.ss_encoder_stream_reset(self.h), "ss_encoder_stream_reset")
        self.stream_stats = (0, 0)

    def encoder_stream_set_tail(self, unsettled_fbank_frames: int):
        """Newest fbank frames that may still change on the next call (1 when the front-end resamples, else 0)."""
        L.check(self.lib.ss_encoder_stream_set_tail(self.h, int(unsettled_fbank_frames)), "ss_encoder_stream_set_tail")

    def encoder_stream_forward(self, fbank: torch.Tensor, attn_chunk: int, conv_chunk: int) -> torch.Tensor:
        """Incremental twin of :meth:`encoder_forward` for streaming: same input (fbank
        of all audio so far) and output, but only the rows that are not final yet are recomputed.
        ``self.stream_stats`` = (rows final after the call, rows recomputed by it)."""
        assert fbank.is_cuda and fbank.dtype == torch.float32 and fbank.is_contiguous()
        T = fbank.shape[0]
        Tp = self.lib.ss_encoder_out_len(T)
        out = torch.empty((Tp, self.cfg.enc_dim), dtype=torch.float32, device=self.device)
        nf, nc = C.c_int32(0), C.c_int32(0)

        def forward():
            L.check(self.lib.ss_encoder_stream_forward(self.h, _stream(), _ptr(fbank), T, int(min(attn_chunk, 1 << 30)),
                                                       int(min(conv_chunk, 1 << 30)), _ptr(out), C.byref(nf), C.byref(nc)),
                    "ss_encoder_stream_forward")
        self._ctc_stash = None
        if self.ctc_speculate and self.persistent_mt > 0 and Tp > 0 and not os.environ.get("SS_NO_CTC_DEFER"):
            # The agents' policy() reads both CTC heads of every encoder output: queue them behind the layers and synchronise ONCE --
            # the encoder's own time-out check is deferred to ss_encoder_stream_status (include/streamspeech_hip.h), so the device
            # runs from the last layer straight into the heads while the host is on its way back (~40 us of a ~1-ms call).
            L.check(self.lib.ss_encoder_stream_set_deferred(self.h, 1), "ss_encoder_stream_set_deferred")
            try:
                forward()
                ibuf = torch.empty((2 * (3 * Tp + 1),), dtype=torch.int32, device=self.device)
                for hd in (0, 1):
                    b = ibuf[hd * (3 * Tp + 1):(hd + 1) * (3 * Tp + 1)]
                    L.check(self.lib.ss_ctc_greedy(self.h, _stream(), hd, _ptr(out), Tp, _ptr(b[:Tp]), _ptr(b[Tp:2 * Tp]), _ptr(b[2 * Tp:3 * Tp]),
                                                   _ptr(b[3 * Tp:]), None), "ss_ctc_greedy")
                host = ibuf.cpu()
                rep = C.c_int32(0)
                L.check(self.lib.ss_encoder_stream_status(self.h, _stream(), C.byref(rep)), "ss_encoder_stream_status")
            finally:
                L.check(self.lib.ss_encoder_stream_set_deferred(self.h, 0), "ss_encoder_stream_set_deferred")
            if rep.value:            # a persistent launch timed out: the call again (one launch per op now), heads on request
                forward()
            else:
                self._ctc_both = ((out.data_ptr(), Tp), {0: host[:3 * Tp + 1], 1: host[3 * Tp + 1:]})
                self.stream_stats = (nf.value, nc.value)
                self._last_enc = (out.data_ptr(), Tp)
                return out
        else:
            forward()
        self._ctc_both = None
        self.stream_stats = (nf.value, nc.value)
        self._last_enc = (out.data_ptr(), Tp)
        return out

    def stream_pool(self, max_sessions: int, max_rows: int, scores: bool = False) -> "StreamPool":
        """A pool of `max_sessions` streaming-encoder slots of `max_rows` output rows each, booked in this handle's scratch set: one
        batched encoder step (and one CTC call per head) for many concurrent streams (:class:`StreamPool`).  `scores`: its CTC calls
        also answer each frame's log-probability and each token's span (ss_stream_pool_set_scores)."""
        return StreamPool(self, max_sessions, max_rows, scores)

    # ---- a8 -------------------------------------------------------------------------------
    # Both CTC heads behind ONE host round trip (off unless a caller sets ``ctc_speculate``; the agents do: policy() always asks for the
    # source head and then the target head of the same encoder output -- reference agent :437-452 -- and each answer used to cost a
    # synchronising device-to-host copy, ~35 us of an ~1-ms call).  The first request for a head of the tensor this engine produced last
    # also runs the OTHER head and parks its host-side answer; the second request takes it.  The parked answer dies with the next
    # encoder call and is handed out once, for the same (pointer, rows) only; a caller that rewrites the encoder output in place between
    # its two requests must leave the switch off.
    ctc_speculate = False

    def _ctc_unpack(self, host, Tp):
        n = int(host[3 * Tp])
        return host[Tp:Tp + n].tolist(), host[2 * Tp:2 * Tp + n].tolist(), host[:Tp], None

    def ctc_align(self, head: int, enc_out: torch.Tensor, tokens: List[int], want_path: bool = True) -> CtcAlignment:
        """Forced alignment of one utterance: the B = 1 call of batch_ctc_align."""
        return self.batch_ctc_align(head, enc_out.contiguous(), [int(enc_out.shape[0])], [list(tokens)], want_path)[0]

    def ctc_spot(self, head: int, enc_out: torch.Tensor, keywords, max_hits: int = 256):
        """Keyword spotting of one utterance: the B = 1 call of batch_ctc_spot."""
        return self.batch_ctc_spot(head, enc_out.contiguous(), [int(enc_out.shape[0])], keywords, max_hits)[0]

    def ctc_beam(self, head: int, enc_out: torch.Tensor, beam: int, cand: Optional[int] = None,
                 nbest: Optional[int] = None, lm=None, lm_weight: float = 0.0, word_score: float = 0.0,
                 lm_eos: bool = True, bias=None, bias_scale: float = 1.0, bias_finish: bool = True) -> List[CtcHypothesis]:
        """CTC prefix beam search of one utterance: the B = 1 call of batch_ctc_beam."""
        return self.batch_ctc_beam(head, enc_out.contiguous(), [int(enc_out.shape[0])], beam, cand, nbest, lm, lm_weight, word_score,
                                   lm_eos, bias, bias_scale, bias_finish)[0]

    def ctc_greedy(self, head: int, enc_out: torch.Tensor, want_logits: bool = False, want_scores: bool = False):
        """-> (tokens list, frame index list, raw argmax tensor, logits or None); with want_scores three more: last frame per token
        (list), summed log-probability per token and log-probability per frame (float32 arrays) -- agent/ctc_decoder.py:61."""
        Tp = enc_out.shape[0]
        key = (enc_out.data_ptr(), Tp)
        if want_scores:                    # its own call: the parked answers of the unscored form hold no scores
            V = self.cfg.src_vocab if head == 0 else self.cfg.tgt_vocab
            ibuf = torch.empty((6 * Tp + 1,), dtype=torch.int32, device=self.device)
            fbuf = ibuf.view(torch.float32)
            logits = torch.empty((Tp, V), dtype=torch.float32, device=self.device) if want_logits else None
            L.check(self.lib.ss_ctc_greedy_scored(self.h, _stream(), head, _ptr(enc_out), Tp, _ptr(ibuf[:Tp]), _ptr(ibuf[Tp:2 * Tp]),
                                                  _ptr(ibuf[2 * Tp:3 * Tp]), _ptr(ibuf[6 * Tp:]), _ptr(logits), _ptr(fbuf[4 * Tp:5 * Tp]),
                                                  _ptr(ibuf[3 * Tp:4 * Tp]), _ptr(fbuf[5 * Tp:6 * Tp])), "ss_ctc_greedy_scored")
            host = ibuf.cpu()
            toks, idx, last, tok_lp, lp = _unpack_scored(host.numpy(), [Tp])[0]
            return toks, idx, host[:Tp], logits, last, tok_lp, lp
        both = getattr(self, "_ctc_both", None)
        if both is not None and not want_logits and both[0] == key and head in both[1]:
            return self._ctc_unpack(both[1].pop(head), Tp)              # computed behind the streaming encoder call (handed out once)
        stash = getattr(self, "_ctc_stash", None)
        if stash is not None:
            self._ctc_stash = None
            if not want_logits and stash[0] == key and stash[1] == head:
                return self._ctc_unpack(stash[2], Tp)
        if self.ctc_speculate and not want_logits and key == getattr(self, "_last_enc", None):
            ibuf = torch.empty((2 * (3 * Tp + 1),), dtype=torch.int32, device=self.device)
            for k, hd in enumerate((head, 1 - head)):
                b = ibuf[k * (3 * Tp + 1):(k + 1) * (3 * Tp + 1)]
                L.check(self.lib.ss_ctc_greedy(self.h, _stream(), hd, _ptr(enc_out), Tp, _ptr(b[:Tp]), _ptr(b[Tp:2 * Tp]), _ptr(b[2 * Tp:3 * Tp]),
                                               _ptr(b[3 * Tp:]), None), "ss_ctc_greedy")
            host = ibuf.cpu()
            self._ctc_stash = (key, 1 - head, host[3 * Tp + 1:])
            return self._ctc_unpack(host[:3 * Tp + 1], Tp)
        V = self.cfg.src_vocab if head == 0 else self.cfg.tgt_vocab
        ibuf = torch.empty((3 * Tp + 1,), dtype=torch.int32, device=self.device)
        raw, toks, idx, cnt = ibuf[:Tp], ibuf[Tp:2 * Tp], ibuf[2 * Tp:3 * Tp], ibuf[3 * Tp:]
        logits = torch.empty((Tp, V), dtype=torch.float32, device=self.device) if want_logits else None
        L.check(self.lib.ss_ctc_greedy(self.h, _stream(), head, _ptr(enc_out), Tp, _ptr(raw), _ptr(toks), _ptr(idx),
                                       _ptr(cnt), _ptr(logits)), "ss_ctc_greedy")
        host = ibuf.cpu()
        n = int(host[3 * Tp])
        return host[Tp:Tp + n].tolist(), host[2 * Tp:2 * Tp + n].tolist(), host[:Tp], logits

    # ---- a9-a10 ---------------------------------------------------------------------------
    def mt_begin(self, enc_out: torch.Tensor):
        self._mt_enc = enc_out  # keep alive
        L.check(self.lib.ss_mt_begin(self.h, _stream(), _ptr(enc_out), enc_out.shape[0]), "ss_mt_begin")

    def mt_append(self, tokens: List[int], pos0: int, ban_eos: bool, force_eos: bool,
                  want_feats: bool = True, want_next: bool = True, n_tail_pad: int = 0) -> Tuple[Optional[torch.Tensor], Optional[int]]:
        n = len(tokens)
        if any(not 0 <= int(t) < self.cfg.tgt_vocab for t in tokens):      # nn.Embedding raises the same in the reference
            raise IndexError(f"token id outside the target dictionary of {self.cfg.tgt_vocab} entries: {tokens}")
        tok = torch.tensor(tokens, dtype=torch.int32).to(self.device)
        feats = torch.empty((n, self.cfg.dec_dim), dtype=torch.float32, device=self.device) if want_feats else None
        nxt = torch.empty((1,), dtype=torch.int32, device=self.device) if want_next else None
        L.check(self.lib.ss_mt_append(self.h, _stream(), _ptr(tok), n, pos0, int(ban_eos), int(force_eos),
                                      _ptr(feats), _ptr(nxt), n_tail_pad), "ss_mt_append")
        nx = int(nxt.item()) if want_next else None
        if nx is not None and nx < 0:
            # csrc/mt_step.hip: a bounded wait of the persistent decode step timed out (its workgroups were not all resident).
            # Loud, then the same call again with one launch per op -- it rewrites the same cache row and features.
            import warnings
            warnings.warn("persistent MT decode step timed out; this context falls back to one launch per op", RuntimeWarning)
            self.set_persistent_mt_step(0)
            return self.mt_append(tokens, pos0, ban_eos, force_eos, want_feats, want_next, n_tail_pad)
        return feats, nx

    def mt_greedy(self, enc_out: torch.Tensor, prefix: List[int], max_len: int, min_len: int = 1):
        """Beam-1 search in one C call -> (tokens after the prefix incl. final eos, feats [n_fed, D])."""
        self._mt_enc = enc_out
        n_pre = len(prefix)
        cap = max_len + 2
        feats = torch.empty((cap, self.cfg.dec_dim), dtype=torch.float32, device=self.device)
        c_pre = (C.c_int32 * max(n_pre, 1))(*prefix)
        c_out = (C.c_int32 * (max_len + 2 - n_pre))()
        n_out, n_feats = C.c_int(0), C.c_int(0)
        L.check(self.lib.ss_mt_greedy(self.h, _stream(), _ptr(enc_out), enc_out.shape[0], c_pre, n_pre, max_len,
                                      min_len, c_out, C.byref(n_out), _ptr(feats), C.byref(n_feats)), "ss_mt_greedy")
        if getattr(self, "persistent_mt", 0):                # a time-out inside makes the library fall back (and say so on stderr)
            self.persistent_mt = int(self.lib.ss_mt_get_persistent(self.h))
        return list(c_out[: n_out.value]), feats[: n_feats.value]

    def set_persistent_mt_step(self, workgroups: int = 64):
        """One persistent launch per MT decode step (0 restores the launch-per-op form); see ss_mt_set_persistent."""
        L.check(self.lib.ss_mt_set_persistent(self.h, int(workgroups)), "ss_mt_set_persistent")
        self.persistent_mt = int(workgroups)

    def set_pack_invariant(self, on: bool = True):
        """Pack-invariant arithmetic of the batch_* calls of this context (default on): see ss_model_set_pack_invariant."""
        L.check(self.lib.ss_model_set_pack_invariant(self.h, int(bool(on))), "ss_model_set_pack_invariant")

    def pack_invariant(self) -> bool:
        return bool(self.lib.ss_model_get_pack_invariant(self.h))

    def mt_truncate(self, length: int):
        L.check(self.lib.ss_mt_truncate(self.h, length), "ss_mt_truncate")

    # ---- a11-a13 --------------------------------------------------------------------------
    def t2u_units(self, mt_feats: torch.Tensor, t2u_causal: bool = False, mask_eos: bool = False,
                  want_logits: bool = False, n_tail_pad: int = 0, keep_raw: bool = False):
        """mt_feats [n,512] -> (collapsed unit-vocab tokens list, raw argmax tensor(host), logits or None); keep_raw: plus the raw
        arg-max ids on the DEVICE (what :meth:`batch_unit_spans` reads)."""
        n = mt_feats.shape[0]
        U = n * self.cfg.ctc_upsample
        ibuf = torch.empty((2 * U + 1,), dtype=torch.int32, device=self.device)
        raw, toks, cnt = ibuf[:U], ibuf[U:2 * U], ibuf[2 * U:]
        logits = torch.empty((U, self.cfg.unit_vocab), dtype=torch.float32, device=self.device) if want_logits else None
        L.check(self.lib.ss_t2u_units(self.h, _stream(), _ptr(mt_feats.contiguous()), n, int(t2u_causal),
                                      int(mask_eos), _ptr(raw), _ptr(toks), _ptr(cnt), _ptr(logits), n_tail_pad), "ss_t2u_units")
        host = ibuf.cpu()
        k = int(host[2 * U])
        if keep_raw:
            return host[U:U + k].tolist(), host[:U], logits, raw
        return host[U:U + k].tolist(), host[:U], logits


    def normalized_probs(self, logits: torch.Tensor, log_probs: bool = True, mask0: int = -1, mask1: int = -1) -> torch.Tensor:
        """model.get_normalized_probs on the device (ss_log_softmax): (log-)softmax over the last axis of dense logits, then ids
        mask0 / mask1 set to -inf (0).  Glue for callers that ask for `lprobs`; the greedy searches never need it."""
        x = logits.to(self.device, torch.float32).contiguous()
        V = x.shape[-1]
        rows = x.numel() // V
        out = torch.empty_like(x)
        L.check(self.lib.ss_log_softmax(_stream(), _ptr(x), rows, V, int(mask0), int(mask1), int(not log_probs), _ptr(out)), "ss_log_softmax")
        return out

    def unit_scores(self, mt_feats: torch.Tensor, t2u_causal: bool = False):
        """Per-position maximum log-probability (natural log, pad / unk / eos masked after the softmax) of the unit
        decoder over the 25 n positions -- the offline search's positional scores (researches/ctc_unity/ctc_generator.py:
        55-63).  -> float32 [U] on the host.  Offline driver with --scores only; not on the timed path."""
        _, _, logits = self.t2u_units(mt_feats, t2u_causal=t2u_causal, mask_eos=True, want_logits=True)
        U, V = logits.shape
        out = torch.empty((U,), dtype=torch.float32, device=self.device)
        c = self.cfg
        L.check(self.lib.ss_row_max_logprob(_stream(), _ptr(logits), U, V, c.pad, c.unk, c.eos, _ptr(out)), "ss_row_max_logprob")
        return out.cpu()


class ContinueRefused(ValueError):
    """A call ss_batch_mt_continue refuses; ``code`` is the SS_ERR_* it returns for it."""

    def __init__(self, msg, code):
        super().__init__(msg)
        self.code = code


class _PlanTables:
    """The int tables a planner returns, read front to back."""

    def __init__(self, words):
        self.t, self.o = list(words), 0

    def take(self, n):
        self.o += n
        return self.t[self.o - n:self.o]

    def quads(self, n):
        v = self.take(4 * n)
        return [tuple(v[4 * i:4 * i + 4]) for i in range(n)]

    def steps(self, n_steps, rows):
        v = self.quads(n_steps * rows)
        return [v[k * rows:(k + 1) * rows] for k in range(n_steps)]


def _run_planner(plan_fn, call: str, args: tuple, n_dims: int):
    """The two-call protocol of the host-only planners: once for the size of the tables -- a refusal raises ContinueRefused with the
    code `call` would return -- then again for the tables -> (dims, _PlanTables)."""
    lib = L.load()
    dims, n_tab = (C.c_int32 * n_dims)(), C.c_int64(0)
    rc = plan_fn(*args, dims, None, 0, C.byref(n_tab))
    if rc != 0:
        raise ContinueRefused(f"{call} refuses the call: {lib.ss_error_string(rc).decode()}", rc)
    tab = (C.c_int32 * n_tab.value)()
    L.check(plan_fn(*args, dims, tab, n_tab.value, C.byref(n_tab)), call + "_plan")
    return list(dims), _PlanTables(tab)


def _plan_args(Tp, n_prefix, max_len, feat_rows, out_stride, prefix_ids, least_stride):
    """What both planners do to their arguments: one length per row, feat_rows / out_stride at the least the call needs (the least
    out_stride of row (max_len, n_prefix) is the planner's own), placeholder ids for the prefixes."""
    B = len(Tp)
    if len(n_prefix) != B or len(max_len) != B:
        raise ContinueRefused("one prefix length and max_len per row", L.SS_ERR_ARG)
    if B and feat_rows is None:
        feat_rows = max(m + 1 for m in max_len)
    if B and out_stride is None:
        out_stride = max(least_stride(m, n) for m, n in zip(max_len, n_prefix))
    ids = list(prefix_ids) if prefix_ids is not None else [4] * sum(max(int(n), 0) for n in n_prefix)
    return B, feat_rows, out_stride, ids


def plan_mt_continue(Tp: List[int], n_prefix: List[int], max_len: List[int], min_len: int = 1, feat_rows: Optional[int] = None,
                     out_stride: Optional[int] = None, max_tgt_pos: int = 1026, prefix_ids: Optional[List[int]] = None,
                     vocab: int = 6000, eos: int = 2) -> dict:
    """Layout and refusals of one ss_batch_mt_continue call, as the library makes them (ss_batch_mt_continue_plan, host only -- the
    same planner the call runs): S = the longest prefix, Tn = the most lock-step steps a row may need, Lcap = S + 1 + Tn cache rows per
    row (row b shifted by shift[b] = S - n_prefix[b], so every row's first generated position sits at cache index S + 1), and the
    tables the call uploads.  feat_rows / out_stride default to the least the call needs.  Raises ContinueRefused with the code the
    call returns."""
    B, feat_rows, out_stride, ids = _plan_args(Tp, n_prefix, max_len, feat_rows, out_stride, prefix_ids, lambda m, n: m - n + 1)
    args = (B, _i32(Tp or [0]), _i32(ids or [0]), _i32(n_prefix or [0]), _i32(max_len or [0]), int(min_len), int(out_stride or 0),
            int(feat_rows or 0), int(max_tgt_pos), int(vocab), int(eos))
    (S, Tn, Lcap, Np), t = _run_planner(L.load().ss_batch_mt_continue_plan, "ss_batch_mt_continue", args, 4)
    p = {"S": S, "Tn": Tn, "Lcap": Lcap, "Np": Np, "feat_rows": feat_rows, "out_stride": out_stride}
    p["max_len_at"], p["min_len_at"] = t.take(B), t.take(B)
    p["shift"] = [-x for x in t.take(B)]
    p["step_cross"], p["prefix_self"], p["prefix_cross"] = t.quads(B), t.quads(B), t.quads(B)
    p["step_self"] = t.steps(max(Tn, 1), B)
    p["prefix_tokens"], p["prefix_pos"], p["cache_row"], p["feat_row"] = t.take(Np), t.take(Np), t.take(Np), t.take(Np)
    p["last_row"] = t.take(B)
    p["r0"] = [seg[0] for seg in p["prefix_self"]]
    assert t.o == len(t.t)
    return p


def plan_mt_beam_continue(Tp: List[int], n_prefix: List[int], max_len: List[int], beam: int, min_len: int = 1,
                          feat_rows: Optional[int] = None, out_stride: Optional[int] = None, max_tgt_pos: int = 1026,
                          prefix_ids: Optional[List[int]] = None, vocab: int = 6000, eos: int = 2, pad: int = 1,
                          len_penalty: float = 1.0, temperature: float = 1.0, no_repeat_ngram_size: int = 0) -> dict:
    """Layout and refusals of one ss_batch_mt_beam_continue call, as the library makes them (ss_batch_mt_beam_continue_plan, host only
    -- the same planner the call runs).  R = B * beam slots; row b's cache is shifted by S - n_prefix[b] (S = the longest prefix), so
    every slot writes cache index c0 + t at lock-step index t.  feat_rows / out_stride default to the least the call needs.  Raises
    ContinueRefused with the code the call returns.  With one of the three search controls off its default the planner is
    ss_batch_mt_beam_continue_plan_opts: the option refusals first (they reach the library as they are, so their code and their place
    in the order are the library's), the repeated-n-gram check of the prefixes last."""
    B, feat_rows, out_stride, ids = _plan_args(Tp, n_prefix, max_len, feat_rows, out_stride, prefix_ids, lambda m, n: m + 1)
    lib = L.load()
    plan_fn = lib.ss_batch_mt_beam_continue_plan
    if not (len_penalty == 1.0 and temperature == 1.0 and no_repeat_ngram_size == 0):
        opts = L.SSMtSearchOpts(C.sizeof(L.SSMtSearchOpts), int(no_repeat_ngram_size), float(len_penalty), float(temperature))
        plan_fn = lambda *a: lib.ss_batch_mt_beam_continue_plan_opts(*a, C.byref(opts))    # noqa: E731
    args = (B, int(beam), _i32(Tp or [0]), _i32(ids or [0]), _i32(n_prefix or [0]), _i32(max_len or [0]), int(min_len),
            int(out_stride or 0), int(feat_rows or 0), int(max_tgt_pos), int(vocab), int(eos), int(pad))
    (S, Tn, Lc, Np, R, c0, nseg, pm), t = _run_planner(plan_fn, "ss_batch_mt_beam_continue", args, 8)
    p = {"S": S, "Tn": Tn, "Lc": Lc, "Np": Np, "R": R, "c0": c0, "prefix_segments": nseg, "last_forced_in_prefix_pass": bool(pm),
         "feat_rows": feat_rows, "out_stride": out_stride}
    p["step_cross"] = t.quads(R)
    p["step_self"] = t.steps(Tn + 1, R)
    p["shift"] = [-x for x in t.take(R)]
    p["r0"] = t.take(B)
    p["prefix_self"], p["prefix_cross"] = t.quads(nseg), t.quads(nseg)
    p["prefix_tokens"], p["prefix_pos"], p["cache_row"], p["feat_row"], p["forced"] = (t.take(Np), t.take(Np), t.take(Np), t.take(Np),
                                                                                       t.take(Np))
    p["last_row"] = t.take(B)
    assert t.o == len(t.t)
    return p


def plan_pool_step(T: List[int], n_rows: List[int], max_rows: int) -> dict:
    """Host-side layout of one batched streaming step (what ss_encoder_stream_forward_batch packs), for checks and tests:
    per session the output rows T2, their packed offset (call order), the stacked offset of its tail rows among the sessions
    with rows to compute, and the 16-query tiles.  `n_rows[i]` = rows that session recomputes (T2 minus rows already final).
    Raises ValueError as the C ABI refuses a call (SS_ERR_ARG): a session past `max_rows` output rows or no input."""
    T2 = []
    for t in T:
        t = int(t)
        if t <= 0:
            raise ValueError("a session without fbank frames")
        t1 = (t + 2 * 2 - 5) // 2 + 1
        t2 = (t1 + 2 * 2 - 5) // 2 + 1
        if t2 <= 0 or t2 > max_rows:
            raise ValueError(f"session of {t2} output rows exceeds the pool's max_rows {max_rows}")
        T2.append(t2)
    off, q_start, qtiles, active = [], [], [], []
    o = q = 0
    for i, (t2, n) in enumerate(zip(T2, n_rows)):
        if not 0 <= n <= t2:
            raise ValueError("rows to compute outside [0, T2]")
        off.append(o)
        q_start.append(q)
        qtiles.append((n + 15) // 16)
        if n > 0:
            active.append(i)
        o += t2
        q += n
    return {"T2": T2, "off": off, "total": o, "q_start": q_start, "M": q, "qtiles": qtiles, "active": active}


class StreamPool:
    """Incremental-encoder state of up to `max_sessions` concurrent streams (ss_stream_pool): slot i holds one utterance's
    per-layer caches, its final output rows and the cached CTC arg-max of those rows.  :meth:`forward` runs ONE encoder step for
    any subset of slots; per slot it behaves exactly like :meth:`HipModel.encoder_stream_forward` on a context of its own.
    Driven by one host thread at a time (like a scratch set)."""

    def __init__(self, model: "HipModel", max_sessions: int, max_rows: int, scores: bool = False):
        self.lib, self.model, self.device = model.lib, model, _require_gpu(model.device)
        self.max_sessions, self.max_rows = int(max_sessions), int(max_rows)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_stream_pool_create(model.h, self.max_sessions, self.max_rows, C.byref(h)), "ss_stream_pool_create")
        self.h = h
        self.scores = False
        if scores:
            self.set_scores(True)
        self._last = None          # (slots, T2 list, packed output tensor) of the last forward: what ctc() reads

    def reset(self, slot: int):
        L.check(self.lib.ss_stream_pool_reset(self.h, int(slot)), "ss_stream_pool_reset")

    def set_scores(self, on: bool):
        """Switch the scored form of :meth:`ctc` / :meth:`ctc_both` on or off; only while no slot holds rows."""
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_stream_pool_set_scores(self.h, 1 if on else 0), "ss_stream_pool_set_scores")
        self.scores = bool(on)

    def _ctc_scored(self, head: int, n: int, lslots, enc, ibuf, tot: int):
        """Queue one head's scored call into ibuf (int32 [6 tot + n], the layout of _unpack_scored)."""
        fbuf = ibuf.view(torch.float32)
        L.check(self.lib.ss_stream_pool_ctc_scored(self.model.h, _stream(), self.h, int(head), n, _i32(lslots), _ptr(enc), _ptr(ibuf[:tot]),
                                                   _ptr(ibuf[tot:2 * tot]), _ptr(ibuf[2 * tot:3 * tot]), _ptr(ibuf[6 * tot:]),
                                                   _ptr(fbuf[4 * tot:5 * tot]), _ptr(ibuf[3 * tot:4 * tot]), _ptr(fbuf[5 * tot:6 * tot])),
                "ss_stream_pool_ctc_scored")

    def set_tail(self, slot: int, unsettled_fbank_frames: int):
        L.check(self.lib.ss_stream_pool_set_tail(self.h, int(slot), int(unsettled_fbank_frames)), "ss_stream_pool_set_tail")

    def check_step(self, slots: List[int], fbanks: List[torch.Tensor], attn_chunks: Optional[List[int]] = None,
                   conv_chunks: Optional[List[int]] = None):
        """The argument checks of a step, on the host (ValueError), before any device call."""
        if not slots or len(slots) != len(fbanks):
            raise ValueError("one fbank per slot, at least one slot")
        for name, ch in (("attn_chunks", attn_chunks), ("conv_chunks", conv_chunks)):
            if ch is not None and len(ch) != len(slots):
                raise ValueError(f"{name}: one entry per slot")
        if len(set(int(s) for s in slots)) != len(slots):
            raise ValueError("duplicate slot in one step")
        for s in slots:
            if not 0 <= int(s) < self.max_sessions:
                raise ValueError(f"slot {s} outside [0, {self.max_sessions})")
        return plan_pool_step([f.shape[0] for f in fbanks], [0] * len(fbanks), self.max_rows)

    def forward(self, slots: List[int], fbanks: List[torch.Tensor], attn_chunks: List[int], conv_chunks: List[int]):
        """One encoder step of the sessions in `slots` (fbank of ALL their audio so far each).  -> (packed output [sum T2, 256] in
        call order, per-session views into it, n_final list, n_computed list)."""
        plan = self.check_step(slots, fbanks, attn_chunks, conv_chunks)
        n = len(slots)
        for f in fbanks:
            if not (f.device == self.device or (f.is_cuda and f.device.index == (self.device.index or 0))):
                raise ValueError(f"fbank on {f.device}, the pool lives on {self.device}")
            if f.dtype != torch.float32 or not f.is_contiguous() or f.dim() != 2 or f.shape[1] != self.model.cfg.input_feat:
                raise ValueError("fbank must be a contiguous float32 [T, 80] tensor")
        out = torch.empty((plan["total"], self.model.cfg.enc_dim), dtype=torch.float32, device=self.device)
        nf, nc = (C.c_int32 * n)(), (C.c_int32 * n)()
        ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in fbanks])
        L.check(self.lib.ss_encoder_stream_forward_batch(
            self.model.h, _stream(), self.h, n, _i32(slots), ptrs, _i32([f.shape[0] for f in fbanks]),
            _i32([min(int(a), 1 << 30) for a in attn_chunks]), _i32([min(int(c), 1 << 30) for c in conv_chunks]),
            _ptr(out), nf, nc), "ss_encoder_stream_forward_batch")
        views = [out[o:o + t2] for o, t2 in zip(plan["off"], plan["T2"])]
        self._last = (list(int(s) for s in slots), plan["T2"], out)     # the tensor itself, not its pointer
        return out, views, list(nf), list(nc)

    def ctc(self, head: int, slots: Optional[List[int]] = None, enc_packed: Optional[torch.Tensor] = None, return_raw: bool = False):
        """Greedy CTC of head `head` over the last step's output -> per-session (tokens, frame index) as ctc_greedy gives them
        (+ the raw per-frame arg-max with return_raw).  Only rows the slots have not seen final yet go through the head."""
        if self._last is None:
            raise ValueError("ctc() before any forward()")
        lslots, T2, lout = self._last
        if slots is not None and [int(s) for s in slots] != lslots:
            raise ValueError("ctc() takes the slots of the last forward(), in its order")
        enc = lout if enc_packed is None else enc_packed
        if enc.shape[0] != sum(T2):
            raise ValueError("packed output of another step")
        n, tot = len(lslots), sum(T2)
        if self.scores:                # -> per session (tokens, index, last, tok_lprob, lprob rows) (+ raw)
            ibuf = torch.empty((6 * tot + n,), dtype=torch.int32, device=self.device)
            self._ctc_scored(head, n, lslots, enc, ibuf, tot)
            return _unpack_scored(ibuf.cpu().numpy(), T2, return_raw)
        ibuf = torch.empty((3 * tot + n,), dtype=torch.int32, device=self.device)
        raw, toks, idx, cnt = ibuf[:tot], ibuf[tot:2 * tot], ibuf[2 * tot:3 * tot], ibuf[3 * tot:]
        L.check(self.lib.ss_stream_pool_ctc(self.model.h, _stream(), self.h, int(head), n, _i32(lslots), _ptr(enc), _ptr(raw),
                                            _ptr(toks), _ptr(idx), _ptr(cnt)), "ss_stream_pool_ctc")
        host = ibuf.cpu().numpy()
        res, off = [], 0
        for b in range(n):
            k = int(host[3 * tot + b])
            rec = (host[tot + off: tot + off + k].tolist(), host[2 * tot + off: 2 * tot + off + k].tolist())
            res.append(rec + (host[off: off + T2[b]].tolist(),) if return_raw else rec)
            off += T2[b]
        return res

    def ctc_both(self):
        """Both heads of the last step behind ONE device-to-host copy -> (head-0 results, head-1 results), each as :meth:`ctc`."""
        if self._last is None:
            raise ValueError("ctc_both() before any forward()")
        lslots, T2, enc = self._last
        n, tot = len(lslots), sum(T2)
        if self.scores:                # the float bits ride in the same int32 buffer: still ONE copy
            per = 6 * tot + n
            ibuf = torch.empty((2 * per,), dtype=torch.int32, device=self.device)
            for hd in (0, 1):
                self._ctc_scored(hd, n, lslots, enc, ibuf[hd * per:(hd + 1) * per], tot)
            host = ibuf.cpu().numpy()
            return _unpack_scored(host[:per], T2), _unpack_scored(host[per:], T2)
        per = 3 * tot + n
        ibuf = torch.empty((2 * per,), dtype=torch.int32, device=self.device)
        for hd in (0, 1):
            b = ibuf[hd * per:(hd + 1) * per]
            L.check(self.lib.ss_stream_pool_ctc(self.model.h, _stream(), self.h, hd, n, _i32(lslots), _ptr(enc), _ptr(b[:tot]),
                                                _ptr(b[tot:2 * tot]), _ptr(b[2 * tot:3 * tot]), _ptr(b[3 * tot:])), "ss_stream_pool_ctc")
        host = ibuf.cpu().numpy()
        res = []
        for hd in (0, 1):
            h = host[hd * per:(hd + 1) * per]
            out, off = [], 0
            for b in range(n):
                k = int(h[3 * tot + b])
                out.append((h[tot + off: tot + off + k].tolist(), h[2 * tot + off: 2 * tot + off + k].tolist()))
                off += T2[b]
            res.append(out)
        return res[0], res[1]

    def stats(self) -> Tuple[int, int]:
        """Test hook: (kernels the pool's calls launched -- its own plus the GEMM-family launches the library's census saw during them --,
        rows its CTC calls ran through a head) since creation."""
        a, b = C.c_int64(0), C.c_int64(0)
        L.check(self.lib.ss_stream_pool_stats(self.h, C.byref(a), C.byref(b)), "ss_stream_pool_stats")
        return int(a.value), int(b.value)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ss_stream_pool_destroy(self.h)
                self.h = None
        except Exception:
            pass


class CtcPartial(NamedTuple):
    """What one CtcStream.advance reports for a session."""
    hyps: List[CtcHypothesis]   # the search's n-best after `frames` frames, best first (none after a NaN row)
    n_stable: int               # the first n_stable tokens are common to every string of the beam: they can never change again
    frames: int                 # frames the search has consumed
    final: bool                 # the utterance's last call (the slot was reset by it)


class CtcStream:
    """The resumable CTC prefix beam search of a text head (ss_ctc_stream): `max_sessions` slots, each the search of one utterance
    kept on the device between calls.  :meth:`advance` moves any subset of slots forward over encoder rows that are FINAL (the
    incremental encoder's n_final); the utterance's last call gives exactly batch_ctc_beam's n-best on all its frames, every other
    call the n-best of the frames so far and how many leading tokens can no longer change.  beam, cand (default
    ctc_beam_default_cand), nbest (default beam), the model lm (an ngram.NgramLM; kept alive here) and its weights, and the hotword
    set bias (a hotwords.CtcBias; kept alive here: ss_ctc_stream_create_bias, hypotheses CtcBiasHypothesis, the finish term in an
    utterance's last call alone) and its scale are fixed at creation; the trie is sized for `max_frames` encoder rows per utterance (at most L.CTC_BEAM_MAX_FRAMES).  The state is booked
    on the model's scratch set and released by :meth:`close`."""

    def __init__(self, model: "HipModel", head: int, max_sessions: int, max_frames: int, beam: int, cand: Optional[int] = None,
                 nbest: Optional[int] = None, lm=None, lm_weight: float = 0.0, word_score: float = 0.0, lm_eos: bool = True,
                 bias=None, bias_scale: float = 1.0, bias_finish: bool = True):
        self.lib, self.model, self.device = model.lib, model, _require_gpu(model.device)
        self.head, self.max_sessions, self.max_frames, self.beam = int(head), int(max_sessions), int(max_frames), int(beam)
        self.cand = ctc_beam_default_cand(beam) if cand is None else int(cand)
        self.nbest = self.beam if nbest is None else int(nbest)
        self.lm, self.bias = lm, bias
        opts = C.byref(L.SSCtcLmOpts(float(lm_weight), float(word_score), int(bool(lm_eos)))) if lm is not None else None
        self.h = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            if bias is not None:
                bopts = L.SSCtcBiasOpts(float(bias_scale), int(bool(bias_finish)), 0)
                L.check(self.lib.ss_ctc_stream_create_bias(model.h, self.head, self.max_sessions, self.max_frames, self.beam, self.cand,
                                                           self.nbest, lm.h if lm is not None else None, opts, bias.h, C.byref(bopts),
                                                           C.byref(h)), "ss_ctc_stream_create_bias")
            else:
                L.check(self.lib.ss_ctc_stream_create(model.h, self.head, self.max_sessions, self.max_frames, self.beam, self.cand,
                                                      self.nbest, lm.h if lm is not None else None, opts, C.byref(h)), "ss_ctc_stream_create")
        self.h = h

    def reset(self, slot: int):
        """A new utterance in `slot` (host-only; the utterance's last advance does it by itself)."""
        L.check(self.lib.ss_ctc_stream_reset(self.h, int(slot)), "ss_ctc_stream_reset")

    def advance(self, slots: List[int], enc_packed: torch.Tensor, T: List[int], upto: List[int], final: List[bool]) -> List[CtcPartial]:
        """Session i owns T[i] packed rows of enc_packed (all its encoder output so far); the search of slots[i] moves to upto[i]
        frames; final[i]: the utterance's last call.  One buffer, one device-to-host copy."""
        n = len(slots)
        stride = max([int(u) for u in upto] + [1])
        k = n * self.nbest
        w = 10 if self.bias is not None else 8 if self.lm is not None else 4   # int32 words per hypothesis record
        # int32 words: hyps [w k] (first: 8-byte aligned) | parts [4 n] | tokens [k][stride]
        ibuf = torch.empty((w * k + 4 * n + k * stride + 1,), dtype=torch.int32, device=self.device)
        L.check(self.lib.ss_ctc_stream_advance(self.model.h, _stream(), self.h, n, _i32(slots), _ptr(enc_packed), _i32(T), _i32(upto),
                                               _i32([1 if f else 0 for f in final]), _ptr(ibuf), _ptr(ibuf[w * k + 4 * n:]), stride,
                                               _ptr(ibuf[w * k:])), "ss_ctc_stream_advance")
        host = ibuf.cpu().numpy()
        part = host[w * k: w * k + 4 * n].reshape(n, 4)
        tok = host[w * k + 4 * n:]
        if self.bias is not None:
            hyp = host[:w * k].view(_BIAS_HYP)
            mk = lambda j: CtcBiasHypothesis(tok[j * stride: j * stride + int(hyp["n_tokens"][j])].tolist(), float(hyp["score"][j]),  # noqa: E731
                                             float(hyp["ctc_score"][j]), float(hyp["lm_score"][j]) if self.lm is not None else None,
                                             float(hyp["bias_score"][j]))
        elif self.lm is not None:
            hyp = host[:w * k].view(np.dtype([("score", "<f8"), ("ctc_score", "<f8"), ("lm_score", "<f8"), ("n_tokens", "<i4"),
                                              ("status", "<i4")]))
            mk = lambda j: CtcHypothesis(tok[j * stride: j * stride + int(hyp["n_tokens"][j])].tolist(), float(hyp["score"][j]),  # noqa: E731
                                         float(hyp["ctc_score"][j]), float(hyp["lm_score"][j]))
        else:
            hyp = host[:w * k].view(np.dtype([("score", "<f8"), ("n_tokens", "<i4"), ("status", "<i4")]))
            mk = lambda j: CtcHypothesis(tok[j * stride: j * stride + int(hyp["n_tokens"][j])].tolist(), float(hyp["score"][j]))  # noqa: E731
        return [CtcPartial([mk(j) for j in range(i * self.nbest, (i + 1) * self.nbest) if hyp["status"][j] == 0], int(part[i, 1]),
                           int(part[i, 0]), bool(final[i])) for i in range(n)]

    def close(self):
        if getattr(self, "h", None):
            self.lib.ss_ctc_stream_destroy(self.h)
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


class CtcSpots(NamedTuple):
    """What one CtcSpotStream.advance reports for a session."""
    hits: list                  # keywords.CtcHit tuples emitted in this call, sorted by (end, keyword, start); rows of the utterance
    n_hits: int                 # the true number (above len(hits): max_hits was too small)
    frames: int                 # frames the spotter has consumed
    status: int                 # 0, or 2 once a NaN row was seen (sticky until the slot is reset)
    final: bool                 # the utterance's last call (the slot was reset by it)


class CtcSpotStream:
    """The resumable keyword spotter of a text head (ss_ctc_spot_stream): `max_sessions` slots, each the recursion of one utterance
    kept on the device between calls.  :meth:`advance` moves any subset of slots forward over encoder rows that are FINAL (the
    incremental encoder's n_final) and returns the hits that were emitted on the way; the hits of all calls of an utterance are
    exactly batch_ctc_spot's on all its frames.  The set (a keywords.CtcKeywords; kept alive here) is fixed at creation.  The state
    is booked on the model's scratch set and released by :meth:`close`."""

    def __init__(self, model: "HipModel", head: int, max_sessions: int, keywords):
        self.lib, self.model, self.device = model.lib, model, _require_gpu(model.device)
        self.head, self.max_sessions, self.keywords = int(head), int(max_sessions), keywords
        self.h = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_ctc_spot_stream_create(model.h, self.head, self.max_sessions, keywords.h, C.byref(h)),
                    "ss_ctc_spot_stream_create")
        self.h = h

    def reset(self, slot: int):
        """A new utterance in `slot` (host-only; the utterance's last advance does it by itself)."""
        L.check(self.lib.ss_ctc_spot_stream_reset(self.h, int(slot)), "ss_ctc_spot_stream_reset")

    def advance(self, slots: List[int], enc_packed: torch.Tensor, T: List[int], upto: List[int], final: List[bool],
                max_hits: int = 64) -> List[CtcSpots]:
        """Session i owns T[i] packed rows of enc_packed (all its encoder output so far); the spotter of slots[i] moves to upto[i]
        frames; final[i]: the utterance's last call.  One buffer, one device-to-host copy."""
        from .keywords import COUNT_DTYPE, HIT_DTYPE, hits_from_records
        n, mh = len(slots), int(max_hits)
        # int32 words: hits [6 n mh] (first: 8-byte aligned) | counts [4 n]
        ibuf = torch.empty((6 * n * max(mh, 0) + 4 * n + 2,), dtype=torch.int32, device=self.device)
        L.check(self.lib.ss_ctc_spot_stream_advance(self.model.h, _stream(), self.h, n, _i32(slots), _ptr(enc_packed), _i32(T), _i32(upto),
                                                    _i32([1 if f else 0 for f in final]), mh, _ptr(ibuf), _ptr(ibuf[6 * n * max(mh, 0):])),
                "ss_ctc_spot_stream_advance")
        host = ibuf.cpu().numpy()
        rec = host[:6 * n * mh].view(HIT_DTYPE).reshape(n, mh)
        cnt = host[6 * n * mh: 6 * n * mh + 4 * n].view(COUNT_DTYPE)
        return [CtcSpots(hits_from_records(rec[i, :min(int(cnt["n_hits"][i]), mh)]), int(cnt["n_hits"][i]), int(cnt["frames"][i]),
                         int(cnt["status"][i]), bool(final[i])) for i in range(n)]

    def close(self):
        if getattr(self, "h", None):
            self.lib.ss_ctc_spot_stream_destroy(self.h)
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


class HipVocoder:
    """ss_vocoder handle (CodeHiFiGANVocoderWithDur replacement)."""

    def __init__(self, generator_state_dict, cfg: VocoderConfig = None, device="cuda:0", _share=None, scratch: "Scratch" = None):
        self.lib = L.load()
        self.cfg = cfg or VocoderConfig()
        self.device = _require_gpu(device)
        if _share is not None:
            names, offsets, numels, self.blob = _share
        else:
            names, offsets, numels, blob = pack_vocoder(generator_state_dict, self.cfg)
            self.blob = blob.to(self.device)
        self._packed = (names, offsets, numels, self.blob)
        c = self.cfg
        cc = L.SSVocoderConfig()
        c.validate()
        # model_in_dim handed to the library is the CODE half's width: a multi-speaker conv_pre contracts the code embeddings only,
        # its speaker half is the "voc.spkr.table" slot of the blob (header: ss_vocoder_forward_spkr)
        cc.num_embeddings, cc.embedding_dim, cc.model_in_dim = c.num_embeddings, c.embedding_dim, c.embedding_dim
        cc.upsample_initial_channel = c.upsample_initial_channel
        cc.n_up = len(c.upsample_rates)
        for i, (u, k) in enumerate(zip(c.upsample_rates, c.upsample_kernel_sizes)):
            cc.upsample_rates[i] = u
            cc.upsample_kernel_sizes[i] = k
        cc.n_res = len(c.resblock_kernel_sizes)
        for j, (k, dil) in enumerate(zip(c.resblock_kernel_sizes, c.resblock_dilation_sizes)):
            cc.resblock_kernel_sizes[j] = k
            for t, dv in enumerate(dil):
                cc.resblock_dilations[j][t] = dv
        cc.dur_hidden, cc.dur_kernel = c.dur_hidden, c.dur_kernel
        self.c_cfg = cc
        cn, co, cm, n = _slots(names, offsets, numels)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_vocoder_create(C.byref(cc), _ptr(self.blob), self.blob.numel(), cn, co, cm, n,
                                               C.byref(h)), "ss_vocoder_create")
        self.h = h
        self.num_speakers = int(self.lib.ss_vocoder_num_speakers(self.h))       # 0: single-speaker
        self.scratch = None
        if scratch is not None:
            self.bind_scratch(scratch)
        self.hop = int(np.prod(c.upsample_rates))
        self.max_dur = 64

    def bind_scratch(self, scratch: "Scratch"):
        L.check(self.lib.ss_vocoder_bind_scratch(self.h, scratch.h), "ss_vocoder_bind_scratch")
        self.scratch = scratch

    def new_context(self, scratch: "Scratch" = None) -> "HipVocoder":
        v = HipVocoder(None, self.cfg, device=str(self.device), _share=self._packed, scratch=scratch)
        if getattr(self, "bf16x3", False):
            v.set_bf16x3(True)
        if getattr(self, "fp16", False):
            v.set_fp16(True)
        return v

    def set_fp16(self, on: bool):
        """Opt-in FP16 matrix-core ResBlock convs of the 64-, 128- and 256-channel stages of this handle (f32 accumulation; the
        duration predictor and every other conv stay f32, so durations are unchanged; waveform within 1e-3 RMS of the f32 path).
        Wins over bf16x3 while both are on; off (the default) is the exact f32 path."""
        with torch.cuda.device(self.device):
            L.check(self.lib.ss_vocoder_set_f16(self.h, int(bool(on))), "ss_vocoder_set_f16")
        self.fp16 = bool(on)

    def set_bf16x3(self, on: bool):
        """Opt-in split-bf16 (3 bf16 MFMAs per k-slice) contraction for the C >= 64 generator convs of this handle; the
        default (off) is exact f32, the reference's arithmetic."""
        L.check(self.lib.ss_vocoder_set_bf16x3(self.h, int(bool(on))), "ss_vocoder_set_bf16x3")
        self.bf16x3 = bool(on)

    def _check_units(self, ids: torch.Tensor):
        """nn.Embedding(num_embeddings, ...) of the reference's CodeGenerator raises IndexError on such ids (codehifigan.py:56-70)."""
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.cfg.num_embeddings):
            raise IndexError(f"unit id outside the vocoder's {self.cfg.num_embeddings} codes")

    def _check_speakers(self, speakers, n: int) -> Optional[List[int]]:
        """The voices of an n-row call: None on a single-speaker handle (which takes none), n ids inside [0, num_speakers) on a
        multi-speaker one.  nn.Embedding(num_speakers, ...) of the reference raises IndexError on an id outside."""
        if not self.num_speakers:
            if speakers is not None:
                raise ValueError("this vocoder is single-speaker: it takes no speaker")
            return None
        if speakers is None:
            raise ValueError('require a speaker for a multi-speaker vocoder (the reference: require "spkr" input)')
        ids = [int(x) for x in speakers]
        if len(ids) != n:
            raise ValueError(f"{len(ids)} speakers for {n} rows")
        if any(x < 0 or x >= self.num_speakers for x in ids):
            raise IndexError(f"speaker id outside the vocoder's {self.num_speakers} speakers")
        return ids

    def batch_forward(self, codes: List[List[int]], dur_prediction=True, forced_dur: Optional[List[List[int]]] = None,
                      speakers: Optional[List[int]] = None):
        """-> (list of wav tensors (views into one packed buffer), list of dur lists).  speakers: one id per row on a
        multi-speaker vocoder -- any mix of voices in the one pack."""
        B = len(codes)
        spk = self._check_speakers(speakers, B)
        K = [len(c) for c in codes]
        flat = torch.tensor([u for c in codes for u in c], dtype=torch.int32)
        self._check_units(flat)
        flat = flat.to(self.device)
        fd = None
        if forced_dur is not None:
            fd = torch.tensor([d for ds in forced_dur for d in ds], dtype=torch.int32).to(self.device)
            cap = int(sum(sum(ds) for ds in forced_dur)) * self.hop
        else:
            cap = sum(K) * (self.max_dur if dur_prediction else 1) * self.hop
        wav = torch.empty((cap,), dtype=torch.float32, device=self.device)
        dur = torch.empty((sum(K),), dtype=torch.int32, device=self.device)
        st, ns = (C.c_int64 * B)(), (C.c_int64 * B)()
        if spk is None:
            L.check(self.lib.ss_batch_vocoder_forward(self.h, _stream(), B, _ptr(flat), _i32(K), int(dur_prediction), _ptr(fd),
                                                      _ptr(wav), cap, _ptr(dur), st, ns), "ss_batch_vocoder_forward")
        else:
            L.check(self.lib.ss_batch_vocoder_forward_spkr(self.h, _stream(), B, _ptr(flat), _i32(K), int(dur_prediction), _ptr(fd),
                                                           _ptr(wav), cap, _ptr(dur), st, ns, _i32(spk)),
                    "ss_batch_vocoder_forward_spkr")
        wavs = [wav[st[b]: st[b] + ns[b]] for b in range(B)]
        return wavs, dur, K

    def batch_tail(self, codes: List[List[int]], n_new: List[int], ctx: List[int], rf: List[int], dur_prediction: bool = True,
                   speakers: Optional[List[int]] = None):
        """B rows of the agent's receptive-field tail (agent.synthesize_tail) in one call (ss_batch_vocoder_tail).  -> (per row the
        samples of its n_new[b] new units (views into one packed buffer), per row (first unit synthesised, durations of the
        synthesised units)).  A windowed row whose context does not cover the receptive field falls back to all its units.
        speakers: one id per row on a multi-speaker vocoder; rows of different voices share the one call."""
        B = len(codes)
        if not (len(n_new) == len(ctx) == len(rf) == B) or B == 0:
            raise ValueError("one unit list, n_new, ctx and rf per row")
        spk = self._check_speakers(speakers, B)
        K = [len(c) for c in codes]
        flat = torch.tensor([u for c in codes for u in c], dtype=torch.int32)
        self._check_units(flat)
        flat = flat.to(self.device)
        cap = sum(int(n) for n in n_new) * (self.max_dur if dur_prediction else 1) * self.hop
        out = torch.empty((max(cap, 1),), dtype=torch.float32, device=self.device)
        first = (C.c_int32 * B)()
        dur = (C.c_int32 * max(sum(K), 1))()
        st, ns = (C.c_int64 * B)(), (C.c_int64 * B)()
        rfs = _i32([-1 if r is None else r for r in rf])
        if spk is None:
            L.check(self.lib.ss_batch_vocoder_tail(self.h, _stream(), B, _ptr(flat), _i32(K), _i32(n_new), _i32(ctx), rfs,
                                                   int(dur_prediction), _ptr(out), cap, first, dur, st, ns), "ss_batch_vocoder_tail")
        else:
            L.check(self.lib.ss_batch_vocoder_tail_spkr(self.h, _stream(), B, _ptr(flat), _i32(K), _i32(n_new), _i32(ctx), rfs,
                                                        int(dur_prediction), _ptr(out), cap, first, dur, st, ns, _i32(spk)),
                    "ss_batch_vocoder_tail_spkr")
        tails = [out[st[b]: st[b] + ns[b]] for b in range(B)]
        info, off = [], 0
        for b in range(B):
            info.append((int(first[b]), list(dur[off: off + K[b] - first[b]])))
            off += K[b]
        return tails, info

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.ss_vocoder_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def forward(self, codes, dur_prediction: bool = True, forced_dur=None, speaker: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """codes: list/array/tensor of unit ids -> (wav [S] float32 device, dur [K] int32 device).  speaker: the voice, on a
        multi-speaker vocoder (required there)."""
        spk = self._check_speakers(None if speaker is None else [speaker], 1)
        codes_t = torch.as_tensor(codes, dtype=torch.int32).reshape(-1)
        if not codes_t.is_cuda:
            self._check_units(codes_t)                      # device-resident ids are guarded by the gather kernel instead
        codes_t = codes_t.to(self.device)
        K = codes_t.numel()
        fd = None if forced_dur is None else torch.as_tensor(forced_dur, dtype=torch.int32).reshape(-1).to(self.device)
        cap = K * self.max_dur * self.hop
        wav = torch.empty((cap,), dtype=torch.float32, device=self.device)
        dur = torch.empty((K,), dtype=torch.int32, device=self.device)
        ns = C.c_int64(0)
        if spk is None:
            rc = self.lib.ss_vocoder_forward(self.h, _stream(), _ptr(codes_t), K, int(dur_prediction), _ptr(fd),
                                             _ptr(wav), cap, _ptr(dur), C.byref(ns))
            L.check(rc, "ss_vocoder_forward")
        else:
            rc = self.lib.ss_vocoder_forward_spkr(self.h, _stream(), _ptr(codes_t), K, int(dur_prediction), _ptr(fd),
                                                  _ptr(wav), cap, _ptr(dur), C.byref(ns), spk[0])
            L.check(rc, "ss_vocoder_forward_spkr")
        return wav[: ns.value], dur
