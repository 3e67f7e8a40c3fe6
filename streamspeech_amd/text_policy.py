"""The host-side decisions of the streaming text agents, in one place: the read/write gate of the simultaneous S2TT agent (reference
agent/speech_to_text.s2tt.streamspeech.agent.py:480-512) and the length rule of the first-pass text search (agent/sequence_generator.py:
229-245, 340).  StreamSpeechS2TTAgent, SequenceGenerator and the concurrent text session pool (text_pool.py) all call these, so a
session decides the same way whichever of them serves it."""
import math
from typing import NamedTuple, Optional

CTC_BEAM_MAX = 32              # SS_CTC_BEAM_MAX_BEAM and SS_CTC_BEAM_MAX_CAND of the header (lib.CTC_BEAM_MAX_BEAM / _CAND)


class Gate(NamedTuple):
    write: bool                # run the text search this call
    src_prefix_len: int        # the agent's src_ctc_prefix_length after the call
    tgt_prefix_len: int        # ... and tgt_ctc_prefix_length
    new_tokens: int            # max_new_tokens of the search (-1: the source is finished, search to the end)


def s2tt_gate(n_src_ctc: int, n_tgt_ctc: int, src_prefix_len: int, tgt_prefix_len: int, n_committed: int, lagging_k1: int,
              stride_n: int, source_finished: bool) -> Gate:
    """Read/write gate on the CTC token counts of the two heads.  n_committed = target subwords committed so far (0 before the
    first write).  A read keeps the prefix lengths as they were unless both heads grew by stride_n (then they advance, as the agent
    stores them before it checks the lagging rule)."""
    if source_finished:
        return Gate(True, src_prefix_len, tgt_prefix_len, -1)
    if n_src_ctc < src_prefix_len + stride_n or n_tgt_ctc < tgt_prefix_len + stride_n:
        return Gate(False, src_prefix_len, tgt_prefix_len, 0)
    src_prefix_len = max(n_src_ctc, src_prefix_len)
    tgt_prefix_len = max(n_tgt_ctc, tgt_prefix_len)
    subword_tokens = ((n_tgt_ctc - lagging_k1) // stride_n) * stride_n
    new_tokens = subword_tokens - n_committed
    return Gate(new_tokens >= 1, src_prefix_len, tgt_prefix_len, new_tokens)


def mt_max_len(start: int, src_len: int, max_new_tokens: int, max_len_a: float, max_len_b: int, max_len: int,
               min_len: int) -> int:
    """Forced-</s> position of a greedy continuation of a `start`-token prefix: prefix + max_new_tokens, or with max_new_tokens = -1
    min(max_len_a * src_len + max_len_b, max_len - 1) (src_len = fbank frames).  Raises as the reference does when no hypothesis
    can be finalized (AssertionError for min_len > max_len, IndexError for a prefix past max_len)."""
    if max_new_tokens == -1:
        out = min(int(max_len_a * src_len + max_len_b), max_len - 1)
    else:
        out = start + max_new_tokens
    assert min_len <= out, "min_len cannot be larger than max_len, please adjust these!"
    if start > out:
        # the reference's step loop `for step in range(start, max_len + 1)` (agent/sequence_generator.py:340) is empty
        # then, nothing is finalized and the agent's finalized_mt[0][0] raises IndexError: same error here
        raise IndexError(f"prefix of {start} tokens is longer than max_len = {out}: no hypothesis can be finalized")
    return out


def asr_beam_emit(prev_text: str, symbols_of_best, n_stable: int, finished: bool):
    """What a streaming ASR session on the resumable CTC prefix beam search (engine.CtcStream) writes after a step: the committed
    text is the " ".join of the first n_stable symbols of the best hypothesis -- the tokens every string of the beam shares, which
    no later frame can change -- or of all of them when the utterance is finished.  -> (new_text, text): new_text is what the
    committed text adds to prev_text (the text committed before).  Raises if it would not extend prev_text: the stable prefix only
    grows, so that cannot happen, and the raise is the check of it -- nothing written is ever retracted."""
    symbols = list(symbols_of_best)
    if not finished:
        if not 0 <= int(n_stable) <= len(symbols):
            raise ValueError(f"n_stable = {n_stable} outside the best hypothesis of {len(symbols)} tokens")
        symbols = symbols[:int(n_stable)]
    text = " ".join(symbols)
    if not text.startswith(prev_text) or (len(text) > len(prev_text) > 0 and text[len(prev_text)] != " "):
        raise ValueError(f"the committed text {text!r} does not extend what was written, {prev_text!r}")
    return text[len(prev_text):], text


HOTWORD_BOOST = 1.5         # --ctc-hotword-boost: the per-token boost of a hotword line that names none (hotwords.read_hotwords)


class CtcBeamOptions:
    """The streaming CTC prefix beam search of ASR sessions (engine.CtcStream): TextSessionPool(ctc_beam=...) and the ASR agent's
    --ctc-beam flags.  beam in [1, 32]; cand (candidates per frame; None: engine.ctc_beam_default_cand) in [1, 32]; nbest (None:
    the beam) in [1, beam]; lm an ngram.NgramLM over source_unigram fused with lm_weight and word_score, or None; bias a
    hotwords.CtcBias over source_unigram weighed by bias_scale, or None.  ValueError here, before any device call, for anything
    the library would refuse."""

    def __init__(self, beam: int, cand: Optional[int] = None, nbest: Optional[int] = None, lm=None, lm_weight: float = 0.5,
                 word_score: float = 0.0, bias=None, bias_scale: float = 1.0):
        self.beam = int(beam)
        self.cand = None if cand is None else int(cand)
        self.nbest = None if nbest is None else int(nbest)
        self.lm, self.lm_weight, self.word_score = lm, float(lm_weight), float(word_score)
        self.bias, self.bias_scale = bias, float(bias_scale)
        if not 1 <= self.beam <= CTC_BEAM_MAX:
            raise ValueError(f"ctc_beam: beam {beam} outside [1, {CTC_BEAM_MAX}]")
        if self.cand is not None and not 1 <= self.cand <= CTC_BEAM_MAX:
            raise ValueError(f"ctc_beam: cand {cand} outside [1, {CTC_BEAM_MAX}]")
        if self.nbest is not None and not 1 <= self.nbest <= self.beam:
            raise ValueError(f"ctc_beam: nbest {nbest} outside [1, beam = {self.beam}]")
        if not (math.isfinite(self.lm_weight) and math.isfinite(self.word_score)):
            raise ValueError("ctc_beam: lm_weight and word_score must be finite")
        if not math.isfinite(self.bias_scale):
            raise ValueError("ctc_beam: bias_scale must be finite")

    def stream_kwargs(self) -> dict:
        """The keywords of engine.CtcStream past (model, head, max_sessions, max_frames)."""
        kw = dict(beam=self.beam, cand=self.cand, nbest=self.nbest)
        if self.lm is not None:
            kw.update(lm=self.lm, lm_weight=self.lm_weight, word_score=self.word_score)
        if self.bias is not None:
            kw.update(bias=self.bias, bias_scale=self.bias_scale)
        return kw


def ctc_beam_flags(args, agent: str = "asr", want_lm: bool = True) -> Optional[CtcBeamOptions]:
    """--ctc-beam K [--ctc-beam-cand C] [--ctc-lm FILE --ctc-lm-weight A --ctc-word-score B] [--ctc-hotwords FILE
    --ctc-hotword-boost S] of the streaming agents -> the options, or None without --ctc-beam.  ValueError: a dependent flag without --ctc-beam, the flags on another agent than the ASR one (the
    S2TT gate and the S2ST path read arg-max token counts), with --word-details (its spans are the arg-max path's), or values out of
    range.  The model file and the hotword file are not read here (the caller reads them over its dictionary and sets .lm /
    .bias)."""
    beam = int(getattr(args, "ctc_beam", 0) or 0)
    cand, lm = getattr(args, "ctc_beam_cand", None), getattr(args, "ctc_lm", None)
    hot, boost = getattr(args, "ctc_hotwords", None), getattr(args, "ctc_hotword_boost", HOTWORD_BOOST)
    if not beam:
        for flag, v, default in (("--ctc-beam-cand", cand, None), ("--ctc-lm", lm, None), ("--ctc-hotwords", hot, None),
                                 ("--ctc-hotword-boost", boost, HOTWORD_BOOST),
                                 ("--ctc-lm-weight", getattr(args, "ctc_lm_weight", 0.5), 0.5),
                                 ("--ctc-word-score", getattr(args, "ctc_word_score", 0.0), 0.0)):
            if v != default:
                raise ValueError(f"{flag} needs --ctc-beam")
        return None
    if agent != "asr":
        raise ValueError(f"--ctc-beam is the streaming ASR agent's: the {agent} agent reads arg-max token counts of the CTC heads")
    if getattr(args, "word_details", False):
        raise ValueError("--ctc-beam cannot be combined with --word-details (its spans are those of the arg-max path)")
    if lm is None and (getattr(args, "ctc_lm_weight", 0.5) != 0.5 or getattr(args, "ctc_word_score", 0.0) != 0.0):
        raise ValueError("--ctc-lm-weight / --ctc-word-score need --ctc-lm")
    if hot is None and boost != HOTWORD_BOOST:
        raise ValueError("--ctc-hotword-boost needs --ctc-hotwords")
    if not math.isfinite(boost):
        raise ValueError("--ctc-hotword-boost must be finite")
    return CtcBeamOptions(beam, cand, None, None, getattr(args, "ctc_lm_weight", 0.5), getattr(args, "ctc_word_score", 0.0))


KEYWORD_THRESHOLD = 1.0     # --ctc-keyword-threshold: tau of a keyword line that names none (keywords.DEFAULT_THRESHOLD)


def ctc_keyword_flags(args, agent: str = "asr") -> Optional[str]:
    """--ctc-keywords FILE [--ctc-keyword-threshold T] of the streaming agents -> the file, or None without the flag.  ValueError:
    the threshold without the file, a threshold that is not a finite number >= 0, the flags on another agent than the ASR one (the
    set is read over source_unigram and spotted on the ASR head; the other agents would ignore it silently).  The file is not read
    here."""
    path, tau = getattr(args, "ctc_keywords", None), float(getattr(args, "ctc_keyword_threshold", KEYWORD_THRESHOLD))
    if path is None:
        if tau != KEYWORD_THRESHOLD:
            raise ValueError("--ctc-keyword-threshold needs --ctc-keywords")
        return None
    if agent != "asr":
        raise ValueError(f"--ctc-keywords is the streaming ASR agent's: the {agent} agent reports no keyword hits")
    if not tau >= 0.0 or not math.isfinite(tau):
        raise ValueError("--ctc-keyword-threshold must be a finite number >= 0")
    return path
