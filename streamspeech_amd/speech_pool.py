"""Concurrent simultaneous S2ST sessions over one session pool: the speech-output agent (StreamSpeechS2STAgent, agent.py; reference
agent/speech_to_speech.streamspeech.agent.py) served many at a time, next to the text kinds of :class:`TextSessionPool`.  Per session,
one :meth:`SpeechSessionPool.step` is exactly one ``StreamSpeechS2STAgent.pushpop(segment)``; across sessions a step is what a text
pool step is (one fbank launch, one encoder step with both CTC heads, the gates on the host, ONE ragged MT continuation shared with
the S2TT writers) and then, for the S2ST sessions that write,
  * ONE ragged MT feature pass for the rows whose final write carries a trailing <pad> (HipModel.batch_mt_features),
  * ONE T2U + unit decoder call with per-row tail-pad masks (HipModel.batch_t2u_units_pad),
  * ONE receptive-field vocoder tail call (HipVocoder.batch_tail; one per duration-prediction setting in use).  On a multi-speaker
    vocoder every session has its own voice (``args.speaker_id``); the voices ride in that one call as per-row speakers.
With ``spoken=True`` at most one unit-spans call (HipModel.batch_unit_spans: one launch, one download) follows each tail call, over
that call's rows, and :meth:`SpeechSessionPool.spoken` answers where each committed word lies in the session's emitted speech.
Driven by one host thread, like the pool.

An S2ST session opened with ``pcm_out="s16le"`` answers :class:`PcmSegment` (16-bit PCM bytes) instead of a SpeechSegment holding a
Python list: the tails of all such writers of a step go through ONE ss_pcm_pack_s16 launch and ONE device-to-host copy into pinned
memory, where a list-fed session pays one ``wav.tolist()`` copy each.  The bytes are frontend.write_wav's rounding of the samples.

An S2ST session opened with ``pcm_out=PcmOut(fmt, sample_rate)`` answers :class:`PcmSegment` in that format at that rate: the tails of
all such writers of a step, and the flush of those that finish without new speech, go through ONE ss_pcm_emit call (the streaming
output resampler over each session's carried history, then the encoder; pcm.PcmEmitter) and ONE device-to-host copy, beside the pack
call of the ``"s16le"`` sessions.  Over an utterance a session's contents concatenate to the encoding of ss_resample over its whole
16-kHz output; between writes it holds back the 10-30 output samples whose filter window is not complete yet."""
import time

import numpy as np
import torch

from .agent import speaker_id_arg
from .frontend import SAMPLE_RATE
from .pcm import PcmEmitter, PcmSegment, pack_s16_host
from .simuleval_shim import SpeechSegment
from .text_pool import KINDS as TEXT_KINDS
from .text_pool import TextSessionPool, _Session
from .text_policy import mt_max_len, s2tt_gate

KINDS = TEXT_KINDS + ("s2st",)
# the S2ST agent's first-pass search (generator_mt): beam 1, max_len_a = 0, max_len_b = 100, min_len = 1 (agent.py)
MAX_LEN_A, MAX_LEN_B, MIN_LEN = 0, 100, 1
DEFAULT_EOS = 2                           # agent.py DEFAULT_EOS: the literal eos the agent tests hypotheses and units against


def vocoder_context(vocoder_cfg, want: int):
    """(context units, receptive field) of the agent's incremental synthesis for --vocoder-context-units `want` (agent.py)."""
    rf = vocoder_cfg.receptive_field_frames() if vocoder_cfg is not None and hasattr(vocoder_cfg, "receptive_field_frames") else None
    ctx = 0 if (rf is None or want == 0) else (want if want > 0 else rf + 8)
    return ctx, rf


def whole_word_cut(tokens, symbol):
    """The agent's whole-word cut of a non-final hypothesis: tokens before the last word-initial ('▁') subword.  -> the cut index j
    (as the agent's loop leaves it: 999999 for an empty list, 0 when only the first subword starts a word or none does)."""
    j = 999999
    for j in range(len(tokens) - 1, -1, -1):
        if symbol(tokens[j]).startswith("▁"):
            break
    return j


class _SpeechSession(_Session):
    def __init__(self, sid, kind, args, engine, dicts, vocoder_cfg, speaker_id=None):
        super().__init__(sid, kind, args, engine, dicts)
        self.speaker_id = speaker_id              # the session's voice on a multi-speaker vocoder (None: single-speaker)
        self.whole_word = args.source_segment_size >= 640
        self.dur_prediction = bool(args.dur_prediction)
        self.vocoder_ctx, self.vocoder_rf = vocoder_context(vocoder_cfg, getattr(args, "vocoder_context_units", -1))
        self.spoken_last = None                   # pools with spoken: (committed tokens, segments) as of the utterance's last write
        self.spoken_words = None                  # the words.Spoken formed of them, once asked

    def reset(self):                          # the S2ST agent's reset()
        super().reset()
        self.prev_output_tokens_mt = None
        self.unit = None
        self.unfinished_wav = None
        self.spoken_rec = None                    # pools with spoken: segments, samples emitted, states seen (made by the first write)


class SpeechSessionPool(TextSessionPool):
    """Up to `max_sessions` concurrent S2ST, S2TT and ASR sessions over one session pool.  `vocoder`: the HipVocoder (or a
    CodeHiFiGANVocoderWithDur, whose .hip is used) every S2ST session synthesises with; without one, S2ST sessions are refused."""
    KINDS = KINDS

    def __init__(self, model, max_sessions: int, max_rows: int, vocoder=None, beam_mt: int = 1, details: bool = False,
                 align: bool = False, search=None, len_penalty: float = 1.0, temperature: float = 1.0, no_repeat_ngram_size: int = 0,
                 spoken: bool = False):
        """spoken: after every tail call of a step ONE unit-spans call (HipModel.batch_unit_spans) over that call's rows maps the
        writers' new units to their decoder states, and spoken(sid) answers the words of the session's committed target tokens with
        the time span each is spoken at in the emitted speech (words.Spoken).  The segments the sessions answer are the same
        either way."""
        super().__init__(model, max_sessions, max_rows, beam_mt=beam_mt, details=details, align=align, search=search,
                         len_penalty=len_penalty, temperature=temperature, no_repeat_ngram_size=no_repeat_ngram_size)
        self.with_spoken = bool(spoken)
        self.vocoder = getattr(vocoder, "hip", vocoder)
        self.t2u_causal = bool(getattr(model, "uni_encoder", False))   # the agent's ctc_generator: t2u_causal = model.uni_encoder
        self._emitter = None                              # pcm.PcmEmitter of the PcmOut sessions, made with the first one's write
        self._flush = []                                  # PcmOut sessions of the step that finish without new speech (_finish_empty)

    def spoken(self, sid: int):
        """The session's words.Spoken as of its last write: the words of all target tokens its utterance has committed with start_ms
        / end_ms on the clock of the speech emitted for the utterance (16-kHz samples / 16: times of the speech, whatever rate or
        format a PcmOut session is answered in), the tail and the total.  None before the first write, after reset(sid), for a
        session that is not s2st, or in a pool without spoken; a finished utterance's words stay until the next one's first write."""
        s = self._get(sid)
        if not self.with_spoken or getattr(s, "spoken_last", None) is None:
            return None
        if s.spoken_words is None:                        # segments are kept by index; the words are formed when asked
            from .words import spoken_from_segments
            s.spoken_words = spoken_from_segments(s.spoken_last[0], s.spoken_last[1], s.dict["target_unigram"], eos=self.model.cfg.eos)
        return s.spoken_words

    def reset(self, sid: int):
        super().reset(sid)
        s = self._get(sid)
        if hasattr(s, "spoken_last"):
            s.spoken_last = s.spoken_words = None

    def _spans_after_tail(self, grp, rows_of, raw, n, info):
        """The ONE unit-spans call after a tail call: grp = the call's (session, units, n_new) rows, rows_of[sid] = the session's row
        in the step's unit pass, raw = that pass's device arg-max ids (row r at ctc_upsample x the prefix sum of n), info = the tail
        call's (first unit synthesised, durations) per row.  Runs before the rows' s.unit moves on."""
        from .words import segments_from_spans
        up = self.model.cfg.ctc_upsample
        off = [0]
        for x in n:
            off.append(off[-1] + int(x))
        idx = [rows_of[s.sid] for s, _, _ in grp]
        if idx == list(range(len(n))):
            sub = raw
        else:                                             # some rows of the unit pass did not write, or wrote in the other tail call
            sub = torch.cat([raw[off[r] * up: off[r + 1] * up] for r in idx], 0)
        spans = self.model.batch_unit_spans(sub, [n[r] for r in idx], [len(u) for _, u, _ in grp], [d for _, d in info],
                                            [f for f, _ in info], [len(u) - k for _, u, k in grp])
        for (s, unit, _), sp in zip(grp, spans):
            rec = s.spoken_rec
            if rec is None:
                rec = s.spoken_rec = {"segments": [], "samples": 0, "seen": 0}
            clock = rec["samples"] // 16
            carried = len(s.unfinished_wav) if s.unfinished_wav is not None else 0
            if carried:
                rec["segments"].append((-1, clock, clock + carried // 16, 0))
                clock += carried // 16
            rec["segments"].extend(segments_from_spans(sp, clock, rec["seen"]))
            rec["seen"] = max(rec["seen"], int(sp.shape[0]))
            rec["samples"] += carried + 320 * int(sp[:, 3].sum())
            s.spoken_last, s.spoken_words = (list(s.tgt_subwords), rec["segments"]), None

    def _check_open(self, kind, args):
        if kind != "s2st":
            return
        if self.vocoder is None:
            raise ValueError("an s2st session needs the pool's vocoder: SpeechSessionPool(..., vocoder=...)")
        if getattr(args, "full_recompute_encoder", False):
            raise ValueError("--full-recompute-encoder: the session pool encodes incrementally by construction")
        speaker_id_arg(args, self.vocoder, "args.speaker_id (--speaker-id)")   # multi-speaker vocoder: refused here, not at the first write

    def _new_session(self, sid, kind, args, dicts):
        if kind != "s2st":
            return super()._new_session(sid, kind, args, dicts)
        return _SpeechSession(sid, kind, args, self.model, dicts, getattr(self.vocoder, "cfg", None),
                              speaker_id_arg(args, self.vocoder))

    # ---- the S2ST agent's policy, split at the pool's shared calls ---------------------------------------------------------------
    def _gate(self, s, src_ids, tgt_ids, n_frames):
        """agent.py policy(): the CTC-count gate (+1 subword in whole-word mode), then the search length of the MT call."""
        n_committed = len(s.tgt_subwords) if s.tgt_subwords is not None else 0
        # subword_tokens + 1 - n_committed == subword_tokens - (n_committed - 1): the S2TT gate with one subword fewer committed
        g = s2tt_gate(len(src_ids), len(tgt_ids), s.src_ctc_prefix_length, s.tgt_ctc_prefix_length,
                      n_committed - (1 if s.whole_word else 0), s.lagging_k1, s.stride_n, s.states.source_finished)
        s.src_ctc_prefix_length, s.tgt_ctc_prefix_length = g.src_prefix_len, g.tgt_prefix_len
        if not g.write:
            return ("read",)
        prefix = list(s.tgt_subwords) if s.tgt_subwords is not None else []
        ml = mt_max_len(len(prefix), n_frames, g.new_tokens, MAX_LEN_A, MAX_LEN_B, self.model.cfg.max_target_positions, MIN_LEN)
        return ("write", prefix, ml, g.new_tokens)

    def _finish_empty(self, s):
        if s.pcm_state is not None:                       # what its resampler still holds goes out with the step's emit call
            self._flush.append(s)
            return ("speech", b"", True, False)
        if s.pcm_out:                                     # a carried unfinished_wav goes out in the session's own format
            carried = s.unfinished_wav.cpu().numpy() if s.unfinished_wav is not None else np.zeros(0, np.float32)
            return ("speech", pack_s16_host(carried).tobytes() if carried.size else b"", True, False)
        return ("speech", list(s.unfinished_wav.tolist()) if s.unfinished_wav is not None else [], True, False)

    def _mt_decide(self, s, toks, view=None):
        """The agent's host decisions between the MT search and T2U.  -> (action or None, n_tokens to keep, n_tail_pad)."""
        fin = s.states.source_finished
        hyp = list(toks)
        tsi = hyp[:-1] if hyp[-1] == DEFAULT_EOS else list(hyp)
        if s.whole_word and not fin:
            j = whole_word_cut(tsi, lambda t: s.dict["target_unigram"][t])
            tsi, hyp = tsi[:j], hyp[:j]
            if j == 0:
                return ("read",), 0, 0
        eos = self.model.cfg.eos
        max_tgt_len = len(hyp) + (1 if s.whole_word else 0)
        tmp = hyp[:-1] if len(hyp) > 0 and hyp[-1] == eos else hyp
        n_tail_pad = max_tgt_len - (len(tmp) + 1)
        assert n_tail_pad in (0, 1), "hypothesis without eos outside whole-word mode (the reference fails here too)"
        prev = [eos] + tmp + [self.model.cfg.pad] * n_tail_pad
        if s.tgt_subwords is not None and list(s.tgt_subwords) == tsi:
            return (("read",) if not fin else self._finish_empty(s)), 0, 0
        s.tgt_subwords = tsi
        if not fin and s.prev_output_tokens_mt is not None:
            if s.prev_output_tokens_mt == prev or len(prev) <= len(s.prev_output_tokens_mt):
                return ("read",), 0, 0
        s.prev_output_tokens_mt = prev
        self._align_note(s, tmp, view)
        return None, len(tmp), n_tail_pad

    def _write_side(self, mine, views, actions):
        t0 = time.perf_counter()
        self._flush = []
        D = self.model.cfg.dec_dim
        rows = []                                         # (session, mt states [n, D], n_tail_pad)
        pads = []                                         # (index in rows, session's encoder view index, tokens)
        for (i, s, prefix, ml, new), toks, fts in mine:
            a, n_tok, n_pad = self._mt_decide(s, prefix + toks, i)
            if a is not None:
                actions[s.sid] = a
                continue
            if n_pad:
                pads.append((len(rows), i, list(s.prev_output_tokens_mt[1:n_tok + 1])))
            rows.append((s, fts[:n_tok + 1], n_pad))
        feats = [f for _, f, _ in rows]
        if pads:
            # the trailing <pad> state of every final whole-word write: ONE ragged feature pass
            enc = torch.cat([views[i] for _, i, _ in pads], 0)
            pf = self.model.batch_mt_features(enc, [views[i].shape[0] for _, i, _ in pads], [t for _, _, t in pads],
                                              [1] * len(pads))
            for (r, _, _), f in zip(pads, pf):
                feats[r] = torch.cat((feats[r], f[-1:]), 0)
        t1 = time.perf_counter()
        voc = []
        if rows:
            n = [f.shape[0] for f in feats]
            packed = torch.zeros((len(rows), max(n), D), dtype=torch.float32, device=feats[0].device)
            for r, f in enumerate(feats):
                packed[r, :f.shape[0]] = f
            if self.with_spoken:
                units, raw_dev = self.model.batch_t2u_units_pad(packed, n, [p for _, _, p in rows], t2u_causal=self.t2u_causal,
                                                                keep_raw=True)
                rows_of = {s.sid: r for r, (s, _, _) in enumerate(rows)}
            else:
                units = self.model.batch_t2u_units_pad(packed, n, [p for _, _, p in rows], t2u_causal=self.t2u_causal)
            for (s, _, _), toks in zip(rows, units):
                fin = s.states.source_finished
                if len(toks) == 0:
                    actions[s.sid] = ("read",) if not fin else self._finish_empty(s)
                    continue
                if toks[-1] == DEFAULT_EOS:
                    toks = toks[:-1]
                unit = []
                for c in toks:
                    u = s.dict["tgt"][c].replace("<s>", "").replace("</s>", "")
                    if u != "":
                        unit.append(int(u))
                cur = unit if s.unit is None else unit[len(s.unit):]
                if len(unit) < 1 or len(cur) < 1:
                    actions[s.sid] = ("read",) if not fin else self._finish_empty(s)
                    continue
                voc.append((s, unit, len(cur)))
        t2 = time.perf_counter()
        handover, raw = 0.0, []                           # raw: (session, tail) of the pcm_out writers, packed together below
        own = []                                          # the same of the PcmOut writers, emitted together below
        tail_calls = span_calls = 0
        spans_s = 0.0
        for dp in (True, False):
            grp = [v for v in voc if v[0].dur_prediction == dp]
            if not grp:
                continue
            tail_calls += 1
            # a multi-speaker vocoder: the rows' voices go along in the same call (no grouping by voice)
            spk = {"speakers": [s.speaker_id for s, _, _ in grp]} if getattr(self.vocoder, "num_speakers", 0) else {}
            tails, tail_info = self.vocoder.batch_tail([u for _, u, _ in grp], [k for _, _, k in grp], [s.vocoder_ctx for s, _, _ in grp],
                                                       [s.vocoder_rf for s, _, _ in grp], dur_prediction=dp, **spk)
            if self.with_spoken:
                ts = time.perf_counter()
                self._spans_after_tail(grp, rows_of, raw_dev, n, tail_info)
                span_calls += 1
                spans_s += time.perf_counter() - ts
            th = time.perf_counter()
            for (s, unit, _), wav in zip(grp, tails):
                if s.unfinished_wav is not None and len(s.unfinished_wav) > 0:
                    wav = torch.cat((s.unfinished_wav, wav), 0)
                s.unit = unit
                if s.pcm_state is not None:
                    own.append((s, wav))
                    continue
                if s.pcm_out:
                    raw.append((s, wav))
                    continue
                # a final write (new_tokens == -1) ends with the agent's reset(), which runs BEFORE the agent builds its segment and
                # clears source_finished: no write says finished=True
                actions[s.sid] = ("speech", wav.tolist(), False, s.states.source_finished)
            handover += time.perf_counter() - th
        th = time.perf_counter()
        n_out = self._pack_out(raw, actions) if raw else 0
        emit_calls, emit_bytes = self._emit_out(own, self._flush, actions) if own or self._flush else (0, 0)
        self._flush = []
        t3 = time.perf_counter()
        # handover_s: from the tails' views in hand to the contents the segments carry (lists or bytes), both routes; it lies inside
        # vocoder_s, which keeps its meaning (the tail calls and what follows them)
        self._side_times = {"mt_features_s": t1 - t0, "units_s": t2 - t1, "vocoder_s": t3 - t2, "handover_s": handover + (t3 - th),
                            "speech_writers": len(voc), "vocoder_tail_calls": tail_calls, "pcm_pack_calls": 1 if n_out else 0,
                            "pcm_bytes_out": 2 * n_out,
                            "pcm_emit_calls": emit_calls, "pcm_emit_bytes_out": emit_bytes}
        if self.with_spoken:
            self._side_times.update({"spans_s": spans_s, "span_calls": span_calls})

    def _emit_out(self, own, flush, actions):
        """The tails of a step's PcmOut writers and the flushes of its PcmOut sessions that finish without new speech -> bytes at
        each session's rate and format: ONE pcm_emit call over all of them, the tails taken where they lie, and ONE device-to-host
        copy (pcm.PcmEmitter).  A final write ends the utterance, so it flushes too.  -> (calls made: 0 or 1, bytes out)."""
        if self._emitter is None:
            self._emitter = PcmEmitter(self.model)
        items = [(s.pcm_state, wav.contiguous(), bool(s.states.source_finished)) for s, wav in own]
        for s in flush:
            carried = s.unfinished_wav if s.unfinished_wav is not None and len(s.unfinished_wav) > 0 else None
            items.append((s.pcm_state, carried, True))
        before = self._emitter.calls
        contents = self._emitter.emit(items)
        for (s, _), content in zip(own, contents):
            actions[s.sid] = ("speech", content, False, s.states.source_finished)
        for s, content in zip(flush, contents[len(own):]):
            actions[s.sid] = ("speech", content, True, False)
        return self._emitter.calls - before, sum(len(c) for c in contents)

    def _pack_out(self, raw, actions) -> int:
        """The tails of a step's pcm_out writers -> 16-bit PCM bytes: ONE ss_pcm_pack_s16 launch over all of them and ONE
        device-to-host copy into pinned memory, then a bytes object per session.  -> samples packed."""
        tails = [w for _, w in raw]
        n = [int(w.numel()) for w in tails]
        total = sum(n)
        if total:
            # views of one packed buffer that follow each other (one batch_tail call) are packed where they lie; otherwise (two
            # duration settings in one step, a carried wav) they are gathered first
            adjacent = all(a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
                           and a.data_ptr() + 4 * a.numel() == b.data_ptr() for a, b in zip(tails, tails[1:]))
            if adjacent and tails[0].is_contiguous():
                src = tails[0].new_empty(0).set_(tails[0].untyped_storage(), tails[0].storage_offset(), (total,))
            else:
                src = torch.cat(tails, 0)
            cuda = src.device.type == "cuda"
            if getattr(self, "_out_dev", None) is None or self._out_dev.numel() < total:
                self._out_dev = torch.empty((2 * total,), dtype=torch.int16, device=src.device)
                self._out_host = torch.empty((2 * total,), dtype=torch.int16, pin_memory=cuda)
            self.model.pcm_pack_s16(src, self._out_dev[:total])
            self._out_host[:total].copy_(self._out_dev[:total], non_blocking=True)
            if cuda:
                torch.cuda.current_stream().synchronize()    # the bytes below are read from the pinned buffer: the copy must have landed
        off = 0
        for (s, _), k in zip(raw, n):
            content = self._out_host[off:off + k].numpy().tobytes() if k else b""
            off += k
            actions[s.sid] = ("speech", content, False, s.states.source_finished)
        return total

    def _segment(self, s, a):
        pcm_out = s.pcm_out
        fmt, rate = (pcm_out.fmt, pcm_out.sample_rate) if s.pcm_state is not None else (pcm_out, SAMPLE_RATE)
        if a[0] == "write":                               # the front-end's early return of a finished source: no speech
            if pcm_out:
                return PcmSegment(index=0, content=b"", fmt=fmt, sample_rate=rate, finished=True)
            return SpeechSegment(index=0, content=[], sample_rate=SAMPLE_RATE, finished=True)
        _, content, finished, done = a
        if done:                                          # the agent's reset(): a fresh utterance, its slot back to the pool
            s.reset()
            self._release(s)
        if pcm_out:
            return PcmSegment(index=0, content=content, fmt=fmt, sample_rate=rate, finished=finished)
        return SpeechSegment(index=0, content=content, sample_rate=SAMPLE_RATE, finished=finished)
