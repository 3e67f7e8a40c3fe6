"""Concurrent streaming ASR and simultaneous S2TT sessions over one session pool (engine.StreamPool): the text-side agents
(agent/speech_to_text.asr.streamspeech.agent.py, agent/speech_to_text.s2tt.streamspeech.agent.py; agent_text.py here) served many
at a time.  Per session, one :meth:`TextSessionPool.step` is exactly one ``agent.pushpop(segment)`` of the matching single-session
agent; across sessions a step is
  * ONE fbank launch for the new frames of every session, whatever its source rate (ss_batch_fbank_frames when all are at 16 kHz,
    else ss_batch_fbank_frames_sr, which resamples inside the row's workgroup from the source-rate history),
  * ONE batched encoder step and both CTC heads (StreamPool.forward / ctc_both; ASR sessions read head 0),
  * the read/write gate of each session on the host (text_policy.s2tt_gate),
  * ONE ragged greedy continuation of the committed prefix of every writing S2TT session (HipModel.batch_mt_continue).
Driven by one host thread, like the pool.

A session opened with ``pcm_in=PcmFormat(...)`` is fed raw PCM bytes (push_pcm) instead of SimulEval's lists of floats: the step copies
the chunks of all such sessions into one pinned arena, uploads it ONCE and decodes every chunk into its session's device history in ONE
ss_pcm_scatter launch (streamspeech_amd/pcm.py), then runs the same single fbank launch.  The decoded samples are the bits the list
route uploads, so everything downstream is unchanged; list-fed sessions run the code they always ran, in the same step.

A session opened with ``mp3_in=True`` (or ``{"join": True}`` for a stream captured mid-way) is fed MP3 bytes as they come off the
wire (push_mp3), in chunks of any size.  The bitstream is parsed on the host at push time (mp3.Mp3Stream: cheap, and it is what tells
the admission check how many samples the chunk releases); the step copies the records of all such sessions into one pinned arena,
uploads it ONCE and ONE ss_mp3_stream_synthesize call decodes them against each session's carried IMDCT blocks straight into its
device history -- the bits of the whole-file decoder.  The three routes may share a step.

A ``pcm_in`` session opened with ``endpoint=Endpoint(...)`` is a continuous stream the pool cuts into utterances itself
(streamspeech_amd/endpoint.py): after the scatter, ONE ss_vad_scan launch scans the new frames of every such session, one small
download brings the result records, and the host decides what each session commits.  An idle session commits nothing and holds no
slot; inside an utterance the session is a plain ``pcm_in`` session fed exactly the samples each step commits, with finished=True in
the step that reaches the cut, after which the pool itself resets it for the next utterance."""
import math
import time
from typing import Dict, Optional

import torch

from .engine import MT_BEAM_MAX, SamplingOptions, SearchOptions, plan_beam_groups, sampling_stream_key
from .frontend import SAMPLE_RATE, OnlineFeatureExtractor, unsettled_fbank_frames
from . import endpoint as EP
from .pcm import PcmArena, PcmFormat, PcmOut
from .simuleval_shim import AgentStates, EmptySegment, TextSegment
from .text_policy import CtcBeamOptions, asr_beam_emit, mt_max_len, s2tt_gate
from .words import CtcDetails, words_from_ctc

KINDS = ("s2tt", "asr")
# the text agents' first-pass search: beam 1, max_len_a = 1, max_len_b = 200, min_len = 1 (agent_text.py)
MAX_LEN_A, MAX_LEN_B, MIN_LEN = 1, 200, 1


def _no_event_result(consumed: int, last_speech: int, mode: int):
    """The result record of a scan over no frames, made on the host: nothing consumed, no event."""
    from .lib import SSVadResult
    return SSVadResult(int(consumed), -1, -1, int(last_speech), 0, int(mode))


def _encoder_out_len(T: int) -> int:
    t1 = (T + 2 * 2 - 5) // 2 + 1
    return (t1 + 2 * 2 - 5) // 2 + 1


def fbank_frames_after(kind_sr: int, n_samples: int, shift_ms: int = 10, window_ms: int = 25) -> int:
    """fbank rows the agent's front-end makes of `n_samples` samples at `kind_sr` Hz (OnlineFeatureExtractor, then the resampler)."""
    per_shift = int(shift_ms * kind_sr / 1000)
    nf = int((n_samples - (window_ms - shift_ms) * kind_sr / 1000) // per_shift)
    if nf <= 0:
        return 0
    if kind_sr == SAMPLE_RATE:
        return nf
    effective = int(nf * shift_ms * kind_sr / 1000 + (window_ms - shift_ms) * kind_sr / 1000)
    g = math.gcd(int(kind_sr), SAMPLE_RATE)
    up, down = SAMPLE_RATE // g, int(kind_sr) // g
    n16 = -(-effective * up // down)
    return 0 if n16 < 400 else 1 + (n16 - 400) // 160


class _Session:
    def __init__(self, sid, kind, args, engine, dicts):
        self.sid, self.kind, self.args = sid, kind, args
        self.sr = int(args.sample_rate)
        self.attn_chunk = args.source_segment_size // 40
        self.conv_chunk = 16 if self.attn_chunk >= 16 else 8
        self.lagging_k1, self.stride_n = args.lagging_k1, args.stride_n
        self.tail = unsettled_fbank_frames(self.sr, SAMPLE_RATE, int(args.shift_size * SAMPLE_RATE / 1000))
        self.fe = OnlineFeatureExtractor(args, engine)
        self.dict = dicts
        self.states = AgentStates()
        self.slot = None
        self.pending = False
        self.pcm_in = None                    # a PcmFormat: the session is fed by push_pcm, and counts samples (fe.n_pcm) instead of
        self.pcm_out = None                   # keeping them in states.source; "s16le": it answers PcmSegment (speech_pool.py)
        self.pcm_state = None                 # a pcm.PcmOutState when pcm_out is a PcmOut: carry buffer, taps, counters (speech_pool.py)
        self.pcm_chunk = None                 # (byte view, frames) pushed for the next step
        self.mp3_in = None                    # {"join": bool}: the session is fed by push_mp3 and counts samples as a PCM-fed one does
        self.mp3 = None                       # its mp3.Mp3Stream (host bitstream state), made at open()
        self.mp3_state = None                 # its device state: the IMDCT blocks of the last two granules (mp3.stream_state)
        self.mp3_chunk = None                 # the mp3.Mp3Chunk parsed by push_mp3 for the next step
        self.mp3_held = 0                     # samples decoded into fe._dev past fe.n_pcm and not released yet (gapless hold-back)
        self.ep = None                        # an endpoint.EndpointState: the pool cuts the session's stream into utterances
        self.details = None                   # a words.CtcDetails of the last step that encoded the session (pools with details)
        self.alignment = None                 # the words.AlignedWord list of the utterance's committed target tokens (pools with align)
        self.nbest = None                     # pools with ctc_beam: the engine.CtcHypothesis list of the last finished utterance
        self.spot_hits = []                   # pools with spot: the keywords.KeywordHit that arrived since hits(sid) was last asked
        self.reset()

    def n_source(self) -> int:
        """Samples received so far: every host decision that reads len(states.source) of a list-fed session reads this."""
        if self.mp3_in is not None:
            return self.fe.n_pcm + (self.mp3_chunk.released if self.mp3_chunk is not None else 0)
        if self.pcm_in is None:
            return len(self.states.source)
        if self.ep is not None:               # an endpointed session counts what its utterance has committed, not what it was sent
            return self.fe.n_pcm
        return self.fe.n_pcm + (self.pcm_chunk[1] if self.pcm_chunk is not None else 0)

    def reset(self):                          # the agent's reset()
        self.mt_writes = 0                    # sampling: writes of this utterance so far, the second half of the stream key
        self.align_rec = []                   # (committed tokens placed so far, the words of one write): frozen once made
        self.tgt_subwords = None
        self.src_ctc_prefix_length = 0
        self.tgt_ctc_prefix_length = 0
        self.asr_text = ""
        self.tgt_text = ""
        self.partial = None                   # pools with ctc_beam: the symbols of the utterance's current best hypothesis
        self.ctc_frames = 0                   # ... and the encoder rows its search has consumed
        self.spot_frames = 0                  # pools with spot: the encoder rows the utterance's spotter has consumed
        self.states.reset()
        self.fe.clear_cache()
        if self.pcm_state is not None:        # a fresh utterance: nothing received, nothing emitted, nothing carried
            self.pcm_state.reset()
        if self.mp3 is not None:              # a fresh utterance is a fresh stream: bitstream state and carried blocks start over
            self.mp3.reset()
        self.mp3_state, self.mp3_chunk, self.mp3_held = None, None, 0


class TextSessionPool:
    """Up to `max_sessions` concurrent ASR / S2TT sessions, each of at most `max_rows` encoder output rows (~40 ms each)."""
    KINDS = KINDS

    def __init__(self, model, max_sessions: int, max_rows: int, beam_mt: int = 1, details: bool = False, align: bool = False,
                 search: Optional[SearchOptions] = None, len_penalty: float = 1.0, temperature: float = 1.0,
                 no_repeat_ngram_size: int = 0, ctc_beam: Optional[CtcBeamOptions] = None, spot=None, spot_max_hits: int = 64):
        """beam_mt > 1: the step's one ragged continuation is a beam search behind every writer's committed prefix
        (HipModel.batch_mt_beam_continue, the agents' --beam-mt); hypothesis 0's tokens and states go on as the greedy ones do.
        details: the step's one CTC call is the scored form, and details(sid) answers the words of both heads with their time
        spans, confidences and stability (words.py); the segments the sessions answer are the same either way.
        align: after the step's writes ONE ragged teacher-forced pass (HipModel.batch_mt_attention, peaks only) places the target
        tokens every session committed in this step in source time by the text decoder's cross-attention, over the encoder rows
        the write saw; alignment(sid) answers the words (words.AlignedWord), frozen once made.  The pass runs after everything
        else of the step, on outputs of its own: the segments the sessions answer are the same either way.
        search (an engine.SearchOptions), or the three keywords len_penalty / temperature / no_repeat_ngram_size: the agents'
        --lenpen, --temperature and --no-repeat-ngram-size.  With one of them off its default the step's continuation is the beam
        search behind the prefix at beam_mt = 1 too; every committed token was chosen under the same ban, so a session's prefix
        never repeats an n-gram and the call never refuses it.
        search=engine.SamplingOptions(topk, topp, seed, search=SearchOptions or None): the agents' --sampling.  Every write draws
        beam_mt chains behind the writer's committed prefix (HipModel.batch_mt_sample_continue) and commits the best-scoring one;
        a write's stream key is engine.sampling_stream_key(session id, the session's writes so far), so a replayed session samples
        the same and two sessions never share a stream.
        ctc_beam (a text_policy.CtcBeamOptions): ASR sessions decode with the resumable CTC prefix beam search in place of the
        arg-max frame path -- the pool owns one engine.CtcStream on head 0 whose slots are the pool's, and after the encoder ONE
        advance serves every ASR session of the step, over the rows the encoder has made final (all rows, with final, for a
        session whose source is finished).  Such a session writes the new text of the prefix every beam string shares, and the
        rest of the best hypothesis at the end: the writes of an utterance add up to its final best hypothesis and none is ever
        retracted.  partial(sid) answers the current best hypothesis, nbest(sid) the last finished utterance's n-best.  S2TT
        sessions (and a subclass's kinds) run as without the option, and so does every launch of a pool built without it.  Not
        with details (its spans are the arg-max path's).
        spot (a keywords.CtcKeywords over the source dictionary): ASR sessions are searched for the set's phrases as they speak --
        the pool owns one engine.CtcSpotStream on head 0 whose slots are the pool's, and after the encoder ONE advance serves every
        ASR session of the step, over the rows the encoder has made final (as the prefix search: all rows, with final, for a
        session whose source is finished), at most spot_max_hits hits per session and step.  hits(sid) answers what arrived.
        With the greedy sessions, with ctc_beam and with details; it reads the encoder rows and touches none of their outputs,
        and a pool built without it launches what it always did."""
        if ctc_beam is not None and details:
            raise ValueError("ctc_beam cannot be combined with details: the words' spans are those of the arg-max path")
        if ctc_beam is not None and not isinstance(ctc_beam, CtcBeamOptions):
            raise ValueError("ctc_beam: a text_policy.CtcBeamOptions")
        if not 1 <= int(beam_mt) <= MT_BEAM_MAX:
            raise ValueError(f"beam_mt {beam_mt} outside [1, {MT_BEAM_MAX}]")
        self.beam_mt = int(beam_mt)
        if search is not None and (len_penalty, temperature, no_repeat_ngram_size) != (1.0, 1.0, 0):
            raise ValueError("give search= or the three keywords, not both")
        self.sampling = None                   # search=SamplingOptions(...): every write samples beam_mt chains behind the prefix
        if isinstance(search, SamplingOptions):
            self.sampling, search = search, search.search
        self.search = search if search is not None else SearchOptions(len_penalty, temperature, no_repeat_ngram_size)
        self.model = model.hip if hasattr(model, "hip") else model
        self.with_details = bool(details)
        self.with_align = bool(align)
        self._align_jobs: list = []            # (session, encoder view index, committed tokens, tokens placed before, record list, t0_ms)
        self.pool = self.model.stream_pool(max_sessions, max_rows, scores=True) if details else self.model.stream_pool(max_sessions, max_rows)
        self.max_sessions, self.max_rows = int(max_sessions), int(max_rows)
        self.ctc_stream = None                 # pools with ctc_beam: the searches of the ASR sessions, slot for slot
        self._stream_rows: list = []           # ... and the rows each of the step's searches moved over
        if ctc_beam is not None:
            from .engine import CtcStream
            from .lib import CTC_BEAM_MAX_FRAMES
            self.ctc_stream = CtcStream(self.model, 0, self.max_sessions, min(self.max_rows, CTC_BEAM_MAX_FRAMES), **ctc_beam.stream_kwargs())
        self.spot_stream = None                # pools with spot: the spotters of the ASR sessions, slot for slot
        self._spot_rows: list = []             # ... and the rows each of the step's spotters moved over
        self._spot_lost = 0                    # ... and the hits of the step past spot_max_hits
        self.spot_max_hits = int(spot_max_hits)
        if spot is not None:
            from .engine import CtcSpotStream
            self.spot_stream = CtcSpotStream(self.model, 0, self.max_sessions, spot)
        self.sessions: Dict[int, _Session] = {}
        self.free = list(range(self.max_sessions))
        self._next = 0
        self.last_step: dict = {}              # timings / counts of the last step (tools/pooled_text_bench.py)
        self._arena = None                     # the pinned staging buffer of the PCM-fed sessions' chunks, made with the first one
        self._mp3_arena = None                 # the same for the records of the MP3-fed sessions
        self._side_times: dict = {}            # timings a subclass's write side adds to last_step
        self._vad_dev = self._vad_host = None  # the result records of a step's endpoint scan: device buffer and its pinned copy

    # ---- lifecycle ------------------------------------------------------------------------------------------------------------
    def open(self, kind: str, args, dicts: Optional[dict] = None, pcm_in: Optional[PcmFormat] = None,
             pcm_out=None, mp3_in=None, endpoint=None) -> int:
        """A new session; `args` are the agent's own parsed flags (segment size, lagging_k1, stride_n, sample rate, chunk sizes).
        `dicts` overrides the dictionaries the agent would load from the flags (keys source_unigram / target_unigram).
        pcm_in=PcmFormat(...): the session is fed raw PCM at args.sample_rate through push_pcm() and nothing else.
        pcm_out="s16le" (s2st sessions only): it answers PcmSegment with 16-bit PCM bytes instead of SpeechSegment with a list.
        pcm_out=PcmOut(fmt, sample_rate) (s2st sessions only): it answers PcmSegment in that format at that rate, resampled and
        encoded on the device with a short history carried per session (speech_pool.py); no other string is accepted.
        mp3_in=True or {"join": bool}: the session is fed an MP3 stream whose sample rate is args.sample_rate through push_mp3() and
        nothing else (join: the stream was captured mid-way, mp3.Mp3StreamDecoder).  Not together with pcm_in.
        endpoint=Endpoint(...) (with pcm_in only): the stream is continuous and the pool cuts it into utterances (endpoint.py);
        push_pcm(finished=True) then ends the stream, not an utterance."""
        if kind not in self.KINDS:
            raise ValueError(f"session kind {kind!r}: one of {self.KINDS}")
        if pcm_in is not None and not isinstance(pcm_in, PcmFormat):
            raise ValueError(f"pcm_in is a PcmFormat, not {pcm_in!r}")
        if pcm_out is not None and ((not isinstance(pcm_out, PcmOut) and not (isinstance(pcm_out, str) and pcm_out == "s16le"))
                                    or kind != "s2st"):
            raise ValueError(f"pcm_out={pcm_out!r} for a {kind} session: only \"s16le\" or a PcmOut, and only for s2st sessions")
        if mp3_in is not None and mp3_in is not False:
            if pcm_in is not None:
                raise ValueError("mp3_in and pcm_in exclude each other: a session is fed one way for its whole life")
            if mp3_in is True:
                mp3_in = {"join": False}
            if not isinstance(mp3_in, dict) or set(mp3_in) - {"join"}:
                raise ValueError(f"mp3_in is True or {{\"join\": bool}}, not {mp3_in!r}")
            mp3_in = {"join": bool(mp3_in.get("join", False))}
        else:
            mp3_in = None
        ep_params = None
        if endpoint is not None:
            if pcm_in is None and mp3_in is None:
                raise ValueError("endpoint needs pcm_in: the scan runs over the session's decoded PCM history")
            if mp3_in is not None:
                raise ValueError("endpoint with mp3_in is not served: the gapless hold-back shares the uncommitted tail of the history")
            if not isinstance(endpoint, EP.Endpoint):
                raise ValueError(f"endpoint is an Endpoint, not {endpoint!r}")
            ep_params = endpoint.params(int(args.sample_rate), args.shift_size, args.window_size,
                                        self._fit_samples(int(args.sample_rate), args.shift_size, args.window_size))
        self._check_open(kind, args)
        if dicts is None:
            from .agent import load_dictionaries
            dicts = load_dictionaries(args, self.model.cfg)
        sid = self._next
        self._next += 1
        s = self._new_session(sid, kind, args, dicts)
        s.pcm_in, s.pcm_out = pcm_in, pcm_out
        if isinstance(pcm_out, PcmOut):
            from .pcm import PcmOutState
            s.pcm_state = PcmOutState(pcm_out, self.model)
        if mp3_in is not None:
            from .mp3 import Mp3Stream
            s.mp3_in, s.mp3 = mp3_in, Mp3Stream(mp3_in["join"], name=f"session {sid}")
        if ep_params is not None:
            s.ep = EP.EndpointState(endpoint, ep_params, self.model.device)
        self.sessions[sid] = s
        return sid

    def _check_open(self, kind: str, args):
        """Refusals of open() beyond the kind (subclasses: ValueError)."""

    def _new_session(self, sid, kind, args, dicts):
        return _Session(sid, kind, args, self.model, dicts)

    def reset(self, sid: int):
        """The agent's reset(): the session starts a fresh utterance (its slot goes back to the pool until it next has audio)."""
        s = self._get(sid)
        s.reset()
        s.details = None
        s.alignment = None
        s.pending = False
        s.pcm_chunk = None
        self._release(s)
        if s.ep is not None:                  # a fresh stream: frame numbering, noise floor and the utterance list start over
            s.ep.reset()

    def close(self, sid: int):
        s = self._get(sid)
        self._release(s)
        s.pcm_state = None
        if s.mp3 is not None:
            s.mp3.close()
            s.mp3, s.mp3_state, s.mp3_chunk = None, None, None
        del self.sessions[sid]

    def details(self, sid: int):
        """The session's words.CtcDetails as of the last step that encoded it: source and target words with start_ms / end_ms on the
        session's own clock (an endpointed session: the stream's), confidence and `stable`.  None before the first such step, after
        reset(sid), or in a pool without details."""
        return self._get(sid).details if self.with_details else None

    def alignment(self, sid: int):
        """The words (words.AlignedWord) of all target tokens the session's utterance has committed, each with the source time span
        the text decoder's cross-attention pointed at when the token was written (an endpointed session: on the stream's clock) and
        its focus.  A write adds words and never changes one.  None before the first write, after reset(sid), or in a pool without
        align; a finished utterance's words stay until then or until the next utterance's first write."""
        return self._get(sid).alignment if self.with_align else None

    @staticmethod
    def _t0_ms(s: _Session) -> int:
        """The session clock's time of its utterance's first sample: 0, or for an endpointed session the utterance's first stream
        sample (an utterance that ended this step: its own)."""
        if s.ep is None:
            return 0
        a = s.ep.utterances[-1]["start"] if s.ep.final else s.ep.utt_start
        return int(a) * 1000 // s.sr

    def _align_note(self, s: _Session, tokens, view):
        """A writer committed `tokens` (all of its utterance's, no </s>): its new ones join the step's attention pass, over the
        step's encoder view `view` (the writer's index among the step's encoded sessions)."""
        if not self.with_align:
            return
        if view is None:
            raise ValueError("a pool with align needs the writer's encoder view index")
        rec = s.align_rec
        while rec and rec[-1][0] > len(tokens):       # (a whole-word cut below what was placed: placed again)
            rec.pop()
        done = rec[-1][0] if rec else 0
        if len(tokens) > done:
            self._align_jobs.append((s, int(view), [int(t) for t in tokens], done, rec, self._t0_ms(s)))

    def _align_flush(self, views) -> int:
        """The step's ONE attention pass over every noted writer -> 1 if it ran."""
        jobs, self._align_jobs = self._align_jobs, []
        if not jobs:
            return 0
        from .words import words_from_attention
        enc = torch.cat([views[i] for _, i, _, _, _, _ in jobs], 0) if len(jobs) > 1 else views[jobs[0][1]].contiguous()
        res = self.model.batch_mt_attention(enc, [int(views[i].shape[0]) for _, i, _, _, _, _ in jobs], [t[:-1] for _, _, t, _, _, _ in jobs],
                                            first=[d for _, _, _, d, _, _ in jobs], want_matrix=False)
        for (s, _, toks, done, rec, t0), (_, peak, prob, _, _) in zip(jobs, res):
            rec.append((len(toks), words_from_attention(toks[done:], peak.tolist(), prob.tolist(), s.dict["target_unigram"], t0_ms=t0,
                                                        eos=self.model.cfg.eos)))
            s.alignment = [w for _, ws in rec for w in ws]
        return 1

    def _set_details(self, s: _Session, src, tgt, n_final: int):
        t0 = self._t0_ms(s)
        fin = bool(s.states.source_finished)
        s.details = CtcDetails(*(words_from_ctc(r[0], r[1], r[2], r[3], s.dict[name], n_final=n_final, finished=fin, t0_ms=t0)
                                 for r, name in ((src, "source_unigram"), (tgt, "target_unigram"))))

    def _get(self, sid) -> _Session:
        if sid not in self.sessions:
            raise KeyError(f"no open session {sid}")
        return self.sessions[sid]

    def partial(self, sid: int):
        """A pool with ctc_beam: the symbols of the ASR session's current best hypothesis, its unstable tail included -- for
        display; what the session has WRITTEN is the stable part.  None before the utterance's first encoded step."""
        return self._get(sid).partial if self.ctc_stream is not None else None

    def nbest(self, sid: int):
        """A pool with ctc_beam: the n-best (engine.CtcHypothesis, best first) of the ASR session's last finished utterance."""
        return self._get(sid).nbest if self.ctc_stream is not None else None

    def hits(self, sid: int):
        """A pool with spot: the keyword hits (keywords.KeywordHit) of the ASR session that arrived since this was last asked, in
        the order they were reported (a step's by end, keyword, start); start_ms / end_ms on the session's own clock (an
        endpointed session: the stream's), placed as words.py places words.  They survive reset(sid): a finished utterance's last
        hits arrive with its last step.  None in a pool without spot."""
        if self.spot_stream is None:
            return None
        s = self._get(sid)
        got, s.spot_hits = s.spot_hits, []
        return got

    def _slot_reset(self, slot: int):
        self.pool.reset(slot)
        if self.spot_stream is not None:       # ... and its spotter
            self.spot_stream.reset(slot)
        if self.ctc_stream is not None:        # wherever the encoder's slot starts over, so does its search
            self.ctc_stream.reset(slot)

    def _release(self, s: _Session):
        if s.slot is not None:
            self._slot_reset(s.slot)
            self.free.append(s.slot)
            s.slot = None

    def _acquire(self, s: _Session):
        if s.slot is None:
            if not self.free:
                raise ValueError(f"session {s.sid}: all {self.max_sessions} slots of the pool are taken")
            s.slot = self.free.pop(0)
            self._slot_reset(s.slot)
            self.pool.set_tail(s.slot, s.tail)

    # ---- one call per session ---------------------------------------------------------------------------------------------------
    def _frames(self, s: _Session, extra: int = 0) -> int:
        return fbank_frames_after(s.sr, s.n_source() + extra, s.args.shift_size, s.args.window_size)

    def _admit(self, items):
        """The capacity check of a set of pushes [(session, segment)] -- or [(session, new frames)] for PCM chunks -- against
        everything already pushed for this step: raises ValueError naming the first session refused and changes nothing.  A session
        is refused when it is already pushed, when its audio would pass max_rows encoder rows, or when it needs a slot (frames, none
        held) and the free slots are spoken for."""
        seen = set()
        for s, _ in items:
            if s.pending or s.sid in seen:
                raise ValueError(f"session {s.sid}: already pushed in this step")
            seen.add(s.sid)
        # slots the step already needs: pushed sessions with frames and no slot (a finished agent does not encode)
        need = sum(1 for s in self.sessions.values()
                   if s.pending and s.slot is None and not s.states.target_finished and self._frames(s) > 0)
        for s, seg in items:
            if s.states.target_finished:
                continue
            T = self._frames(s, seg if isinstance(seg, int) else len(getattr(seg, "content", None) or []))
            if T > 0 and _encoder_out_len(T) > self.max_rows:
                raise ValueError(f"session {s.sid}: {_encoder_out_len(T)} encoder rows would pass the pool's max_rows {self.max_rows}")
            if T > 0 and s.slot is None:
                need += 1
                if need > len(self.free):
                    raise ValueError(f"session {s.sid}: no free slot -- the {self.max_sessions} slots of the pool are held or "
                                     f"needed by other sessions of this step")

    def push(self, sid: int, segment):
        """The agent's push(), checked against the pool's capacity first (_admit): a refused push raises ValueError naming the
        session and changes nothing; the sessions pushed before and after it step as usual."""
        s = self._get(sid)
        self._check_route([s], pcm=False)
        self._admit([(s, segment)])
        s.states.update_source(segment)
        s.pending = True

    def _check_route(self, sessions, pcm: bool, mp3: bool = False):
        """A session is fed one way for its whole life: segments (push / step), raw PCM (push_pcm) or an MP3 stream (push_mp3).
        ValueError, nothing changes."""
        for s in sessions:
            if (s.mp3_in is not None) != mp3:
                raise ValueError(f"session {s.sid}: opened with mp3_in={s.mp3_in!r}, it is fed by "
                                 + ("push_mp3() only" if s.mp3_in is not None else
                                    "push_pcm() only" if s.pcm_in is not None else "push() / step() segments only"))
            if mp3:
                continue
            if (s.pcm_in is not None) != pcm:
                raise ValueError(f"session {s.sid}: opened with pcm_in={s.pcm_in!r}, it is fed by "
                                 + ("push_pcm() only" if s.pcm_in is not None else "push() / step() segments only"))

    def push_pcm(self, sid: int, data, finished: bool = False):
        """push() for a session opened with pcm_in: `data` holds the new frames in the session's format -- bytes, bytearray, memoryview,
        or a C-contiguous NumPy / CPU torch array of the matching dtype; a partial frame is ValueError.  The same admission check as
        push(), counted in frames.  The bytes are copied at the next step(), so a mutable buffer must stay as it is until then."""
        from .pcm import as_bytes
        s = self._get(sid)
        self._check_route([s], pcm=True)
        mv = as_bytes(data, s.pcm_in)
        frames = s.pcm_in.frames(mv.nbytes)
        if s.ep is not None:
            return self._push_endpoint(s, mv, frames, finished)
        self._admit([(s, frames)])
        s.pcm_chunk = (mv, frames)
        s.states.source_finished = bool(finished)
        s.pending = True

    def push_mp3(self, sid: int, data, finished: bool = False):
        """push() for a session opened with mp3_in: `data` holds the next bytes of its MP3 stream, any number of them (bytes,
        bytearray, memoryview or a uint8 array); finished=True ends the stream (a complete last frame is then accepted without its
        look-ahead).  The bitstream is parsed here, which tells how many samples the chunk releases; the same admission check as
        push() runs on that count.  A refused push -- route, a stream the decoder refuses (mp3.Mp3Error), a sample rate other than
        args.sample_rate (ValueError naming both, at the first accepted header), admission -- raises naming the session and changes
        nothing, the decoder's state included.  The samples reach the device at the next step()."""
        s = self._get(sid)
        self._check_route([s], pcm=False, mp3=True)
        if s.pending:
            raise ValueError(f"session {s.sid}: already pushed in this step")
        s.mp3.mark()
        chunk = s.mp3.push(data, finished)        # Mp3Error: the object is as it was
        try:
            rate = chunk.info["sample_rate"]
            if rate and rate != s.sr:
                raise ValueError(f"session {s.sid}: the MP3 stream is at {rate} Hz, the session was opened with sample_rate {s.sr}")
            self._admit([(s, chunk.released)])
        except ValueError:
            s.mp3.rollback()
            raise
        s.mp3_chunk = chunk
        s.states.source_finished = bool(finished)
        s.pending = True

    def _mp3_stage(self, sessions):
        """The records of a step's MP3-fed sessions: copied into the arena, ONE upload, ONE ss_mp3_stream_synthesize into the sessions'
        device histories (behind the samples a gapless stream still holds back), the released ones committed.
        -> (bytes uploaded, granule-channels decoded).  Single-buffered like _pcm_stage."""
        if self._mp3_arena is None:
            self._mp3_arena = PcmArena(self.model.device)
        self._mp3_arena.clear()
        items = []
        for s in sessions:
            ch = s.mp3_chunk
            if ch.granules:
                if s.mp3_state is None:
                    from .mp3 import stream_state
                    s.mp3_state = stream_state(ch.channels, self.model.device)
                dst, at = s.fe.pcm_reserve(ch.written, keep=s.mp3_held)
                items.append((ch, s.mp3_state, dst, at + s.mp3_held, 0))
        n_rec, n_bytes = self.model.mp3_stream_decode(self._mp3_arena, items) if items else (0, 0)
        for s in sessions:
            ch = s.mp3_chunk
            s.mp3_held += ch.written - ch.released
            s.fe.pcm_commit(ch.released)
            s.mp3_chunk = None
        return n_bytes, n_rec

    def _pcm_stage(self, sessions):
        """The chunks of a step's PCM-fed sessions: copied into the arena, ONE upload, ONE ss_pcm_scatter into the sessions' device
        histories.  -> bytes moved.  The arena is single-buffered: the step's CTC read (or, in a step that encodes nothing, the
        upload's event at the next clear()) orders the copy before the buffer is written again."""
        if self._arena is None:
            self._arena = PcmArena(self.model.device)
        self._arena.clear()
        segs, dsts = [], []
        for s in sessions:
            mv, frames = s.pcm_chunk
            off = self._arena.add(mv)
            held = 0
            if s.ep is not None:                  # an endpointed session writes behind what it has not committed yet
                held = s.ep.held
                self._ep_room(s, frames)
            dst, at = s.fe.pcm_reserve(frames, keep=held)
            segs.append((off, at + held, frames, s.pcm_in.code, s.pcm_in.channels, len(dsts)))
            dsts.append(dst)
        stage, n = self._arena.upload()
        if n:                                     # nothing but empty chunks (a bare finished=True): no copy, no launch
            self.model.pcm_scatter(stage, n, segs, dsts)
        for s in sessions:
            if s.ep is not None:                  # what it commits is decided after the scan (_endpoint_stage)
                s.ep.held += s.pcm_chunk[1]
            else:
                s.fe.pcm_commit(s.pcm_chunk[1])
            s.pcm_chunk = None
        return n

    # ---- endpointed sessions (endpoint.py) ---------------------------------------------------------------------------------------
    def _fit_samples(self, sr: int, shift_ms, window_ms) -> int:
        """The longest utterance, in samples at `sr`, whose encoder rows fit max_rows (the bound _admit holds plain sessions to)."""
        fits = lambda n: _encoder_out_len(max(fbank_frames_after(sr, n, shift_ms, window_ms), 0)) <= self.max_rows   # noqa: E731
        lo, hi = 0, 1
        while fits(hi) and hi < 1 << 40:
            lo, hi = hi, 2 * hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if fits(mid) else (lo, mid)
        return lo

    def _ep_total(self, s) -> int:
        """Stream samples an endpointed session has received, the chunk pushed for the next step included."""
        return s.ep.base + s.fe.n_pcm + s.ep.held + (s.pcm_chunk[1] if s.pcm_chunk is not None else 0)

    def backlog(self, sid: int) -> int:
        """Samples of an endpointed session's stream from its first unscanned frame on (less than a window and a shift when every
        step keeps up; more while a scan stopped at a cut, or while the session waits for a slot)."""
        s = self._get(sid)
        if s.ep is None:
            raise ValueError(f"session {sid} was not opened with endpoint")
        return max(0, self._ep_total(s) - max(s.ep.next_frame * s.ep.p.H, s.ep.base))

    def utterances(self, sid: int) -> list:
        """The utterances an endpointed session has ended since open() / reset(): [{"start", "end", "kind"}] in stream samples, kind
        "silence", "forced" or "stream_end"."""
        s = self._get(sid)
        if s.ep is None:
            raise ValueError(f"session {sid} was not opened with endpoint")
        return [dict(u) for u in s.ep.utterances]

    def _push_endpoint(self, s, mv, frames, finished):
        """push_pcm of an endpointed session.  The only size refusal: backlog plus chunk past the longest utterance."""
        e = s.ep
        if s.pcm_chunk is not None:
            raise ValueError(f"session {s.sid}: already pushed in this step")
        if e.stream_finished:
            raise ValueError(f"session {s.sid}: its stream has ended (finished=True); reset({s.sid}) starts a new one")
        if self.backlog(s.sid) + frames > e.p.max_utterance_samples:
            raise ValueError(f"session {s.sid}: {self.backlog(s.sid)} unscanned samples and {frames} more would pass the longest "
                             f"utterance ({e.p.max_utterance_samples} samples): step() the pool first")
        s.pcm_chunk = (mv, frames)
        e.stream_finished = bool(finished)
        s.pending = True

    def _ep_room(self, s, frames: int):
        """An endpointed session's history is a view into a buffer of its own with room for one window IN FRONT of it: frames are
        counted from the stream's beginning, so the first unscanned frame may begin up to W - H samples before a cut, where the
        next utterance's history (index 0 of fe._dev, as the fbank reads it) begins.  Grown here, by doubling, so that
        fe.pcm_reserve never reallocates it; seated again after the agent's reset() dropped the view."""
        e, c = s.ep, s.ep.p.W
        have = s.fe.n_pcm + e.held
        if e.buf is None or e.buf.numel() < c + have + frames:
            buf = torch.empty((c + max(2 * (have + frames), 1 << 16),), dtype=torch.float32, device=self.model.device)
            if e.buf is not None and e.lead + have:
                buf[c - e.lead:c + have] = e.buf[c - e.lead:c + have]
            e.buf = buf
        if s.fe._dev is None or s.fe._dev.data_ptr() != e.buf.data_ptr() + 4 * c:
            s.fe._dev = e.buf[c:]

    def _ep_drop(self, s, d: int, m: int):
        """Move an endpointed session's history so that its sample d becomes sample 0, with the m samples from there on and up to a
        window of what lies before: a device copy, no host copy."""
        e, c = s.ep, s.ep.p.W
        if d <= 0:
            return
        lead = min(c, e.lead + d)
        e.buf[c - lead:c + m] = e.buf[c + d - lead:c + d + m].clone()
        e.lead, e.base = lead, e.base + d

    def _endpoint_stage(self, eps, spare: int, out: dict) -> dict:
        """After the scatter: ONE ss_vad_scan over the unscanned frames of every endpointed session of the step, ONE download of the
        result records into pinned memory and one synchronisation; then, per session, what it commits.  Sessions outside an
        utterance are answered here (EmptySegment) and take no further part in the step."""
        jobs, segs = [], []
        for s in eps:
            e = s.ep
            if e.done or e.deferred is not None:
                continue
            total = self._ep_total(s)
            n = e.p.frames_present(total) - e.next_frame
            jobs.append((s, total, n))
            if n > 0:
                segs.append(e.p.seg(s.fe._dev.data_ptr() - 4 * e.lead, e.dev_state.data_ptr(), 0, e.base - e.lead,
                                    e.lead + s.fe.n_pcm + e.held, e.next_frame, n))
        results = []
        if segs:
            need = EP.RESULT_BYTES * len(segs)
            dev = torch.device(self.model.device)
            if self._vad_dev is None or self._vad_dev.numel() < need:
                self._vad_dev = torch.empty((2 * need,), dtype=torch.uint8, device=dev)
                self._vad_host = torch.empty((2 * need,), dtype=torch.uint8, pin_memory=dev.type == "cuda")
            self.model.vad_scan(segs, self._vad_dev[:need])
            self._vad_host[:need].copy_(self._vad_dev[:need], non_blocking=True)
            if dev.type == "cuda":
                torch.cuda.current_stream().synchronize()    # the records below are read from the pinned buffer
            results = EP.read_results(self._vad_host.numpy(), len(segs))
        stats = {"vad_scan_calls": 1 if segs else 0, "vad_frames": sum(n for _, _, n in jobs if n > 0), "endpoint_starts": 0,
                 "endpoint_ends": 0, "endpoint_commits": {}}
        it = iter(results)
        todo = [(s, s.ep.deferred[0], s.ep.deferred[1]) for s in eps if s.ep.deferred is not None]
        for s, total, n in jobs:
            e = s.ep
            r = next(it) if n > 0 else _no_event_result(e.next_frame, e.last_speech, e.mode)
            todo.append((s, r, total))
        for s, r, total in todo:
            spare = self._endpoint_apply(s, r, total, spare, out, stats)
        return stats

    def _endpoint_apply(self, s, r, total: int, spare: int, out: dict, stats: dict) -> int:
        """One session's result record -> its history, its commit of this step and its answer if it is outside an utterance.
        `total`: the stream samples it held when the record was made.  -> the spare slots left."""
        e, p = s.ep, s.ep.p
        if (e.in_utt or r.events & EP.START) and s.slot is None:
            if spare <= 0:                        # no slot for a new speaker: the record waits, the session is not scanned meanwhile
                e.deferred = (r, total)
                out[s.sid] = EmptySegment()
                return spare
            self._acquire(s)
            spare -= 1
        e.deferred = None
        e.next_frame, e.mode, e.last_speech = int(r.consumed), int(r.mode), int(r.last_speech)
        now = self._ep_total(s)
        at_end = e.stream_finished and e.next_frame >= p.frames_present(now)
        if not e.in_utt:
            if not r.events & EP.START:
                # idle: nothing is committed; keep the pre-roll, a possible onset run and one window behind the next frame
                keep_from = max(e.prev_cut, e.next_frame * p.H - p.idle_keep + p.W, e.base)
                if keep_from - e.base >= max(p.idle_keep, p.H * (1000 // 10)):
                    e.held -= keep_from - e.base
                    self._ep_drop(s, keep_from - e.base, e.held)
                e.done = at_end
                out[s.sid] = EmptySegment(finished=at_end)
                return spare
            a = max(e.prev_cut, int(r.start_frame) * p.H - p.pre_roll_samples, e.base)
            e.held -= a - e.base
            self._ep_drop(s, a - e.base, e.held)
            e.in_utt, e.utt_start = True, a
            stats["endpoint_starts"] += 1
        committed = e.base + s.fe.n_pcm
        fin, kind = False, None
        if r.events & (EP.END | EP.FORCED):
            b, fin, kind = int(r.cut_sample), True, "silence" if r.events & EP.END else "forced"
        elif at_end:
            b, fin, kind, e.done = now, True, "stream_end", True
        else:                                     # never past a cut a later scan may still find
            b = max(committed, min(total, (e.last_speech + 1 + p.post_roll) * p.H + p.W - p.H))
        n = b - committed
        s.fe.pcm_commit(n)
        e.held -= n
        s.states.source_finished = fin
        stats["endpoint_commits"][s.sid] = (committed, n, fin)
        if fin:
            stats["endpoint_ends"] += 1
            e.utterances.append({"start": e.utt_start, "end": b, "kind": kind})
            e.prev_cut = e.utt_start = b
            e.in_utt = bool(r.events & EP.FORCED)
            e.final = True
        return spare

    def _endpoint_finish(self, eps):
        """The end of a step: a session whose utterance ended is reset as reset(sid) resets it -- agent state, slot, pcm_state -- with
        the samples behind the cut as the beginning of what comes next; the noise floor and the frame numbering carry on.  A session
        with unscanned frames (the scan stopped at the cut), a waiting record or a stream end to report stays pending."""
        for s in eps:
            e = s.ep
            if e.final:
                e.final = False
                s.reset()                         # drops fe's view of the history, not the buffer: the samples behind the cut (and the
                self._release(s)                  # window before it the next frame may reach into) move to its beginning
                self._ep_drop(s, e.prev_cut - e.base, e.held)
                self._ep_room(s, 0)
            s.pending = (not e.done) and (e.deferred is not None or e.stream_finished
                                          or e.p.frames_present(self._ep_total(s)) > e.next_frame)

    def step(self, segments: Optional[dict] = None) -> dict:
        """{sid: SpeechSegment} -> {sid: Segment}: per session exactly one agent.pushpop(segment), for these sessions and any pushed
        since the last step.  The pushes of `segments` are admitted together: if one is refused, ValueError names it and the WHOLE
        call is refused before anything moves (to step the others anyway, push() them one by one and call step())."""
        if segments:
            items = [(self._get(sid), seg) for sid, seg in segments.items()]
            self._check_route([s for s, _ in items], pcm=False)
            self._admit(items)
            for s, seg in items:
                s.states.update_source(seg)
                s.pending = True
        todo = [s for s in self.sessions.values() if s.pending]
        out: Dict[int, object] = {}
        actions: Dict[int, tuple] = {}
        t0 = time.perf_counter()
        # ---- front-end: finished agents answer at once; the new rows of every other session in one launch ----
        feats, batch, fe_calls, fe_rows = {}, [], 0, 0
        eps = [s for s in todo if s.ep is not None]
        # slots the step's other sessions were promised by _admit: a START may take what is left
        spare = len(self.free) - sum(1 for s in todo if s.ep is None and s.slot is None and not s.states.target_finished
                                     and self._frames(s) > 0) if eps else 0
        fed = [s for s in todo if s.pcm_chunk is not None and not s.states.target_finished]
        pcm_bytes = self._pcm_stage(fed) if fed else 0
        vad = self._endpoint_stage(eps, spare, out) if eps else None
        fed3 = [s for s in todo if s.mp3_chunk is not None and not s.states.target_finished]
        mp3_bytes_in = sum(s.mp3_chunk.n_bytes for s in fed3)
        mp3_bytes, mp3_recs = self._mp3_stage(fed3) if fed3 else (0, 0)
        for s in todo:
            s.pending = False
            if s.sid in out:                      # an endpointed session outside an utterance: answered by _endpoint_stage
                continue
            if s.states.target_finished:
                s.pcm_chunk = None                # a finished agent's audio is not kept (the list route appends and never reads it)
                s.mp3_chunk = None
                out[s.sid] = EmptySegment(finished=True)
                continue
            st = s.fe.stage_pcm() if (s.pcm_in is not None or s.mp3_in is not None) else s.fe.stage(s.states.source)
            if st is None:
                actions[s.sid] = ("write", "", True) if s.states.source_finished else ("read",)
                continue
            nf, eff = st
            final = nf                            # 16 kHz: every row is final
            if s.sr != SAMPLE_RATE:
                plan = s.fe.sr_rows(eff, s.sr)    # rows after resampling and how many are final, as the library counts them
                if plan is None:                  # a ratio the batched call refuses (taps too large): this session resamples its history
                    fb = self.model.fbank_cmvn(self.model.resample(s.fe._dev[:eff], s.sr, SAMPLE_RATE), 32768.0)
                    fe_calls, fe_rows = fe_calls + 2, fe_rows + fb.shape[0]
                    nf = fb.shape[0]
                    if nf:
                        feats[s.sid] = fb
                else:
                    nf, final = plan
                if nf == 0:                       # too short after resampling: the agent's early return, as above
                    actions[s.sid] = ("write", "", True) if s.states.source_finished else ("read",)
                if nf == 0 or plan is None:
                    continue
            batch.append((s, s.fe.new_rows(nf), nf, final, eff))
        if batch:
            hist, first = [s.fe._dev for s, _, _, _, _ in batch], [k for _, k, _, _, _ in batch]
            cnt, outs = [nf - k for _, k, nf, _, _ in batch], [s.fe._fb[k:nf] for s, k, nf, _, _ in batch]
            if all(s.sr == SAMPLE_RATE for s, _, _, _, _ in batch):
                self.model.batch_fbank_frames(hist, first, cnt, outs)
            else:                                 # 16-kHz sessions of a mixed step pass through: the same bits
                self.model.batch_fbank_frames_sr(hist, [eff for _, _, _, _, eff in batch], [s.sr for s, _, _, _, _ in batch], first,
                                                 cnt, outs)
            fe_calls, fe_rows = fe_calls + 1, fe_rows + sum(cnt)
            for s, k, nf, final, _ in batch:
                feats[s.sid] = s.fe.commit_rows(nf, final)
        t1 = time.perf_counter()
        # ---- one encoder step + both CTC heads ----
        enc = [s for s in todo if s.sid in feats]
        writers, n_steps, mine, views, mt_groups = [], 0, [], None, []
        beam_asr = []                             # pools with ctc_beam: the step's ASR sessions, by their index in enc
        if enc:
            for s in enc:
                self._acquire(s)
            packed, views, n_fin, _ = self.pool.forward([s.slot for s in enc], [feats[s.sid] for s in enc],
                                                        [s.attn_chunk for s in enc], [s.conv_chunk for s in enc])
            beam_asr = [i for i, s in enumerate(enc) if s.kind == "asr"] if self.ctc_stream is not None else []
            if len(beam_asr) < len(enc):          # (a pool with details: the scored form, records of five)
                src, tgt = self.pool.ctc_both()
            else:                                 # ASR sessions only, all on the prefix search: no arg-max call
                src = tgt = [None] * len(enc)
            parts = self._ctc_stream_step(enc, beam_asr, packed, views, n_fin) if beam_asr else {}
            spot_asr = [i for i, s in enumerate(enc) if s.kind == "asr"] if self.spot_stream is not None else []
            if spot_asr:
                self._spot_step(enc, spot_asr, packed, views, n_fin)
            if self.with_details:
                for i, s in enumerate(enc):
                    self._set_details(s, src[i], tgt[i], n_fin[i])
            if fed:
                self._arena.synchronized()        # the CTC read waited for everything queued before it, the arena's upload included
            if fed3:
                self._mp3_arena.synchronized()
            t2 = time.perf_counter()
            for i, s in enumerate(enc):
                if i in parts:
                    actions[s.sid] = self._asr_beam(s, parts[i])
                    continue
                if s.kind == "asr":
                    actions[s.sid] = self._asr(s, src[i][0])
                    continue
                if s.kind not in KINDS:           # a subclass's kind: its own gate -> an action, or a writer (prefix, max_len, new)
                    w = self._gate(s, src[i][0], tgt[i][0], feats[s.sid].shape[0])
                    if w[0] == "write":
                        writers.append((i, s) + tuple(w[1:]))
                    else:
                        actions[s.sid] = w
                    continue
                g = s2tt_gate(len(src[i][0]), len(tgt[i][0]), s.src_ctc_prefix_length, s.tgt_ctc_prefix_length,
                              len(s.tgt_subwords) if s.tgt_subwords is not None else 0, s.lagging_k1, s.stride_n,
                              s.states.source_finished)
                s.src_ctc_prefix_length, s.tgt_ctc_prefix_length = g.src_prefix_len, g.tgt_prefix_len
                if not g.write:
                    actions[s.sid] = ("read",)
                    continue
                prefix = list(s.tgt_subwords) if s.tgt_subwords is not None else []
                ml = mt_max_len(len(prefix), feats[s.sid].shape[0], g.new_tokens, MAX_LEN_A, MAX_LEN_B,
                                self.model.cfg.max_target_positions, MIN_LEN)
                writers.append((i, s, prefix, ml, g.new_tokens))
            # ---- one ragged continuation of every writer's prefix ----
            if writers:
                if len(writers) == len(enc):
                    enc_w, Tp = packed, [views[i].shape[0] for i in range(len(enc))]
                else:
                    enc_w = torch.cat([views[i] for i, _, _, _, _ in writers], 0)
                    Tp = [views[i].shape[0] for i, _, _, _, _ in writers]
                keys = None
                if self.sampling is not None:
                    keys = [sampling_stream_key(s.sid, s.mt_writes) for _, s, _, _, _ in writers]
                    for _, s, _, _, _ in writers:
                        s.mt_writes += 1
                res, mt_groups = self._mt_call(enc_w, Tp, [p for _, _, p, _, _ in writers], [m for _, _, _, m, _ in writers], keys)
                for w, (toks, fts) in zip(writers, res):
                    i, s, prefix, ml, new = w
                    n_steps = max(n_steps, len(toks) - 1)
                    if s.kind in KINDS:
                        actions[s.sid] = self._s2tt_write(s, prefix + toks, new, i)
                    else:
                        mine.append((w, toks, fts))
        else:
            t2 = t1
        t3 = time.perf_counter()
        if mine:                                  # a subclass's write side after the shared MT call (its own timings)
            self._write_side(mine, views, actions)
        n_align = self._align_flush(views) if self.with_align else 0     # after every other device call of the step
        # ---- actions -> segments, as GenericAgent.pop ----
        for s in todo:
            if s.sid in out:
                continue
            a = actions[s.sid]
            if a[0] == "read":
                out[s.sid] = EmptySegment()
                continue
            if s.kind not in KINDS:               # a subclass's kind makes its own segment
                out[s.sid] = self._segment(s, a)
                continue
            seg = TextSegment(index=0, content=a[1], finished=a[2])
            s.states.update_target(seg)
            out[s.sid] = seg
            if s.states.target_finished:          # finished without the agent's reset(): it answers EmptySegment(finished=True)
                self._release(s)                  # from now on, so its slot goes back; reset(sid) starts a fresh utterance
        self.last_step = {"sessions": len(todo), "encoded": len(enc), "writers": len(writers), "mt_steps": n_steps, "mt_groups": mt_groups,
                          "ctc_scored": 1 if (enc and self.with_details) else 0,       # the step's CTC call was the scored form
                          "mt_attention": n_align,                                      # batch_mt_attention calls of the step (pools with align)
                          "frontend_calls": fe_calls, "fbank_rows": fe_rows,       # front-end device calls of the step, rows they computed
                          # the PCM route: uploads and ss_pcm_scatter launches of the step (0 or 1 each), bytes uploaded; a subclass's
                          # write side sets the pack side (ss_pcm_pack_s16 launches, bytes downloaded)
                          "pcm_uploads": 1 if pcm_bytes else 0, "pcm_scatter_calls": 1 if pcm_bytes else 0, "pcm_bytes_in": pcm_bytes,
                          "pcm_pack_calls": 0, "pcm_bytes_out": 0,
                          # sessions that answer at their own rate and format (PcmOut): ss_pcm_emit calls of the step (0 or 1), bytes
                          "pcm_emit_calls": 0, "pcm_emit_bytes_out": 0,
                          # the MP3 route: uploads and ss_mp3_stream_synthesize calls of the step (0 or 1 each), MP3 bytes the step's
                          # pushes brought, granule-channels decoded
                          "mp3_uploads": 1 if mp3_bytes else 0, "mp3_synth_calls": 1 if mp3_recs else 0, "mp3_bytes_in": mp3_bytes_in,
                          "mp3_granules": mp3_recs,
                          "frontend_s": t1 - t0, "encoder_ctc_s": t2 - t1, "mt_s": t3 - t2, "total_s": time.perf_counter() - t0}
        # the endpoint scan: ss_vad_scan launches of the step (0 or 1), frames handed to it, utterances begun and ended, and per
        # session inside an utterance (first stream sample, samples, finished) of what the step committed
        self.last_step.update({"vad_scan_calls": 0, "vad_frames": 0, "endpoint_starts": 0, "endpoint_ends": 0, "endpoint_commits": {}}
                              if vad is None else vad)
        if self.ctc_stream is not None:           # ss_ctc_stream_advance calls of the step (0 or 1), rows they ran through the head
            self.last_step.update({"ctc_stream_calls": 1 if (enc and beam_asr) else 0,
                                   "ctc_stream_rows": sum(self._stream_rows) if (enc and beam_asr) else 0})
        if self.spot_stream is not None:          # ss_ctc_spot_stream_advance calls of the step (0 or 1), rows through the head, hits lost
            ran = bool(enc) and any(s.kind == "asr" for s in enc)
            self.last_step.update({"ctc_spot_calls": 1 if ran else 0, "ctc_spot_rows": sum(self._spot_rows) if ran else 0,
                                   "ctc_spot_lost": self._spot_lost if ran else 0})
        self.last_step.update(self._side_times)
        self._side_times = {}
        if eps:
            self._endpoint_finish(eps)
        return out

    def _mt_call(self, enc_w, Tp, prefixes, max_len, keys=None):
        """The step's ONE ragged continuation of every writer's committed prefix -> (per writer (tokens after the prefix incl. the
        final eos, decoder states of the fed positions), the [start, end) writer ranges of the device calls it took).  beam_mt = 1:
        the greedy continuation, as always.  beam_mt > 1: the beam search behind the prefix, hypothesis 0 of each writer; writers x
        beam_mt hypothesis rows are at most 256 per device call, so a step with more writers runs as the consecutive sub-calls of
        plan_beam_groups inside the engine call (nobody is refused).  A search option set: the same beam call at beam_mt = 1 too."""
        search = self.search.kwargs()
        if self.sampling is not None:          # keys: one stream key per writer
            nbest, feats = self.model.batch_mt_sample_continue(enc_w, Tp, prefixes, max_len, self.beam_mt, keys, min_len=MIN_LEN,
                                                               **self.sampling.kwargs(), **search)
            return [(h[0]["tokens"][len(p):], f) for h, f, p in zip(nbest, feats, prefixes)], plan_beam_groups(len(Tp), self.beam_mt)
        if self.beam_mt == 1 and not search:
            return self.model.batch_mt_continue(enc_w, Tp, prefixes, max_len, MIN_LEN), [(0, len(Tp))]
        nbest, feats = self.model.batch_mt_beam_continue(enc_w, Tp, prefixes, max_len, self.beam_mt, MIN_LEN, **search)
        return [(h[0]["tokens"][len(p):], f) for h, f, p in zip(nbest, feats, prefixes)], plan_beam_groups(len(Tp), self.beam_mt)

    # ---- hooks of a subclass's session kinds (speech_pool.py) -------------------------------------------------------------------
    def _gate(self, s, src_ids, tgt_ids, n_frames):
        """-> ("write", prefix, max_len, new_tokens) to join the step's MT call, or the session's action."""
        raise NotImplementedError(s.kind)

    def _write_side(self, mine, views, actions):
        """After the MT call: [((i, s, prefix, max_len, new), tokens, decoder states)] of this kind's writers -> actions[sid]."""
        raise NotImplementedError

    def _segment(self, s, a):
        raise NotImplementedError(s.kind)

    # ---- the agents' write paths ------------------------------------------------------------------------------------------------
    def _finish(self, s: _Session):
        s.states.target_finished = True
        s.reset()                                 # the agent's reset(): a fresh utterance, its slot back to the pool
        self._release(s)

    def _asr(self, s: _Session, tokens):
        words = [s.dict["source_unigram"][c] for c in tokens]
        text = " ".join(words)
        new_text = text[len(s.asr_text):]
        s.asr_text = text
        if s.states.source_finished:
            self._finish(s)
        return ("write", new_text, s.states.target_finished)

    def _ctc_stream_step(self, enc, beam_asr, packed, views, n_fin) -> dict:
        """The step's ONE advance of the prefix searches of its ASR sessions -> {index in enc: engine.CtcPartial}."""
        T2 = [int(views[i].shape[0]) for i in beam_asr]
        rows = packed if len(beam_asr) == len(enc) else torch.cat([views[i] for i in beam_asr], 0)
        final = [bool(enc[i].states.source_finished) for i in beam_asr]
        upto = [t2 if fin else int(n_fin[i]) for i, t2, fin in zip(beam_asr, T2, final)]
        got = self.ctc_stream.advance([enc[i].slot for i in beam_asr], rows, T2, upto, final)
        self._stream_rows = [p.frames - enc[i].ctc_frames for i, p in zip(beam_asr, got)]
        for i, p in zip(beam_asr, got):
            enc[i].ctc_frames = 0 if p.final else p.frames
        return dict(zip(beam_asr, got))

    def _spot_step(self, enc, spot_asr, packed, views, n_fin):
        """The step's ONE advance of the spotters of its ASR sessions, over the rows _ctc_stream_step takes; what they emit joins
        the sessions' spot_hits on the session clock."""
        from .keywords import KeywordHit
        from .words import FRAME_MS
        T2 = [int(views[i].shape[0]) for i in spot_asr]
        rows = packed if len(spot_asr) == len(enc) else torch.cat([views[i] for i in spot_asr], 0)
        final = [bool(enc[i].states.source_finished) for i in spot_asr]
        upto = [t2 if fin else int(n_fin[i]) for i, t2, fin in zip(spot_asr, T2, final)]
        got = self.spot_stream.advance([enc[i].slot for i in spot_asr], rows, T2, upto, final, self.spot_max_hits)
        self._spot_rows = [p.frames - enc[i].spot_frames for i, p in zip(spot_asr, got)]
        self._spot_lost = sum(p.n_hits - len(p.hits) for p in got)
        texts = self.spot_stream.keywords.texts
        for i, p in zip(spot_asr, got):
            s = enc[i]
            s.spot_frames = 0 if p.final else p.frames
            t0 = self._t0_ms(s)
            s.spot_hits.extend(KeywordHit(h.keyword, texts[h.keyword], t0 + h.start * FRAME_MS, t0 + (h.end + 1) * FRAME_MS, h.score, h.norm)
                               for h in p.hits)

    def _asr_beam(self, s: _Session, part):
        symbols = [s.dict["source_unigram"][c] for c in part.hyps[0].tokens] if part.hyps else []
        s.partial = symbols
        new_text, s.asr_text = asr_beam_emit(s.asr_text, symbols, part.n_stable, part.final)
        if part.final:
            s.nbest = part.hyps
            self._finish(s)
        return ("write", new_text, s.states.target_finished)

    def _s2tt_write(self, s: _Session, toks, new_tokens, view=None):
        sub = toks[:-1] if toks[-1] == 2 else toks
        words = [s.dict["target_unigram"][c] for c in sub]
        if s.tgt_subwords is not None and list(s.tgt_subwords) == list(sub):
            return ("write", "", True) if s.states.source_finished else ("read",)
        s.tgt_subwords = list(sub)
        self._align_note(s, sub, view)
        text = " ".join(words)
        new_text = text[len(s.tgt_text):]
        s.tgt_text = text
        if s.states.source_finished and new_tokens == -1:
            self._finish(s)
        return ("write", new_text, s.states.target_finished)
