"""StreamSpeechS2STAgent -- drop-in for the reference SimulEval agent
(agent/speech_to_speech.streamspeech.agent.py:101-770) with the model math on MI355X.

Same class name, ``@entrypoint``, ``add_args`` flags, ``reset`` / ``policy`` contract
(``ReadAction`` | ``WriteAction(SpeechSegment(content=list[float], sample_rate=16000, finished))``)
and the same read/write gating; every tensor op of the reference policy is replaced by a C-ABI
stage (fbank -> encoder -> CTC x2 -> MT greedy -> T2U + unit decoder -> vocoder).  Like the
reference it recomputes the whole utterance-so-far on every call (incremental state
is the next step, not parity-affecting).
"""
import argparse
import json
import os
from pathlib import Path

import numpy as np
import torch
import yaml

from .frontend import FEATURE_DIM, ORG_SAMPLE_RATE, SAMPLE_RATE, SHIFT_SIZE, WINDOW_SIZE, OnlineFeatureExtractor
from .generators import CTCDecoder, CTCSequenceGenerator, SequenceGenerator
from .modules import CodeHiFiGANVocoderWithDur, Dictionary, StreamSpeechModel, load_model_state
from .simuleval_shim import ReadAction, SpeechSegment, SpeechToSpeechAgent, WriteAction, entrypoint

DEFAULT_EOS = 2


def _detok(symbols):
    text = "".join(symbols)
    for a, b in (("_", " "), ("▁", " "), ("<unk>", " "), ("<s>", ""), ("</s>", "")):
        text = text.replace(a, b)
    return text[1:] if len(text) > 0 and text[0] == " " else text


def word_details(agent, src_hyp, tgt_hyp):
    """--word-details: the words of both CTC heads from the scored hypotheses of this policy() call.  `stable` needs the rows that
    are final, which only the incremental encoder counts (engine.stream_stats): None under --full-recompute-encoder."""
    from .words import details_from_hyps
    eng = agent.model.hip if hasattr(agent.model, "hip") else agent.model
    n_final = None
    if getattr(agent.model.encoder, "incremental", False) and getattr(eng, "stream_stats", None) is not None:
        n_final = int(eng.stream_stats[0])
    return details_from_hyps(src_hyp, tgt_hyp, agent.dict["source_unigram"], agent.dict["ctc_target_unigram"], n_final=n_final,
                             finished=bool(agent.states.source_finished))


def speaker_id_arg(args, vocoder, flag="--speaker-id"):
    """The voice of an agent or session: args.speaker_id on a multi-speaker vocoder (required there, inside its speakers), None on
    a single-speaker one, which ignores the flag."""
    n = int(getattr(getattr(vocoder, "hip", vocoder), "num_speakers", 0) or 0)
    if not n:
        return None
    spk = getattr(args, "speaker_id", None)
    if spk is None:
        raise ValueError(f"the vocoder is multi-speaker ({n} speakers): {flag} is required")
    if not 0 <= int(spk) < n:
        raise ValueError(f"{flag} {spk} is outside the vocoder's {n} speakers")
    return int(spk)


def synthesize_tail(vocoder, unit, n_new, dur_prediction, ctx=0, rf=None, spkr=None, info=None):
    """Speech of the last ``n_new`` units of ``unit`` (agent :743-753: vocoder over all units, keep
    ``wav[-dur[-n_new:].sum()*320:]``).  With ``ctx`` > 0 only the last ``n_new + ctx`` units are
    synthesised: identical tail, because the frames further left than the
    generator's receptive field ``rf`` cannot reach it.  ``spkr``: the speaker id a multi-speaker vocoder synthesises with, passed
    as ``x["spkr"]`` on both calls.  Returns (tail, wav of what was synthesised).  ``info``: a dict that receives ``first`` (the
    first unit synthesised) and ``dur`` (the durations [1, K - first] of the synthesised units) of the call whose tail is kept."""
    wav = dur = None
    first = 0
    extra = {} if spkr is None else {"spkr": torch.tensor([[int(spkr)]], dtype=torch.long)}
    if ctx > 0 and len(unit) > n_new + ctx:
        x = {"code": torch.tensor(unit[-(n_new + ctx):], dtype=torch.long).view(1, -1), **extra}
        wav, dur = vocoder(x, dur_prediction)
        # frames left of the new units whose durations are exact (the 2 left-most context units see a
        # truncated duration-predictor window) must cover the generator's receptive field
        first = len(unit) - (n_new + ctx)
        if int(dur[:, 2:ctx].sum()) < rf + 2:
            wav = None
    if wav is None:
        first = 0
        x = {"code": torch.tensor(unit, dtype=torch.long).view(1, -1), **extra}
        wav, dur = vocoder(x, dur_prediction)
    if info is not None:
        info["first"], info["dur"] = first, dur
    return wav[-int(dur[:, -n_new:].sum()) * 320:], wav


def load_dictionaries(args, cfg):
    """The agents' dictionaries (agent :400-420): target units + the three multitask text dictionaries named by
    --multitask-config-yaml (placeholders of the model's sizes where none is given)."""
    d = {"tgt": Dictionary.units(1000)}
    mt_cfg = {}
    if args.multitask_config_yaml is not None:
        mpath = os.path.join(args.data_bin, args.multitask_config_yaml)
        if os.path.exists(mpath):
            with open(mpath) as f:
                mt_cfg = yaml.load(f, Loader=yaml.BaseLoader) or {}
    for name, n in (("target_unigram", cfg.tgt_vocab), ("source_unigram", cfg.src_vocab),
                    ("ctc_target_unigram", cfg.tgt_vocab)):
        path = (mt_cfg.get(name) or {}).get("dict")
        if path and not os.path.exists(path):
            path = os.path.join(args.data_bin, *Path(path).parts[-2:])
        d[name] = Dictionary.load(path) if path and os.path.exists(path) else Dictionary.placeholder(n)
    return d


def _beam_mt_arg(v):
    k = int(v)
    if not 1 <= k <= 32:
        raise argparse.ArgumentTypeError("--beam-mt must be in [1, 32]")
    return k


def _search_kwargs(args) -> dict:
    """--lenpen / --temperature / --no-repeat-ngram-size as generators.SequenceGenerator takes them; nothing at their defaults."""
    p, t, n = float(getattr(args, "lenpen", 1.0)), float(getattr(args, "temperature", 1.0)), int(getattr(args, "no_repeat_ngram_size", 0))
    if (p, t, n) == (1.0, 1.0, 0):
        return {}
    return {"len_penalty": p, "temperature": t, "no_repeat_ngram_size": n}


def _sampling_kwargs(args) -> dict:
    """--sampling / --sampling-topk / --sampling-topp / --seed as generators.SequenceGenerator takes them; nothing without --sampling."""
    if not getattr(args, "sampling", False):
        return {}
    return {"sampling": True, "sampling_topk": int(getattr(args, "sampling_topk", -1)),
            "sampling_topp": float(getattr(args, "sampling_topp", -1.0)), "seed": int(getattr(args, "seed", 1))}


def _greedy_mt(args) -> bool:
    """The reference agent's own search: beam 1, no search option set, no sampling.  Only then the persistent MT step is armed."""
    return int(getattr(args, "beam_mt", 1)) == 1 and not _search_kwargs(args) and not _sampling_kwargs(args)


def sampling_key_kwargs(agent) -> dict:
    """With --sampling: the stream key of this write of the agent's generator_mt -- its --sampling-session and the count of its
    writes since reset() -- as generate_decoder's keyword; nothing otherwise."""
    if getattr(agent.generator_mt, "sampling", None) is None:
        return {}
    from .engine import sampling_stream_key
    n = getattr(agent, "_mt_writes", 0)
    agent._mt_writes = n + 1
    return {"sampling_key": sampling_stream_key(int(getattr(agent.args, "sampling_session", 0)), n)}


def _beam_kwargs(args) -> dict:
    """generator_mt's search options beyond the reference agent's: nothing at the default beam 1 with no search option set (the
    agent builds what it always built)."""
    kw = _search_kwargs(args)
    if int(getattr(args, "beam_mt", 1)) > 1:
        kw["unk_penalty"] = float(getattr(args, "unkpen", 0.0))
    kw.update(_sampling_kwargs(args))
    return kw



def mt_alignment_update(agent, enc, tokens, t0_ms=0):
    """--mt-alignment: `tokens` are all committed target tokens (no </s>) after a write of policy(), `enc` the encoder rows that write
    saw.  The words of the tokens this write added are placed in source time by ONE batch_mt_attention pass that answers only their
    positions (first = the tokens placed before), over `enc` -- what the decoder attended to when it produced them, and what the
    reference records -- and are then frozen: a later write adds words, it never changes one.  agent.alignment = all of them.
    The pass rewrites the scratch set's MT cross-attention K/V and workspace, so the callers issue it where the search has returned
    and no single-utterance MT state is needed any more.  (Should a whole-word cut ever shorten the committed tokens, the words that
    reached past the cut are dropped and placed again.)"""
    from .words import words_from_attention
    tokens = [int(t) for t in tokens]
    rec = agent._mt_align
    while rec and rec[-1][0] > len(tokens):
        rec.pop()
    done = rec[-1][0] if rec else 0
    if len(tokens) > done:
        enc = (enc[:, 0] if enc.dim() == 3 else enc).contiguous()
        _, peak, prob, _, _ = agent.engine.batch_mt_attention(enc, [int(enc.shape[0])], [tokens[:-1]], first=[done], want_matrix=False)[0]
        words = words_from_attention(tokens[done:], peak.tolist(), prob.tolist(), agent.generator_mt.tgt_dict, t0_ms=t0_ms,
                                     eos=agent.generator_mt.eos)
        rec.append((len(tokens), words))
    agent.alignment = [w for _, ws in rec for w in ws]


def spoken_update(agent, raw, n_states, n_units, n_new, first, dur, tokens, carried, emitted):
    """--spoken-words: one write of policy() adds its segments.  `raw` = the device arg-max ids of the write's unit pass over its
    n_states decoder states, n_units all units so far of which the last n_new are new, `first` / `dur` the first unit the tail call
    synthesised and the durations from there on, `tokens` all committed target tokens (no </s>), `carried` the samples of an
    unfinished_wav prepended to this write (emitted here, no state's), `emitted` the samples the write returns.  ONE
    batch_unit_spans call; the clock at the write's start is the samples emitted before it, divided by 16.  agent.spoken then
    answers the words of all committed tokens in the emitted speech (words.Spoken), formed when it is asked."""
    from .words import segments_from_spans
    rec = agent._spoken_rec
    if rec is None:                       # the utterance's first write: the previous utterance's words go now
        rec = agent._spoken_rec = {"segments": [], "samples": 0, "seen": 0}
    clock = rec["samples"] // 16
    if carried:
        rec["segments"].append((-1, clock, clock + int(carried) // 16, 0))
        clock += int(carried) // 16
    spans = agent.engine.batch_unit_spans(raw, [int(n_states)], [int(n_units)], [dur], [int(first)], [int(n_units) - int(n_new)])[0]
    rec["segments"].extend(segments_from_spans(spans, clock, rec["seen"]))
    rec["seen"] = max(rec["seen"], int(n_states))
    rec["samples"] += int(emitted)
    agent._spoken_last = ([int(t) for t in tokens], rec["segments"])
    agent._spoken_words = None


@entrypoint
class StreamSpeechS2STAgent(SpeechToSpeechAgent):
    """Simultaneous speech-to-speech translation agent for StreamSpeech on the HIP backend."""

    def __init__(self, args, model=None, vocoder=None):
        from .text_policy import ctc_beam_flags, ctc_keyword_flags
        ctc_beam_flags(args, "S2ST")                       # (raises: the flags are the ASR agent's)
        ctc_keyword_flags(args, "S2ST")
        super().__init__(args)
        self.eos = DEFAULT_EOS
        self.args = args
        self.gpu = True
        self.device = getattr(args, "device_str", "cuda:0")
        self.load_model_vocab(args, model)
        self.max_len = args.max_len
        self.force_finish = args.force_finish
        torch.set_grad_enabled(False)

        eng = self.model.hip if hasattr(self.model, "hip") else self.model
        self.engine = eng
        beam_mt = int(getattr(args, "beam_mt", 1))
        if hasattr(eng, "set_persistent_mt_step") and _greedy_mt(args):   # HIP engine: the greedy MT decode step as one persistent launch (mt_step.hip)
            eng.set_persistent_mt_step(int(getattr(args, "mt_step_workgroups", 64)))
        tgt_dict_mt = self.dict[self.model.mt_task_name]
        tgt_dict = self.dict["tgt"]
        uni = getattr(self.model, "uni_encoder", False)
        self.ctc_generator = CTCSequenceGenerator(tgt_dict, eng, use_incremental_states=False, t2u_causal=uni)
        self.asr_ctc_generator = CTCDecoder(self.dict["source_unigram"], eng, 0)
        self.st_ctc_generator = CTCDecoder(self.dict["ctc_target_unigram"], eng, 1)
        if hasattr(eng, "set_persistent_mt_step"):
            eng.ctc_speculate = True                     # policy() asks for both CTC heads of every encoder output: one host round trip (engine.ctc_greedy)
        # generator_mt of the reference: beam 1, max_len_a=0, max_len_b=100, min_len=1 (agent :162-180); --beam-mt k searches with a
        # beam behind the committed prefix instead (generators.SequenceGenerator)
        self.generator_mt = SequenceGenerator(eng, tgt_dict_mt, beam_size=beam_mt, max_len_a=0, max_len_b=100, max_len=0,
                                              min_len=1, eos=tgt_dict_mt.eos(), use_incremental_states=False,
                                              **_beam_kwargs(args))
        if vocoder is not None:
            self.vocoder = vocoder
        else:
            vcfg = None
            if args.vocoder_cfg and os.path.exists(args.vocoder_cfg):
                with open(args.vocoder_cfg) as f:
                    vcfg = json.load(f)
            self.vocoder = CodeHiFiGANVocoderWithDur(args.vocoder, vcfg, device=self.device)
            if getattr(args, "vocoder_fp16", False):
                self.vocoder.hip.set_fp16(True)
        self.speaker_id = speaker_id_arg(args, self.vocoder)     # None: a single-speaker vocoder
        self.dur_prediction = args.dur_prediction
        # Incremental synthesis: the reference re-synthesises ALL units at every write
        # and keeps the tail (agent :743-753).  The generator has a finite receptive field, so the same
        # tail comes out of the last (new + context) units only; context = receptive field + the +-2
        # units the duration predictor looks at + slack.  0 restores the full re-synthesis.
        vcfg = getattr(getattr(self.vocoder, "hip", self.vocoder), "cfg", None)
        rf = vcfg.receptive_field_frames() if vcfg is not None and hasattr(vcfg, "receptive_field_frames") else None
        want = getattr(args, "vocoder_context_units", -1)
        self.vocoder_rf = rf
        self.vocoder_ctx = 0 if (rf is None or want == 0) else (want if want > 0 else rf + 8)
        self.lagging_k1, self.lagging_k2 = args.lagging_k1, args.lagging_k2
        self.segment_size = args.segment_size
        self.stride_n, self.stride_n2 = args.stride_n, args.stride_n2
        self.unit_per_subword = args.unit_per_subword
        if args.extra_output_dir is not None:
            self.asr_file = Path(args.extra_output_dir + "/asr.txt")
            self.st_file = Path(args.extra_output_dir + "/st.txt")
            self.unit_file = Path(args.extra_output_dir + "/unit.txt")
            self.quiet = False
        else:
            self.quiet = True
        self.output_asr_translation = args.output_asr_translation
        self.whole_word = args.source_segment_size >= 640
        self.reset()

    @staticmethod
    def add_args(parser):
        a = parser.add_argument
        a("--model-path", type=str, required=True, help="path to your pretrained model (or synthetic:<seed>)")
        a("--data-bin", type=str, required=True, help="Path of data binary")
        a("--config-yaml", type=str, default=None, help="Path to config yaml file")
        a("--multitask-config-yaml", type=str, default=None, help="Path to config yaml file")
        a("--global-stats", type=str, default=None, help="Path to json file containing cmvn stats")
        a("--tgt-splitter-type", type=str, default="SentencePiece", help="Subword splitter type for target text")
        a("--tgt-splitter-path", type=str, default=None, help="Subword splitter model path for target text")
        a("--user-dir", type=str, default="researches/ctc_unity", help="User directory for model")
        a("--agent-dir", type=str, default="agent", help="User directory for agents")
        a("--max-len", type=int, default=200, help="Max length of translation")
        a("--force-finish", default=False, action="store_true", help="Force the model to finish the hypothsis")
        a("--shift-size", type=int, default=SHIFT_SIZE, help="Shift size of feature extraction window.")
        a("--window-size", type=int, default=WINDOW_SIZE, help="Window size of feature extraction window.")
        a("--sample-rate", type=int, default=ORG_SAMPLE_RATE, help="Sample rate")
        a("--feature-dim", type=int, default=FEATURE_DIM, help="Acoustic feature dimension.")
        a("--vocoder", type=str, required=True, help="path to the CodeHiFiGAN vocoder (or synthetic:<seed>)")
        a("--vocoder-cfg", type=str, required=False, default=None, help="path to the CodeHiFiGAN vocoder config")
        a("--dur-prediction", action="store_true", help="enable duration prediction (for reduced/unique code sequences)")
        a("--vocoder-fp16", action="store_true", default=False,
          help="run the vocoder's 64- to 256-channel ResBlock convs on FP16 matrix cores (f32 accumulation; waveform within 1e-3 RMS, "
               "unit ids and durations unchanged); default: exact f32")
        a("--speaker-id", type=int, default=None,
          help="the voice of a multi-speaker vocoder (\"multispkr\": true in --vocoder-cfg): required there, ignored otherwise")
        a("--lagging-k1", type=int, default=0, help="lagging number")
        a("--lagging-k2", type=int, default=0, help="lagging number")
        a("--segment-size", type=int, default=320, help="segment-size")
        a("--stride-n", type=int, default=1, help="lagging number")
        a("--stride-n2", type=int, default=1, help="lagging number")
        a("--unit-per-subword", type=int, default=15, help="lagging number")
        a("--full-recompute-encoder", default=False, action="store_true",
          help="re-encode all received audio at every policy() call like the reference (default: reuse final rows)")
        a("--vocoder-context-units", type=int, default=-1,
          help="left-context units re-synthesised with each new unit tail (-1: receptive field + 8, 0: all units like the reference)")
        a("--mt-step-workgroups", type=int, default=64,
          help="first-pass text decoder: one persistent launch per decode step on this many workgroups (64 | 128 | 256; the agent "
               "decodes one utterance at a time, which is what that form needs); 0: one launch per op")
        a("--beam-mt", type=_beam_mt_arg, default=1,
          help="beam of the first-pass text search behind the committed prefix (1 = greedy, the reference agent; at most 32).  Above 1 "
               "every write is a fresh beam search with the offline generator's prefix_tokens semantics, and the persistent MT step "
               "(--mt-step-workgroups), which belongs to the greedy search, is not armed")
        a("--unkpen", type=float, default=0.0, help="subtracted from the <unk> log-probability of the beam search of --beam-mt > 1; ignored at --beam-mt 1 (the greedy "
               "search of the reference agent has no such penalty)")
        a("--lenpen", type=float, default=1.0,
          help="text search: a finished hypothesis' score is divided by length ** lenpen (1 = the plain length)")
        a("--temperature", type=float, default=1.0, help="text search: the logits are divided by it before the log-softmax")
        a("--no-repeat-ngram-size", type=int, default=0,
          help="text search: no n-gram of this size occurs twice in a hypothesis, committed prefix included (0 = off; 2 .. 32).  With "
               "any of these three off its default every write is a search behind the committed prefix as with --beam-mt > 1 (at "
               "beam 1 too), and the persistent MT step is not armed")
        a("--sampling", action="store_true", default=False,
          help="text search: every write samples --beam-mt chains behind the committed prefix and commits the best-scoring one "
               "(the persistent MT step is not armed); the stream key of a write is --sampling-session and the count of writes so "
               "far, so a replayed session samples the same")
        a("--sampling-topk", type=int, default=-1, help="with --sampling: sample from the k most likely tokens (-1 = off)")
        a("--sampling-topp", type=float, default=-1.0,
          help="with --sampling: sample from the smallest set of tokens whose mass reaches p (-1 = off; not with top-k)")
        a("--seed", type=int, default=1, help="seed of --sampling")
        a("--sampling-session", type=int, default=0, help="with --sampling: this session's id in the stream key")
        a("--word-details", action="store_true", default=False,
          help="after every policy() that ran the encoder, agent.details holds the words of both CTC heads with their time spans, "
               "confidences and stability (streamspeech_amd/words.py); default: off, the heads run exactly as without the flag")
        a("--ctc-beam", type=int, default=0,
          help="streaming ASR agent: K > 0 replaces the arg-max frame path by a CTC prefix beam search of beam K that is resumed on "
               "the encoder rows each call makes final (engine.CtcStream); every call writes the new text of the prefix all beam "
               "strings share, the last call the rest of the best hypothesis (agent.nbest: the final n-best); 0 = off, every "
               "launch and every output as without the flag")
        a("--ctc-beam-cand", type=int, default=None, help="with --ctc-beam: tokens a prefix is extended by per frame (default beam + 1, at most 32)")
        a("--ctc-lm", default=None, metavar="FILE",
          help="with --ctc-beam: an ARPA n-gram model (.arpa / .arpa.gz) over source_unigram, fused into the search")
        a("--ctc-lm-weight", type=float, default=0.5, help="with --ctc-lm: the weight of the model's log-probability (default 0.5)")
        a("--ctc-word-score", type=float, default=0.0, help="with --ctc-lm: added per token of a hypothesis (default 0)")
        a("--ctc-hotwords", default=None, metavar="FILE",
          help="with --ctc-beam: phrases to prefer, one per line as space-separated source_unigram pieces, optionally a tab and the "
               "phrase's per-token boost (hotwords.read_hotwords); biases the search towards them")
        a("--ctc-hotword-boost", type=float, default=1.5,
          help="with --ctc-hotwords: the per-token boost, in natural-log units, of a line that names none (default 1.5)")
        a("--ctc-keywords", default=None, metavar="FILE",
          help="streaming ASR agent: phrases to spot, one per line as space-separated source_unigram pieces, optionally a tab and "
               "the phrase's threshold (keywords.read_keywords); agent.hits collects their occurrences (keywords.KeywordHit, ms on "
               "the utterance's clock) as the encoder makes rows final; no beam search is needed; the S2TT and S2ST agents refuse "
               "the flag; default: off, every launch and every output as without the flag")
        a("--ctc-keyword-threshold", type=float, default=1.0,
          help="with --ctc-keywords: the threshold tau, in natural-log units per label, of a line that names none (default 1.0, a "
               "starting point that was not tuned on a trained checkpoint)")
        a("--mt-alignment", action="store_true", default=False,
          help="after every policy() that wrote, agent.alignment holds the words of all committed target tokens (the text decoder's, "
               "which the S2TT agent prints and the S2ST path speaks) with the source time span the decoder's cross-attention "
               "points at (streamspeech_amd/words.py AlignedWord); one extra decoder pass per write; default: off, every launch "
               "and every output as without the flag")
        a("--spoken-words", action="store_true", default=False,
          help="after every policy() that wrote, agent.spoken holds the words of all committed target tokens with the time span "
               "each is spoken at in the OUTPUT speech, in ms on the clock of the emitted samples (streamspeech_amd/words.py "
               "Spoken); exact, from the unit decoder's arg-max and the predicted durations; one small extra launch per write; "
               "default: off, every launch and every output as without the flag")
        a("--extra-output-dir", type=str, default=None, help="extra output dir")
        a("--output-asr-translation", type=bool, default=False, help="extra output dir")

    details = None      # --word-details: the words.CtcDetails of the last policy() that ran the encoder
    alignment = None    # --mt-alignment: the words.AlignedWord list of all committed target tokens, after the last policy() that wrote
    _spoken_last = None     # --spoken-words: (committed tokens, segments) as of the last write; the segments are kept by state index
    _spoken_words = None

    @property
    def spoken(self):
        """--spoken-words: the words.Spoken of all committed target tokens in the emitted speech as of the last policy() that
        wrote (None before the first); a finished utterance's words stay until the next utterance's first write."""
        if self._spoken_last is None:
            return None
        if self._spoken_words is None:
            from .words import spoken_from_segments
            self._spoken_words = spoken_from_segments(self._spoken_last[0], self._spoken_last[1], self.generator_mt.tgt_dict,
                                                      eos=self.generator_mt.eos)
        return self._spoken_words

    def reset(self):
        self._mt_writes = 0     # --sampling: writes so far, the second half of the stream key
        self._mt_align = []     # --mt-alignment: (committed tokens placed so far, the words of one write), frozen
        self._spoken_rec = None  # --spoken-words: segments, samples emitted and states seen of the utterance (made by its first write)
        self.src_seg_num = 0
        self.tgt_subwords_indices = None
        self.src_ctc_indices = None
        self.src_ctc_prefix_length = 0
        self.tgt_ctc_prefix_length = 0
        self.tgt_units_indices = None
        self.prev_output_tokens_mt = None
        self.tgt_text = []
        self.mt_decoder_out = None
        self.unit = None
        self.wav = []
        self.post_transcription = ""
        self.unfinished_wav = None
        self.states.reset()
        enc = getattr(getattr(self, "model", None), "encoder", None)
        if enc is not None and hasattr(enc, "reset_stream"):
            enc.reset_stream()                     # incremental encoder cache: one utterance at a time
        fe = getattr(self, "feature_extractor", None)
        if fe is not None:
            fe.clear_cache()                       # converted sample history of the previous utterance
        try:
            self.generator_mt.reset_incremental_states()
            self.ctc_generator.reset_incremental_states()
        except Exception:  # noqa: BLE001
            pass

    def load_model_vocab(self, args, model=None):
        """agent :355-420: checkpoint -> model, CMVN stats, dictionaries, chunk sizes."""
        args.global_cmvn = None
        config = {}
        if args.config_yaml is not None:
            ypath = os.path.join(args.data_bin, args.config_yaml)
            if os.path.exists(ypath):
                with open(ypath, "r") as f:
                    config = yaml.load(f, Loader=yaml.BaseLoader) or {}
                from .frontend import check_eval_transforms
                check_eval_transforms(config, getattr(args, "gen_subset", None) or "test")
                if "global_cmvn" in config:
                    npz = config["global_cmvn"]["stats_npz_path"]
                    if not os.path.exists(npz):  # reference YAMLs hold absolute paths of the authors' machine
                        npz = os.path.join(args.data_bin, os.path.basename(npz))
                    args.global_cmvn = np.load(npz)
        if args.global_cmvn is None and getattr(args, "global_stats", None):
            args.global_cmvn = np.load(args.global_stats)
        if model is None:
            sd, uni = load_model_state(args.model_path)     # raises IOError("Model file not found") like the agent
            model = StreamSpeechModel(sd, device=self.device, cmvn=args.global_cmvn, uni_encoder=uni)
        self.model = model
        self.models = [model]
        eng = model.hip if hasattr(model, "hip") else model
        self.feature_extractor = OnlineFeatureExtractor(args, eng)

        chunk_size = args.source_segment_size // 40
        model.encoder.chunk_size = chunk_size
        conv_chunk = 16 if chunk_size >= 16 else 8
        for conv in model.encoder.subsample.conv_layers:
            conv.chunk_size = conv_chunk
        for layer in model.encoder.conformer_layers:
            layer.conv_module.depthwise_conv.chunk_size = conv_chunk
        if hasattr(model.encoder, "incremental"):
            model.encoder.incremental = not getattr(args, "full_recompute_encoder", False)
            # a resampled source re-computes its last ~10 output samples when more audio arrives (zero-padded
            # FIR edge), so the newest fbank frame is not settled: the incremental encoder must not cache rows
            # that can see it
            if hasattr(eng, "encoder_stream_set_tail"):
                from .frontend import unsettled_fbank_frames
                eng.encoder_stream_set_tail(unsettled_fbank_frames(int(args.sample_rate), SAMPLE_RATE,
                                                                   int(args.shift_size * SAMPLE_RATE / 1000)))

        self.dict = load_dictionaries(args, eng.cfg)

    @torch.inference_mode()
    def policy(self):
        feature = self.feature_extractor(self.states.source)
        if feature.size(0) == 0 and not self.states.source_finished:
            return ReadAction()
        if feature.size(0) < 1:
            return self._finish_empty() if self.states.source_finished else ReadAction()

        src_indices = feature.unsqueeze(0)
        src_lengths = torch.tensor([feature.size(0)]).long()
        model = self.model
        encoder_out = model.encoder(src_indices, src_lengths)
        self.encoder_outs = [encoder_out]

        # ASR / ST CTC heads (agent :437-478)
        wd = bool(getattr(self.args, "word_details", False))
        wkw = {"want_scores": True} if wd else {}
        finalized_asr = self.asr_ctc_generator.generate(encoder_out, aux_task_name="source_unigram", **wkw)
        src_ctc_indices = finalized_asr[0][0]["tokens"].int()
        if (self.states.source_finished and not self.quiet) or self.output_asr_translation:
            text = _detok([self.dict["source_unigram"][c] for c in src_ctc_indices])
            if self.states.source_finished and not self.quiet:
                with open(self.asr_file, "a") as f:
                    print(text, file=f)
            if self.output_asr_translation:
                print("Streaming ASR:", text)
        finalized_st = self.st_ctc_generator.generate(encoder_out, aux_task_name="ctc_target_unigram", **wkw)
        tgt_ctc_indices = finalized_st[0][0]["tokens"].int()
        if wd:
            self.details = word_details(self, finalized_asr[0][0], finalized_st[0][0])

        # read/write gate on the CTC token counts (agent :480-512)
        if not self.states.source_finished:
            src_ctc_prefix_length = src_ctc_indices.size(-1)
            tgt_ctc_prefix_length = tgt_ctc_indices.size(-1)
            self.src_ctc_indices = src_ctc_indices
            if (src_ctc_prefix_length < self.src_ctc_prefix_length + self.stride_n
                    or tgt_ctc_prefix_length < self.tgt_ctc_prefix_length + self.stride_n):
                return ReadAction()
            self.src_ctc_prefix_length = max(src_ctc_prefix_length, self.src_ctc_prefix_length)
            self.tgt_ctc_prefix_length = max(tgt_ctc_prefix_length, self.tgt_ctc_prefix_length)
            subword_tokens = ((tgt_ctc_prefix_length - self.lagging_k1) // self.stride_n) * self.stride_n
            if self.whole_word:
                subword_tokens += 1
            new_subword_tokens = (subword_tokens - self.tgt_subwords_indices.size(-1)
                                  if self.tgt_subwords_indices is not None else subword_tokens)
            if new_subword_tokens < 1:
                return ReadAction()
        else:
            self.src_ctc_indices = src_ctc_indices
            new_subword_tokens = -1
        new_subword_tokens = int(new_subword_tokens)

        # 1. MT decoder: greedy continuation of the committed prefix (agent :520-538)
        finalized_mt = self.generator_mt.generate_decoder(
            self.encoder_outs, src_indices, src_lengths, {"id": 1}, self.tgt_subwords_indices, None, None,
            aux_task_name=model.mt_task_name, max_new_tokens=new_subword_tokens, **sampling_key_kwargs(self))
        hyp = finalized_mt[0][0]
        if hyp["tokens"][-1] == 2:
            tgt_subwords_indices = hyp["tokens"][:-1].unsqueeze(0)
        else:
            tgt_subwords_indices = hyp["tokens"].unsqueeze(0)

        if self.whole_word:  # agent :540-574 (the KV-cache surgery there is dead code: no incremental states)
            if not self.states.source_finished:
                j = 999999
                for j in range(tgt_subwords_indices.size(-1) - 1, -1, -1):
                    if self.generator_mt.tgt_dict[tgt_subwords_indices[0][j]].startswith("▁"):
                        break
                tgt_subwords_indices = tgt_subwords_indices[:, :j]
                hyp["tokens"] = hyp["tokens"][:j]
                if j == 0:
                    return ReadAction()

        # agent :576-591: max_tgt_len = len(tokens) (+1 in whole-word mode), row = [eos, tokens-without-eos, <pad>...].
        # A non-final whole-word hypothesis was cut to [:j] above and lost its eos, so its row has NO pad; a
        # final one keeps the eos and gets exactly one trailing <pad> position.
        max_tgt_len = len(hyp["tokens"]) + (1 if self.whole_word else 0)
        tmp = hyp["tokens"].int()
        if len(tmp) > 0 and tmp[-1] == self.generator_mt.eos:
            tmp = tmp[:-1]
        n_tail_pad = max_tgt_len - (len(tmp) + 1)
        assert n_tail_pad in (0, 1), "hypothesis without eos outside whole-word mode (the reference fails here too)"
        prev_output_tokens_mt = torch.full((1, max_tgt_len), self.model.target_unigram_decoder.padding_idx
                                           if hasattr(self.model, "target_unigram_decoder") else 1, dtype=torch.int32)
        prev_output_tokens_mt[0, 0] = self.generator_mt.eos
        prev_output_tokens_mt[0, 1:len(tmp) + 1] = tmp
        if (self.states.source_finished and not self.quiet) or self.output_asr_translation:
            text = _detok([self.generator_mt.tgt_dict[c] for c in tmp])
            if self.states.source_finished and not self.quiet:
                with open(self.st_file, "a") as f:
                    print(text, file=f)
            if self.output_asr_translation:
                print("Simultaneous translation:", text)

        if self.tgt_subwords_indices is not None and torch.equal(self.tgt_subwords_indices, tgt_subwords_indices):
            if not self.states.source_finished:
                return ReadAction()
            return self._finish_empty()
        self.tgt_subwords_indices = tgt_subwords_indices

        if not self.states.source_finished and self.prev_output_tokens_mt is not None:
            if (torch.equal(self.prev_output_tokens_mt, prev_output_tokens_mt)
                    or prev_output_tokens_mt.size(-1) <= self.prev_output_tokens_mt.size(-1)):
                return ReadAction()
        self.prev_output_tokens_mt = prev_output_tokens_mt

        # MT decoder states of [eos, tokens...] = the features the greedy pass already produced
        # (causal: a prefix slice is exact); the reference recomputes them (agent :638-651).
        mt_feats = hyp["features"][: len(tmp) + 1]
        if n_tail_pad:
            # whole-word mode: prev_output_tokens_mt carries one trailing <pad> (agent :576-584); the
            # reference runs that position through the MT decoder, T2U encoder and unit decoder with
            # key-padding masks, and its 25 unit positions are decoded like any other
            eng = self.engine
            if self.generator_mt.beam_size > 1 or self.generator_mt.search or self.generator_mt.sampling is not None:   # the beam search leaves no single-utterance KV cache to append to: one ragged pass
                enc = self.encoder_outs[0]["encoder_out"][0]
                enc = (enc[:, 0] if enc.dim() == 3 else enc).contiguous()
                mt_feats = eng.batch_mt_features(enc, [int(enc.shape[0])], [[int(t) for t in tmp]], [1])[0]
            else:
                eng.mt_truncate(len(tmp) + 1)
                pad_feat, _ = eng.mt_append([int(prev_output_tokens_mt[0, -1])], len(tmp) + 1, False, False,
                                            want_next=False, n_tail_pad=1)
                mt_feats = torch.cat((mt_feats, pad_feat), 0)
        self.mt_decoder_out = mt_feats
        if getattr(self.args, "mt_alignment", False):      # the search and the tail-pad append are done: the MT state is not needed any more
            mt_alignment_update(self, self.encoder_outs[0]["encoder_out"][0], tmp)

        # 2+3. T2U encoder + CTC unit decoder + CTC search (agent :661-689)
        sw = bool(getattr(self.args, "spoken_words", False))
        finalized = self.ctc_generator.generate(mt_feats, prefix=self.tgt_units_indices, n_tail_pad=n_tail_pad,
                                                **({"keep_raw": True} if sw else {}))
        if len(finalized[0][0]["tokens"]) == 0:
            if not self.states.source_finished:
                return ReadAction()
            return self._finish_empty()
        tmp_u = finalized[0][0]["tokens"].int()
        if tmp_u[-1] == self.eos:
            tmp_u = tmp_u[:-1]
        unit = []
        for c in tmp_u:
            u = self.dict["tgt"][c].replace("<s>", "").replace("</s>", "")
            if u != "":
                unit.append(int(u))
        if self.states.source_finished and not self.quiet:
            with open(self.unit_file, "a") as f:
                print(" ".join(str(_) for _ in unit), file=f)
        cur_unit = unit if self.unit is None else unit[len(self.unit):]
        if len(unit) < 1 or len(cur_unit) < 1:
            if not self.states.source_finished:
                return ReadAction()
            return self._finish_empty()

        # 4. vocoder over ALL units so far; emit the tail that belongs to the new units (agent :743-753)
        tail_info = {} if sw else None
        new_wav, wav = synthesize_tail(self.vocoder, unit, len(cur_unit), self.dur_prediction, self.vocoder_ctx,
                                       self.vocoder_rf, **({} if self.speaker_id is None else {"spkr": self.speaker_id}),
                                       **({"info": tail_info} if sw else {}))
        carried = 0
        if self.unfinished_wav is not None and len(self.unfinished_wav) > 0:
            carried = len(self.unfinished_wav)
            new_wav = torch.cat((self.unfinished_wav, new_wav), dim=0)
        if sw:
            spoken_update(self, finalized[0][0]["raw_device"], mt_feats.shape[0], len(unit), len(cur_unit), tail_info["first"],
                          tail_info["dur"].view(-1).tolist(), tmp.tolist(), carried, len(new_wav))
        self.wav = wav
        self.unit = unit

        if self.states.source_finished and new_subword_tokens == -1:
            self.states.target_finished = True
            # self.reset() in the reference (agent :759-761) also clears the states; kept
            self.reset()
        return WriteAction(
            SpeechSegment(content=new_wav.tolist(), sample_rate=SAMPLE_RATE, finished=self.states.source_finished),
            finished=self.states.target_finished)

    def _finish_empty(self):
        return WriteAction(
            SpeechSegment(content=(self.unfinished_wav.tolist() if self.unfinished_wav is not None else []),
                          sample_rate=SAMPLE_RATE, finished=True),
            finished=True)
