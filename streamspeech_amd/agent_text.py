"""Streaming-ASR and simultaneous-S2TT agents of StreamSpeech on the HIP backend: strict prefixes of
the S2ST path -- same encoder + CTC heads (+ MT greedy search), text out.

Reference: agent/speech_to_text.asr.streamspeech.agent.py:385-433 and
agent/speech_to_text.s2tt.streamspeech.agent.py:381-545 (same flags as the S2ST agent minus the
vocoder ones)."""
import torch

from .agent import StreamSpeechS2STAgent, _beam_kwargs, _greedy_mt, _detok, mt_alignment_update, sampling_key_kwargs, word_details
from .frontend import OnlineFeatureExtractor  # noqa: F401  (re-exported for parity with the reference files)
from .generators import CTCDecoder, SequenceGenerator
from .simuleval_shim import ReadAction, SpeechToTextAgent, WriteAction, entrypoint
from .text_policy import asr_beam_emit, ctc_beam_flags, ctc_keyword_flags, s2tt_gate


def _add_text_args(parser):
    StreamSpeechS2STAgent.add_args(parser)
    for act in parser._actions:           # the text agents have no vocoder
        if "--vocoder" in act.option_strings:
            act.required = False


class _TextAgentBase(SpeechToTextAgent):
    def __init__(self, args, model=None):
        super().__init__(args)
        self.args = args
        self.device = getattr(args, "device_str", "cuda:0")
        # checkpoint / CMVN / dictionaries / chunk sizes exactly as the S2ST agent (agent :355-420)
        StreamSpeechS2STAgent.load_model_vocab(self, args, model)
        torch.set_grad_enabled(False)
        eng = self.model.hip if hasattr(self.model, "hip") else self.model
        self.engine = eng
        beam_mt = int(getattr(args, "beam_mt", 1))
        if hasattr(eng, "set_persistent_mt_step") and _greedy_mt(args):   # HIP engine: the greedy MT decode step as one persistent launch (mt_step.hip)
            eng.set_persistent_mt_step(int(getattr(args, "mt_step_workgroups", 64)))
        self.asr_ctc_generator = CTCDecoder(self.dict["source_unigram"], eng, 0)
        self.st_ctc_generator = CTCDecoder(self.dict["ctc_target_unigram"], eng, 1)
        if hasattr(eng, "set_persistent_mt_step"):       # both CTC heads per call only in the translation agent (engine.ctc_greedy)
            eng.ctc_speculate = type(self).__name__ == "StreamSpeechS2TTAgent"
        tgt_dict_mt = self.dict[self.model.mt_task_name]
        # the text agents search with max_len_a=1, max_len_b=200 (s2tt agent :161-180) -- NOT the S2ST agent's 0 / 100:
        # a final hypothesis may run to (fbank frames + 200) subwords
        self.generator_mt = SequenceGenerator(eng, tgt_dict_mt, beam_size=beam_mt, max_len_a=1, max_len_b=200, max_len=0,
                                              min_len=1, eos=tgt_dict_mt.eos(), use_incremental_states=False, **_beam_kwargs(args))
        self.lagging_k1, self.stride_n = args.lagging_k1, args.stride_n
        self.quiet = args.extra_output_dir is None
        if not self.quiet:
            from pathlib import Path
            self.asr_file = Path(args.extra_output_dir + "/asr.txt")
            self.st_file = Path(args.extra_output_dir + "/st.txt")
        self.reset()

    add_args = staticmethod(_add_text_args)
    details = None      # --word-details: the words.CtcDetails of the last policy() that ran the encoder
    alignment = None    # --mt-alignment: the words.AlignedWord list of all committed target tokens, after the last policy() that wrote

    def _ctc_hyps(self, enc):
        """The two CTC hypotheses of policy(); with --word-details the scored form, and agent.details from them."""
        if not getattr(self.args, "word_details", False):
            return None
        src = self.asr_ctc_generator.generate(enc, aux_task_name="source_unigram", want_scores=True)[0][0]
        tgt = self.st_ctc_generator.generate(enc, aux_task_name="ctc_target_unigram", want_scores=True)[0][0]
        self.details = word_details(self, src, tgt)
        return src, tgt

    def reset(self):
        self._mt_writes = 0     # --sampling: writes so far, the second half of the stream key
        self._mt_align = []     # --mt-alignment: (committed tokens placed so far, the words of one write), frozen
        self.tgt_subwords_indices = None
        self.src_ctc_prefix_length = 0
        self.tgt_ctc_prefix_length = 0
        self.asr_text = ""
        self.tgt_text = ""
        self.states.reset()
        enc = getattr(getattr(self, "model", None), "encoder", None)
        if enc is not None and hasattr(enc, "reset_stream"):
            enc.reset_stream()                     # incremental encoder cache: one utterance at a time
        if getattr(self, "ctc_stream", None) is not None:
            self.ctc_stream.reset(0)               # --ctc-beam: the search of the utterance before
            self._ctc_frames = 0
        if getattr(self, "spot_stream", None) is not None:
            self.spot_stream.reset(0)              # --ctc-keywords: the spotter of the utterance before (agent.hits stays)
            self._spot_frames = 0
        fe = getattr(self, "feature_extractor", None)
        if fe is not None:
            fe.clear_cache()                       # converted sample history of the previous utterance

    def _encode(self):
        feature = self.feature_extractor(self.states.source)
        if feature.size(0) == 0:
            return None, None, None
        src_indices = feature.unsqueeze(0)
        return self.model.encoder(src_indices, None), src_indices, torch.tensor([feature.size(0)]).long()


@entrypoint
class StreamSpeechASRAgent(_TextAgentBase):
    """Streaming ASR: encoder + source_unigram CTC greedy, emits the newly confirmed subwords.  With --ctc-beam K the arg-max path
    gives way to the resumable CTC prefix beam search (engine.CtcStream, one slot): each call moves the search over the rows the
    incremental encoder has made final and writes the new text of the stable prefix; the last call takes all rows and writes the
    rest of the best hypothesis, so the writes of an utterance add up to its final best hypothesis and none is ever retracted.
    An utterance may run to lib.CTC_BEAM_MAX_FRAMES encoder rows (60 s)."""

    ctc_stream = None
    spot_stream = None
    hits = None         # --ctc-keywords: the keywords.KeywordHit of every policy() so far, in the order they were reported
    nbest = None        # --ctc-beam: the engine.CtcHypothesis list of the last finished utterance, best first
    partial = None      # --ctc-beam: the symbols of the current best hypothesis, unstable tail included (for display)

    def __init__(self, args, model=None):
        if getattr(args, "mt_alignment", False):
            raise ValueError("--mt-alignment needs the first-pass text search; the ASR agent has none")
        opts = ctc_beam_flags(args, "asr")                 # before anything is loaded: the refusals need no GPU
        kw_file = ctc_keyword_flags(args, "asr")
        super().__init__(args, model)
        if kw_file:
            from .engine import CtcSpotStream
            from .keywords import CtcKeywords
            self.keywords = CtcKeywords.from_file(args.ctc_keywords, self.dict["source_unigram"], float(args.ctc_keyword_threshold))
            self.hits, self._spot_frames = [], 0
            self.spot_stream = CtcSpotStream(self.engine, 0, 1, self.keywords)
        if opts is not None:
            from .engine import CtcStream
            from .lib import CTC_BEAM_MAX_FRAMES
            if getattr(args, "ctc_lm", None):
                from .ngram import NgramLM, read_arpa
                opts.lm = NgramLM(read_arpa(args.ctc_lm, self.dict["source_unigram"]))
            if getattr(args, "ctc_hotwords", None):
                from .hotwords import CtcBias, read_hotwords
                d = self.dict["source_unigram"]
                opts.bias = CtcBias(*read_hotwords(args.ctc_hotwords, d, args.ctc_hotword_boost), len(d), d.pad(), d.unk())
            self._ctc_frames = 0
            self.ctc_stream = CtcStream(self.engine, 0, 1, CTC_BEAM_MAX_FRAMES, **opts.stream_kwargs())

    def _beam_policy(self, enc):
        rows = enc["encoder_out"][0][:, 0, :].contiguous()
        T2, fin = int(rows.shape[0]), bool(self.states.source_finished)
        # rows below the incremental encoder's n_final never change; without the incremental encoder nothing is final before the end
        n_final = int(self.engine.stream_stats[0]) if getattr(self.model.encoder, "incremental", False) else 0
        upto = T2 if fin else max(self._ctc_frames, min(n_final, T2))
        part = self.ctc_stream.advance([0], rows, [T2], [upto], [fin])[0]
        self._ctc_frames = 0 if fin else upto
        symbols = [self.dict["source_unigram"][c] for c in part.hyps[0].tokens] if part.hyps else []
        self.partial = symbols
        new_text, self.asr_text = asr_beam_emit(self.asr_text, symbols, part.n_stable, fin)
        if fin:
            self.nbest = part.hyps
            if not self.quiet:
                with open(self.asr_file, "a") as f:
                    print(_detok(symbols), file=f)
            self.states.target_finished = True
            self.reset()
        return WriteAction(new_text, finished=self.states.target_finished)

    def _spot(self, enc):
        """--ctc-keywords: the spotter moves over the rows the incremental encoder has made final (all, with final, at the end),
        as _beam_policy moves the search; what it emits joins agent.hits."""
        from .keywords import KeywordHit
        from .words import FRAME_MS
        rows = enc["encoder_out"][0][:, 0, :].contiguous()
        T2, fin = int(rows.shape[0]), bool(self.states.source_finished)
        n_final = int(self.engine.stream_stats[0]) if getattr(self.model.encoder, "incremental", False) else 0
        upto = T2 if fin else max(self._spot_frames, min(n_final, T2))
        got = self.spot_stream.advance([0], rows, [T2], [upto], [fin])[0]
        self._spot_frames = 0 if fin else upto
        self.hits.extend(KeywordHit(h.keyword, self.keywords.texts[h.keyword], h.start * FRAME_MS, (h.end + 1) * FRAME_MS, h.score, h.norm)
                         for h in got.hits)

    @torch.inference_mode()
    def policy(self):
        enc, _, _ = self._encode()
        if enc is None:
            return WriteAction("", finished=True) if self.states.source_finished else ReadAction()
        if self.spot_stream is not None:
            self._spot(enc)
        if self.ctc_stream is not None:
            return self._beam_policy(enc)
        scored = self._ctc_hyps(enc)
        hyp = scored[0] if scored else self.asr_ctc_generator.generate(enc, aux_task_name="source_unigram")[0][0]
        tokens = [self.dict["source_unigram"][c] for c in hyp["tokens"].int()]
        if self.states.source_finished and not self.quiet:
            with open(self.asr_file, "a") as f:
                print(_detok(tokens), file=f)
        text = " ".join(tokens)
        new_text = text[len(self.asr_text):]
        self.asr_text = text
        if self.states.source_finished:
            self.states.target_finished = True
            self.reset()
        return WriteAction(new_text, finished=self.states.target_finished)


@entrypoint
class StreamSpeechS2TTAgent(_TextAgentBase):
    """Simultaneous speech-to-text translation: encoder + both CTC heads (read/write gate) + MT greedy."""

    def __init__(self, args, model=None):
        ctc_beam_flags(args, "S2TT")                       # (raises: the flags are the ASR agent's)
        ctc_keyword_flags(args, "S2TT")
        super().__init__(args, model)

    @torch.inference_mode()
    def policy(self):
        enc, src_indices, src_lengths = self._encode()
        if enc is None:
            return WriteAction("", finished=True) if self.states.source_finished else ReadAction()
        scored = self._ctc_hyps(enc)
        if scored:
            src_ctc, tgt_ctc = scored[0]["tokens"].int(), scored[1]["tokens"].int()
        else:
            src_ctc = self.asr_ctc_generator.generate(enc, aux_task_name="source_unigram")[0][0]["tokens"].int()
            tgt_ctc = self.st_ctc_generator.generate(enc, aux_task_name="ctc_target_unigram")[0][0]["tokens"].int()
        gate = s2tt_gate(src_ctc.size(-1), tgt_ctc.size(-1), self.src_ctc_prefix_length, self.tgt_ctc_prefix_length,
                         self.tgt_subwords_indices.size(-1) if self.tgt_subwords_indices is not None else 0, self.lagging_k1,
                         self.stride_n, self.states.source_finished)
        self.src_ctc_prefix_length, self.tgt_ctc_prefix_length = gate.src_prefix_len, gate.tgt_prefix_len
        if not gate.write:
            return ReadAction()
        new_subword_tokens = gate.new_tokens
        hyp = self.generator_mt.generate_decoder([enc], src_indices, src_lengths, {"id": 1}, self.tgt_subwords_indices,
                                                 None, None, aux_task_name=self.model.mt_task_name,
                                                 max_new_tokens=int(new_subword_tokens), **sampling_key_kwargs(self))[0][0]
        toks = hyp["tokens"]
        tgt_subwords_indices = (toks[:-1] if toks[-1] == 2 else toks).unsqueeze(0)
        tokens = [self.generator_mt.tgt_dict[c] for c in tgt_subwords_indices[0]]
        if self.states.source_finished and not self.quiet:
            with open(self.st_file, "a") as f:
                print(_detok(tokens), file=f)
        if self.tgt_subwords_indices is not None and torch.equal(self.tgt_subwords_indices, tgt_subwords_indices):
            return WriteAction("", finished=True) if self.states.source_finished else ReadAction()
        self.tgt_subwords_indices = tgt_subwords_indices
        if getattr(self.args, "mt_alignment", False):      # the search has returned: nothing reads the MT scratch any more
            mt_alignment_update(self, enc["encoder_out"][0], tgt_subwords_indices[0].tolist())
        text = " ".join(tokens)
        new_text = text[len(self.tgt_text):]
        self.tgt_text = text
        if self.states.source_finished and new_subword_tokens == -1:
            self.states.target_finished = True
            self.reset()
        return WriteAction(new_text, finished=self.states.target_finished)
