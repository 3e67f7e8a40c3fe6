"""Generators the agent instantiates, same names / argument meaning / return structure as the
reference's ``agent/ctc_decoder.py``, ``agent/ctc_generator.py`` and ``agent/sequence_generator.py``,
over the HIP stages.  ``engine`` is anything with the HipModel method set (tests substitute a
CPU-oracle adapter to exercise the host control flow without a GPU).
"""
from typing import Dict, List, Optional

import torch

from .text_policy import mt_max_len


class CTCDecoder:
    """agent/ctc_decoder.py:30-111 -- ASR / ST CTC greedy search (blank = index 0)."""

    def __init__(self, tgt_dict, engine, head: int):
        self.tgt_dict, self.engine, self.head = tgt_dict, engine, head
        self.pad, self.eos, self.unk = tgt_dict.pad(), tgt_dict.eos(), tgt_dict.unk()

    @torch.no_grad()
    def generate(self, encoder_out, prefix=None, aux_task_name=None, want_lprobs=False, want_scores=False, **kw):
        """want_scores: the hypothesis also carries `positional_scores` (float32 [Tp], agent/ctc_decoder.py:61-62,104) and `score`
        (their sum, :105, taken on the host in float64), plus `last` / `token_scores`: each token's last frame and the sum of
        positional_scores over its run of frames (what streamspeech_amd.words turns into word spans and confidences)."""
        enc = encoder_out["encoder_out"][0]
        enc = enc[:, 0] if enc.dim() == 3 else enc
        last = tok_lp = lp = None
        if want_scores:
            toks, index, raw, logits, last, tok_lp, lp = self.engine.ctc_greedy(self.head, enc.contiguous(), want_logits=want_lprobs,
                                                                                want_scores=True)
        else:
            toks, index, raw, logits = self.engine.ctc_greedy(self.head, enc.contiguous(), want_logits=want_lprobs)
        if prefix is not None:  # agent/ctc_decoder.py:90-92
            pre = [int(t) for t in prefix.view(-1).tolist()]
            merged = pre + raw.tolist()[len(pre):]
            from .pipeline import ctc_collapse_host, ctc_collapse_spans_host
            if want_scores:      # the scores stay those of the arg-max (the reference splices ids only), the spans follow the merged ids
                toks, index, last, tok_lp = ctc_collapse_spans_host(merged, lp, 0, self.pad)
            else:
                toks, index = ctc_collapse_host(merged, 0, self.pad)
            raw = torch.tensor(merged, dtype=torch.int32)
        lprobs = None
        if logits is not None:
            # model.get_normalized_probs + "never select pad, unk" (agent/ctc_decoder.py:52-60), on the engine (ss_log_softmax)
            lprobs = self.engine.normalized_probs(logits, True, self.pad, self.unk).unsqueeze(0)
        hyp = {"tokens": torch.tensor(toks, dtype=torch.long), "org_tokens": raw, "lprobs": lprobs,
               "index": index, "attn": None, "alignment": None}
        if want_scores:
            import numpy as np
            hyp.update({"positional_scores": torch.from_numpy(np.ascontiguousarray(lp, dtype=np.float32)),
                        "score": float(np.asarray(lp, dtype=np.float64).sum()), "last": list(last),
                        "token_scores": torch.from_numpy(np.ascontiguousarray(tok_lp, dtype=np.float32))})
        return [[hyp]]


    @torch.no_grad()
    def align(self, encoder_out, tokens, **kw):
        """Forced alignment of the given label ids on this head: what generate takes plus the labels -> a hypothesis with `tokens`,
        `index` (each token's first frame), `last`, `token_scores` (float32, the sum of the per-frame log-probability over the
        token's run), `score` (log p(tokens | audio), the CTC forward sum), `viterbi_score` (the best path's), `status` (0 aligned,
        1 infeasible, 2 NaN) and `path` (token id per frame, 0 = blank).  words.details_from_hyps / words_from_ctc take it as they
        take generate's; an infeasible hypothesis has no tokens placed (`index` / `last` are -1, `token_scores` NaN)."""
        enc = encoder_out["encoder_out"][0]
        enc = enc[:, 0] if enc.dim() == 3 else enc
        ids = [int(t) for t in (tokens.view(-1).tolist() if torch.is_tensor(tokens) else tokens)]
        a = self.engine.ctc_align(self.head, enc.contiguous(), ids)
        import numpy as np
        return [[{"tokens": torch.tensor(ids, dtype=torch.long), "index": list(a.first), "last": list(a.last),
                  "token_scores": torch.from_numpy(np.ascontiguousarray(a.tok_lprob, dtype=np.float32)), "score": a.score,
                  "viterbi_score": a.viterbi_score, "status": a.status, "path": a.path, "attn": None, "alignment": None}]]


    @torch.no_grad()
    def beam_search(self, encoder_out, beam, cand=None, nbest=None, lm=None, lm_weight=0.0, word_score=0.0, bias=None, bias_scale=1.0,
                    **kw):
        """CTC prefix beam search on this head: what generate takes plus the beam -> [[hypothesis, ...]] best first, each with
        `tokens` (never blank, pad or unk) and `score`, the log of the summed probability of the alignments of those tokens --
        the scale of align's `score`, so align(encoder_out, h["tokens"]) places a hypothesis in time for words.*.
        lm (an ngram.NgramLM over this head's dictionary), lm_weight, word_score: shallow fusion -- `score` is then the fused one
        the hypotheses are ranked by, and each hypothesis also has `ctc_score` (the scale above) and `lm_score`.
        bias (a hotwords.CtcBias over this head's dictionary), bias_scale: hotword biasing, with lm or without -- `score` is the
        fused one, and each hypothesis also has `ctc_score` and `bias_score` (and `lm_score` with lm)."""
        enc = encoder_out["encoder_out"][0]
        enc = enc[:, 0] if enc.dim() == 3 else enc
        if bias is not None:
            fuse = {} if lm is None else {"lm": lm, "lm_weight": float(lm_weight), "word_score": float(word_score)}
            hyps = self.engine.ctc_beam(self.head, enc.contiguous(), int(beam), cand, nbest, bias=bias, bias_scale=float(bias_scale), **fuse)
            extra = lambda h: {"ctc_score": h.ctc_score, **({} if lm is None else {"lm_score": h.lm_score}),  # noqa: E731
                               "bias_score": h.bias_score}
        elif lm is None:
            hyps = self.engine.ctc_beam(self.head, enc.contiguous(), int(beam), cand, nbest)
            extra = lambda h: {}  # noqa: E731
        else:
            hyps = self.engine.ctc_beam(self.head, enc.contiguous(), int(beam), cand, nbest, lm=lm, lm_weight=float(lm_weight),
                                        word_score=float(word_score))
            extra = lambda h: {"ctc_score": h.ctc_score, "lm_score": h.lm_score}  # noqa: E731
        return [[{"tokens": torch.tensor(h.tokens, dtype=torch.long), "score": h.score, "attn": None, "alignment": None,
                  "positional_scores": None, **extra(h)} for h in hyps]]

    @torch.no_grad()
    def spot(self, encoder_out, keywords, max_hits=256, **kw):
        """Keyword spotting on this head: what generate takes plus the set (a keywords.CtcKeywords over this head's dictionary)
        -> the utterance's keywords.CtcHit tuples sorted by (end, keyword, start), start and end in encoder rows, both inclusive
        (words.FRAME_MS each).  No beam search is involved, and a phrase the arg-max path got a piece wrong on is still found
        within its threshold."""
        enc = encoder_out["encoder_out"][0]
        enc = enc[:, 0] if enc.dim() == 3 else enc
        return self.engine.ctc_spot(self.head, enc.contiguous(), keywords, int(max_hits))


class CTCSequenceGenerator:
    """agent/ctc_generator.py:26-123 -- NAR unit search over the T2U+unit-decoder stage
    (blank = tgt_dict.blank_index = 1004)."""

    def __init__(self, tgt_dict, engine, use_incremental_states=False, t2u_causal=False, mask_eos=False):
        assert not use_incremental_states
        self.tgt_dict, self.engine = tgt_dict, engine
        self.t2u_causal, self.mask_eos = t2u_causal, mask_eos
        self.incremental_states = None

    def reset_incremental_states(self):
        self.incremental_states = None

    @torch.no_grad()
    def generate(self, mt_features: torch.Tensor, prefix=None, n_tail_pad: int = 0, keep_raw: bool = False, **kw):
        """mt_features [n,512] = the MT decoder states the reference feeds to synthesizer_encoder
        (agent :652-689; T2U encoder and unit decoder run inside one C-ABI stage).  keep_raw: the hypothesis also carries
        ``raw_device``, the arg-max ids where the engine left them (what engine.batch_unit_spans reads)."""
        assert prefix is None, "tgt_units_indices is never set by the reference agent (SURVEY.md App. B)"
        if keep_raw:
            toks, raw, _, raw_dev = self.engine.t2u_units(mt_features, t2u_causal=self.t2u_causal, mask_eos=self.mask_eos,
                                                          n_tail_pad=n_tail_pad, keep_raw=True)
            return [[{"tokens": torch.tensor(toks, dtype=torch.long), "org_tokens": raw, "attn": None, "alignment": None,
                      "raw_device": raw_dev}]]
        toks, raw, _ = self.engine.t2u_units(mt_features, t2u_causal=self.t2u_causal, mask_eos=self.mask_eos,
                                             n_tail_pad=n_tail_pad)
        return [[{"tokens": torch.tensor(toks, dtype=torch.long), "org_tokens": raw, "attn": None, "alignment": None}]]


def unpack_constraints(constraints, B: int):
    """The ``constraints=`` of a generator call -> per-utterance phrase lists.  Takes fairseq's packed tensor [B, maxlen]
    (token_generation_constraints.pack_constraints: each row is the phrase count, then every phrase followed by a 0, zero-padded)
    or a list of B lists of token id lists."""
    if torch.is_tensor(constraints):
        if constraints.dim() == 1:
            constraints = constraints.unsqueeze(0)
        if constraints.dim() != 2 or constraints.size(0) != B:
            raise ValueError(f"packed constraints of shape {tuple(constraints.shape)} for a batch of {B}")
        out = []
        for row in constraints.tolist():
            phrases, off = [], 1
            for _ in range(int(row[0])):
                if 0 not in row[off:]:
                    raise ValueError("packed constraints: a phrase without its closing 0")
                where = row.index(0, off)
                phrases.append([int(t) for t in row[off:where]])
                off = where + 1
            out.append(phrases)
        return out
    out = [[[int(t) for t in p] for p in (c or [])] for c in constraints]
    if len(out) != B:
        raise ValueError(f"constraints for {len(out)} utterances, batch of {B}")
    return out


class SequenceGenerator:
    """agent/sequence_generator.py:165-582 at beam_size = 1: greedy first-pass text
    decoding with prefix and ``max_new_tokens``.  Keeps the reference's token-buffer semantics
    ([eos, prefix...], forced eos at max_len, eos banned below min_len) but feeds only NEW positions
    to the decoder thanks to the KV cache (per-position results are identical).

    beam_size > 1: a beam search behind the forced prefix with the semantics of the OFFLINE generator's ``prefix_tokens``
    (unity/sequence_generator.py with fairseq's ``_prefix_tokens``: one live hypothesis after the prefix, scores and length
    normalisation count the prefix), on the engine's ``batch_mt_beam_continue``.  The agents' own generator pre-fills the prefix and
    ranks k identical rows at the first free step, which is defined only at beam 1; that is the path above and it is unchanged.

    len_penalty / temperature / no_repeat_ngram_size: the reference generator's arguments of the same names (ss_mt_search_opts in
    include/streamspeech_hip.h has their exact rules).  With any of them off its default the search is ``batch_mt_beam_continue`` at
    beam 1 as well.  ``match_source_len=True`` raises.

    sampling / sampling_topk / sampling_topp / seed: the names fairseq's ``build_generator`` reads (-1 = the control is off).  With
    ``sampling`` the search is ``batch_mt_sample_continue``: beam_size independent ancestral samples behind the prefix, ordered by
    score (the rule: ss_mt_sample_opts in the header).  The stream key of a call is ``sampling_key=`` of generate_decoder, else the
    sample's ``"id"``, else 0: the same key and seed give the same samples.

    constraints= of generate_decoder: phrases every hypothesis must contain, in order (fairseq's --constraints with the ordered
    representation; the rule: ss_batch_mt_beam_cons in the header), as fairseq's packed tensor or a list of token id lists per
    utterance (unpack_constraints).  The search is then ``batch_mt_beam`` with them, at every beam size.  A forced prefix with
    constraints is refused, and a generator built for sampling raises the reference's own error.

    want_attention: hypothesis 0 also carries what the reference's generator records (agent/sequence_generator.py:383-392, fairseq's
    finalize_hypos): ``"attention"``, float32 [src_len, tgt_len], the head-averaged cross-attention of the last decoder layer --
    column p is the decoder position that predicted token p -- and ``"alignment"``, fairseq's hard alignment, an int tensor
    [tgt_len, 2] of (arg-max source frame, target index) pairs.  Both come from ONE teacher-forced pass over the hypothesis' own
    tokens after the search (engine.batch_mt_attention), on every route; the search itself launches what it launches without the
    switch.  With a forced prefix the prefix columns are those of that pass (the reference's agent generator leaves them
    uninitialised).  Hypotheses 1.. of a beam keep ``None`` in both fields.  The pass rewrites the scratch set's MT cross-attention
    K/V: a single-utterance MT state begun with mt_begin is not live after it."""

    def __init__(self, engine, tgt_dict, beam_size=1, max_len_a=0, max_len_b=200, max_len=0, min_len=1,
                 eos=None, use_incremental_states=False, unk_penalty=0.0, normalize_scores=True, want_attention=False,
                 len_penalty=1.0, temperature=1.0, no_repeat_ngram_size=0, match_source_len=False, sampling=False,
                 sampling_topk=-1, sampling_topp=-1.0, seed=1, **kw):
        from .engine import check_search_options, sampling_from_fairseq
        self.sampling = sampling_from_fairseq(sampling, sampling_topk, sampling_topp, seed)
        self.want_attention = bool(want_attention)
        if match_source_len:
            raise ValueError("match_source_len is not supported: its source length is in encoder frames, which means nothing for "
                             "the text decoder")
        # the reference generator's len_penalty / temperature / no_repeat_ngram_size; any of them off its default sends every search
        # through batch_mt_beam_continue (at beam 1 too, where that call is the greedy continuation bit for bit with the options off)
        self.search = {}
        if check_search_options(len_penalty, temperature, no_repeat_ngram_size) is not None:
            self.search = {"len_penalty": float(len_penalty), "temperature": float(temperature),
                           "no_repeat_ngram_size": int(no_repeat_ngram_size)}
        if not 1 <= int(beam_size) <= 32:
            raise ValueError(f"beam_size {beam_size} outside [1, 32]")
        self.beam_size, self.unk_penalty, self.normalize_scores = int(beam_size), float(unk_penalty), bool(normalize_scores)
        self.engine, self.tgt_dict = engine, tgt_dict
        self.max_len_a, self.max_len_b, self.min_len = max_len_a, max_len_b, min_len
        self.max_len = max_len or engine.cfg.max_target_positions
        self.eos = tgt_dict.eos() if eos is None else eos
        self.pad = tgt_dict.pad()
        self.incremental_states = None
        self.use_incremental_states = use_incremental_states

    def reset_incremental_states(self):
        self.incremental_states = None

    def _attach_attention(self, enc, hyp):
        """The two attention fields of a finished hypothesis: its L tokens end in </s>, the L - 1 before it are fed."""
        toks = [int(t) for t in hyp["tokens"].tolist()]
        attn, peak, _, _, _ = self.engine.batch_mt_attention(enc, [int(enc.shape[0])], [toks[:-1]])[0]
        hyp["attention"] = attn.t().contiguous()
        hyp["alignment"] = torch.stack([peak.to(torch.int64), torch.arange(len(toks), dtype=torch.int64)], 1)

    @torch.no_grad()
    def generate_decoder(self, encoder_outs, src_tokens, src_lengths, sample=None, prefix_tokens=None,
                         constraints=None, bos_token=None, aux_task_name="", encoder_outs_aug=None,
                         max_new_tokens=-1, **kw):
        enc = encoder_outs[0]["encoder_out"][0]
        enc = enc[:, 0] if enc.dim() == 3 else enc
        src_len = src_tokens.size(1)
        prefix = [] if prefix_tokens is None else [int(t) for t in prefix_tokens.view(-1).tolist()]
        start = len(prefix)
        max_len = mt_max_len(start, src_len, max_new_tokens, self.max_len_a, self.max_len_b, self.max_len, self.min_len)
        eng = self.engine
        phrases = unpack_constraints(constraints, 1)[0] if constraints is not None else []
        if constraints is not None and self.sampling is not None:     # Sampling.supports_constraints is False
            raise NotImplementedError("Target-side constraints were provided, but search method doesn't support them")
        if phrases and prefix:
            raise ValueError("constraints behind a forced prefix are not supported: a constraint bans </s> until every phrase is out")
        if self.beam_size > 1 or self.search or self.sampling is not None or phrases:
            enc = enc.contiguous()
            if phrases:
                nbest, f, n = eng.batch_mt_beam(enc, [int(enc.shape[0])], [max_len], self.beam_size, self.min_len, self.unk_penalty,
                                                self.normalize_scores, constraints=[phrases], **self.search)
                feats = [f[0, :n[0]]]
            elif self.sampling is not None:
                key = kw.get("sampling_key")
                if key is None:
                    ids = sample.get("id") if isinstance(sample, dict) else None
                    if torch.is_tensor(ids):
                        ids = int(ids.view(-1)[0]) if ids.numel() else None
                    key = int(ids) if ids is not None else 0
                nbest, feats = eng.batch_mt_sample_continue(enc, [int(enc.shape[0])], [prefix], [max_len], self.beam_size, [int(key)],
                                                            min_len=self.min_len, unk_penalty=self.unk_penalty,
                                                            normalize=self.normalize_scores, **self.sampling.kwargs(), **self.search)
            else:
                nbest, feats = eng.batch_mt_beam_continue(enc, [int(enc.shape[0])], [prefix], [max_len], self.beam_size, self.min_len,
                                                          self.unk_penalty, self.normalize_scores, **self.search)
            hyps = [{"tokens": torch.tensor(h["tokens"], dtype=torch.long), "features": None, "score": h["score"], "attention": None,
                     "alignment": None, "positional_scores": torch.tensor(h["positional_scores"], dtype=torch.float32)}
                    for h in nbest[0]]
            hyps[0]["features"] = feats[0]
            if self.want_attention:
                self._attach_attention(enc, hyps[0])
            return [hyps]
        if hasattr(eng, "mt_greedy"):
            enc = enc.contiguous()
            out, feats = eng.mt_greedy(enc, prefix, max_len, self.min_len)
            hyp = {"tokens": torch.tensor(prefix + out, dtype=torch.long), "features": feats, "score": None,
                   "attention": None, "alignment": None, "positional_scores": None}
            if self.want_attention:
                self._attach_attention(enc, hyp)
            return [[hyp]]
        enc = enc.contiguous()
        eng.mt_begin(enc)
        feats_all = []
        feats, nxt = eng.mt_append([self.eos] + prefix, 0, ban_eos=(start < self.min_len), force_eos=(start >= max_len))
        feats_all.append(feats)
        out = [nxt]
        step = start + 1
        while nxt != self.eos and step <= max_len:
            feats, nxt = eng.mt_append([out[-1]], step, ban_eos=(step < self.min_len), force_eos=(step >= max_len))
            feats_all.append(feats)
            out.append(nxt)
            step += 1
        tokens = torch.tensor(prefix + out, dtype=torch.long)
        # features for positions [eos, prefix..., generated minus the last]: what the reference
        # recomputes via mt_decoder(prev_output_tokens_mt, features_only=True) (agent :638-642)
        hyp = {"tokens": tokens, "features": torch.cat(feats_all, 0), "score": None, "attention": None,
               "alignment": None, "positional_scores": None}
        if self.want_attention:     # after the loop: the single-utterance MT state is no longer needed
            self._attach_attention(enc, hyp)
        return [[hyp]]


class SequenceScorer:
    """fairseq's ``sequence_scorer.SequenceScorer`` (--score-reference) on the first-pass text decoder: how likely the model finds a
    GIVEN target, position by position.  ``SequenceScorer(tgt_dict, engine=...)``; ``generate(models, sample)`` takes
    ``sample["target"]``, a padded int tensor [B, L] whose rows end in </s> (pad is stripped, as fairseq strips it), and the source
    either as ``sample["encoder_out"]`` -- a list of B encoder outputs as the model wrapper's ``encoder`` returns them -- or as
    ``sample["net_input"]`` (``src_tokens`` [B, T, 80], ``src_lengths``), encoded through ``models[0].encoder`` one utterance at a
    time.  -> per sample ``[{"tokens", "score", "attention": None, "alignment": None, "positional_scores"}]``: tokens the target
    without pad, positional_scores float32 [len] in natural log under the plain log_softmax, score their mean with </s> counted.
    The B targets are scored in ONE ragged pass (engine.batch_mt_score).  No ensembles: ``models`` holds one model."""

    def __init__(self, tgt_dict, softmax_batch=None, compute_alignment=False, eos=None, symbols_to_strip_from_output=None,
                 engine=None):
        if engine is None:
            raise ValueError("SequenceScorer needs engine= (anything with HipModel.batch_mt_score)")
        if compute_alignment:
            raise ValueError("compute_alignment is not supported: SequenceGenerator(want_attention=True) gives alignments")
        self.tgt_dict, self.engine = tgt_dict, engine
        self.pad = tgt_dict.pad()
        self.eos = tgt_dict.eos() if eos is None else eos

    @torch.no_grad()
    def generate(self, models, sample, **kw):
        if models is not None and len(models) > 1:
            raise ValueError("ensembles are not supported")
        target = sample["target"]
        B = int(target.size(0))
        rows = []
        for b in range(B):
            t = [int(x) for x in target[b].tolist() if int(x) != self.pad]
            if not t or t[-1] != self.eos:
                raise ValueError(f"target row {b} does not end in </s>")
            rows.append(t)
        if sample.get("encoder_out") is not None:
            eos_ = list(sample["encoder_out"])
        else:
            ni = sample["net_input"]
            src, lens = ni["src_tokens"], ni.get("src_lengths")
            eos_ = [models[0].encoder(src[b:b + 1, :int(lens[b])] if lens is not None else src[b:b + 1]) for b in range(B)]
        if len(eos_) != B:
            raise ValueError("one encoder output per target row")
        encs = []
        for eo in eos_:
            enc = eo["encoder_out"][0]
            encs.append((enc[:, 0] if enc.dim() == 3 else enc).contiguous())
        packed = encs[0] if B == 1 else torch.cat(encs, 0)
        res = self.engine.batch_mt_score(packed, [int(e.shape[0]) for e in encs], [t[:-1] for t in rows])
        return [[{"tokens": torch.tensor(t, dtype=torch.long), "score": r["score"], "attention": None, "alignment": None,
                  "positional_scores": r["positional_scores"]}] for t, r in zip(rows, res)]
