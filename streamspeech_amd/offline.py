"""Offline batch driver with the reference's `fairseq-generate` output format.

Reference flow (researches/ctc_unity/test_scripts/pred.offline-s2st.sh): `fairseq-generate --task
speech_to_speech_ctc ...` prints, per utterance, `A-<id>\\t<asr text>`, `S-<id>\\t<ctc target text>` and
`D-<id>\\t<translation>` into generate-<subset>.log (sequence_generator_multi_decoder_ctc.py:227,248,289)
and `H-/D-/P-<id>` lines with the unit sequence into <results-path>/generate-<subset>.txt
(fairseq_cli/generate.py:257-300); the script then cuts `.asr/.tgt/.unit` files out of those and
runs examples/speech_to_speech/generate_waveform_from_code.py, which writes `<line-no>_pred.wav`.
This driver produces the same files from the HIP path, so the reference's scoring scripts
(sacrebleu / wer / asr_bleu) run unchanged on its output.

Batching mirrors fairseq: utterances are ordered by length (dataset.ordered_indices) and cut into
batches; each batch runs as one ragged no-padding pack through the ss_batch_* entry points (every
utterance keeps its B = 1 arithmetic).  Sharding mirrors `--num-shards/--shard-id`.

The `score` column of H-/D- is the sum of the per-position maximum log-probabilities in the
reference (ctc_generator.py:60-91); the HIP path takes the argmax of the unit logits without forming
log-probabilities, so the column is written as 0 and `P-` lines are omitted unless --scores is
given (then both come from ss_row_max_logprob over the unit logits of the single-utterance entry
point: one more kernel, no torch arithmetic).  The two TEXT CTC heads do form them on request: `--word-times`
runs the scored search (ss_batch_ctc_greedy_scored, the arg-max's log-probability from the same read of the row) and writes
generate-<subset>.asr.words / .st.words, one `id\tword\tstart_ms\tend_ms\tconfidence` line per word (streamspeech_amd/words.py);
every other file is written as without the flag.  `T-` lines (generate.py:258-259) are written when
the manifest carries target units (`tgt_audio` column, as the reference's S2UT manifests do).

`--align-reference` answers the complementary question about the text the recipe ships with every utterance (the multitask
manifests `<data>/<task>/<subset>.tsv`, columns `id` and `tgt_text`, pre-tokenised subwords): where do these words lie in this audio,
and how likely does the model find them.  After the encoder of each batch one forced alignment per text head (ss_batch_ctc_align)
over the rows that have a reference writes generate-<subset>.asr.ref.words / .st.ref.words (the columns of .words) and
generate-<subset>.ref.scores (`id\thead\tn_tokens\tlog_likelihood\tviterbi_score\tstatus`); every other file is written as without it.

`--score-reference` asks the same of the autoregressive first-pass text decoder -- fairseq's `--score-reference` (SequenceScorer):
the reference translation of the `target_unigram` multitask manifest is fed teacher-forced (one batch_mt_score per batch, after
its search and unit pass) and scored position by position under the plain log_softmax.  It writes generate-<subset>.mt.ref.scores
(`id\tn_tokens\tscore\tsum\taccuracy\tstatus`: n_tokens counts </s>; score = sum / n_tokens as SequenceScorer forms it; accuracy =
the share of positions the decoder would have chosen itself) and generate-<subset>.mt.ref.words
(`id\tword\tpieces\tlprob\tconfidence\tmin_lprob\tnot_top`).  Both files are in NATURAL logs (the `H-` / `P-` unit scores of
--scores are base 2, as fairseq-generate prints them).  `--speak-reference` implies it and also speaks the reference: the scored rows' decoder states go through
the unit pass and the vocoder (--speaker-id and --dur-prediction honoured) into generate-<subset>.ref.unit and ref_wav/<n>_pred.wav --
the oracle-text upper bound of the second pass.  Every other file is written as without the flags.

The first-pass text search is greedy by default; `--beam-mt k` runs the reference's beam search (generator_mt with beam_size_mt = k,
`--unkpen`, `--unnormalized`) on the GPU (ss_batch_mt_beam), and `--beam` is accepted for parity (the CTC unit generator has no search).
`--no-repeat-ngram-size` and `--lenpen` are that generator's further controls (ss_batch_mt_beam_opts); either off its default runs the
beam search at `--beam-mt 1` too.  The generator's temperature is the `temperature` argument of generate(); this driver's command
line goes on rejecting `--temperature`, which the recipe does not pass.
`--sampling` (with `--sampling-topk K` or `--sampling-topp P`, and `--seed`) samples instead of searching: `--beam-mt N` is then the
number of independent samples per utterance (ss_batch_mt_sample; the stream key of an utterance is its sample id).  The best-scoring
sample is the D- text and is spoken, as hypothesis 0 of a beam is; generate-<subset>.mt.samples holds all N (id, rank, score, text).
`--constraints [ordered] --constraints-file FILE` is fairseq's lexically constrained beam search (ss_batch_mt_beam_cons): every
phrase the file lists for a sample id stands in its translation, in order; `C-<id>` lines go to the log and
generate-<subset>.mt.constraints reports each phrase (id, phrase, met 0 / 1, token position).  `--constraints unordered` is refused.

Pinned against the reference's own generator classes run on CPU (oracle/ref_offline.py ->
tests/golden/offline_generator.json; tests/test_offline_generator_cpu.py, tests/test_offline_generator_gpu.py).
"""
import argparse
import math
import os
import random
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import frontend
from .pipeline import units_from_tokens
from .words import FRAME_MS, segments_from_spans, spoken_from_segments, words_from_attention, words_from_ctc, words_from_scores


def detok(symbols: Sequence[str]) -> str:
    """sequence_generator_multi_decoder_ctc.py:218-226: join, '_' and the SentencePiece mark become
    spaces, <unk> a space, <s>/</s> vanish, one leading space is dropped."""
    text = "".join(symbols)
    for a, b in (("_", " "), ("▁", " "), ("<unk>", " "), ("<s>", ""), ("</s>", "")):
        text = text.replace(a, b)
    return text[1:] if text.startswith(" ") else text


def ordered_batches(lengths: Sequence[int], batch_size: int, max_tokens: int = 0) -> List[List[int]]:
    """Length-sorted batches (longest first) bounded by `batch_size` utterances and, if > 0, by
    `max_tokens` = batch_count * longest_length (fairseq batch_by_size semantics for speech input)."""
    order = sorted(range(len(lengths)), key=lambda i: (-lengths[i], i))
    out, cur = [], []
    for i in order:
        longest = lengths[cur[0]] if cur else lengths[i]
        if cur and (len(cur) >= batch_size or (max_tokens > 0 and (len(cur) + 1) * longest > max_tokens)):
            out.append(cur)
            cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def generate(model, vocoder, items: Sequence[Tuple[int, torch.Tensor]], dicts: Dict[str, object], results_path: str,
             subset: str = "test", batch_size: int = 32, max_tokens: int = 0, max_len_a: float = 0.0,
             max_len_b: int = 200, max_len_a_mt: float = 0.0, max_len_b_mt: int = 200, dur_prediction: bool = True, dump_wav: bool = True, t2u_causal: bool = False,
             scores: bool = False, log=None, targets: Optional[Dict[int, Sequence[int]]] = None, beam_mt: int = 1,
             unk_penalty: float = 0.0, normalize: bool = True, pcm16_out: bool = False, speaker_id: int = -1,
             features: bool = False, word_times: bool = False, mt_alignment: bool = False, len_penalty: float = 1.0,
             temperature: float = 1.0, no_repeat_ngram_size: int = 0,
             references: Optional[Dict[str, Dict[int, Sequence[int]]]] = None, spoken_words: bool = False,
             mt_references: Optional[Dict[int, Sequence[int]]] = None, speak_reference: bool = False, sampling: bool = False,
             sampling_topk: int = -1, sampling_topp: float = -1.0, seed: int = 1, ctc_beam: int = 0,
             ctc_beam_cand: Optional[int] = None, ctc_nbest: Optional[int] = None,
             constraints: Optional[Dict[int, Sequence[Sequence[int]]]] = None, ctc_lm: Optional[Dict[str, object]] = None,
             ctc_lm_weight: float = 0.5, ctc_word_score: float = 0.0, ctc_bias: Optional[Dict[str, object]] = None,
             ctc_bias_scale: float = 1.0, ctc_keywords: Optional[Dict[str, object]] = None,
             ctc_keyword_max_hits: int = 256) -> Dict[int, Dict]:
    """items: (sample id, 16 kHz float PCM in [-1, 1] on the device).  Writes generate-<subset>.log/.txt,
    the cut .asr/.tgt/.unit files and pred_wav/<n>_pred.wav; returns the per-id hypotheses.
    features=True: the items are (sample id, raw fbank rows [T, 80] float32 on the device) instead -- the recipe's precomputed
    src_fbank80.zip features; the model's global CMVN is applied to the packed rows (ss_batch_cmvn) and src_len is T.
    pcm16_out (--pcm16-io): the waveforms of a batch become 16-bit PCM on the device (one ss_pcm_pack_s16, one download per batch)
    and pred_wav/ is written from those bytes -- the same files, without a float download and a host rounding per utterance.
    speaker_id (--speaker-id; multi-speaker vocoders only): the voice of every utterance; -1 draws one per utterance with
    random.randint(0, num_speakers - 1) like generate_waveform_from_code.py:69-75 and records it in the log (`K-<id>` lines).
    mt_alignment (--mt-alignment): also writes generate-<subset>.mt.words, the words of every `D-` hypothesis placed in source time by
    the text decoder's cross-attention (words.words_from_attention), from one batch_mt_attention per batch after its search; every
    other file is the one written without it.
    len_penalty / temperature / no_repeat_ngram_size (--lenpen, no flag here, --no-repeat-ngram-size): the reference generator's
    controls of the first-pass text search (ss_mt_search_opts); any of them off its default runs the beam search at beam_mt = 1 too.
    sampling / sampling_topk / sampling_topp / seed (--sampling, --sampling-topk, --sampling-topp, --seed; fairseq's names, -1 = off):
    beam_mt independent samples per utterance instead of a search (batch_mt_sample, key = the sample id); the best-scoring one takes
    hypothesis 0's place everywhere, and generate-<subset>.mt.samples lists them all (id, rank, score, text), beam_mt lines per id.
    references (--align-reference): {"asr": {sample id: label ids}, "st": {...}}, the reference text of each head as ids of its
    dictionary.  One batch_ctc_align per head and batch over the rows that have one; writes generate-<subset>.asr.ref.words /
    .st.ref.words and generate-<subset>.ref.scores (a line per sample and head: status aligned / infeasible / nan, or no_reference /
    invalid_label / too_long / no_audio where nothing was aligned) and changes no other file.
    spoken_words (--spoken-words): also writes generate-<subset>.spoken.words, the words of every `D-` hypothesis with the time span
    each is spoken at in its pred_wav (words.spoken_from_segments; a last `</s>` line holds the speech that belongs to no word, if
    any), from ONE batch_unit_spans call per batch over the arg-max ids of its unit pass and the durations of its vocoder call;
    rows without units get no lines; refused without the vocoder call (dump_wav False); every other file is the one written
    without it.
    mt_references (--score-reference): {sample id: the reference translation as ids of target_unigram, without </s>}.  One
    batch_mt_score per batch over the rows with a usable reference, after the batch's search and unit pass (it rewrites the MT
    scratch); writes generate-<subset>.mt.ref.scores (a line per sample: n tokens with </s>, score = sum / n, sum, teacher-forced
    accuracy, status scored / no_reference / invalid_label / too_long / no_audio) and generate-<subset>.mt.ref.words
    (words.words_from_scores), both in natural logs, and changes no other file.
    speak_reference (--speak-reference; needs mt_references): the scored rows' decoder states also go through batch_t2u_units and
    vocoder.batch_forward (speaker_id and dur_prediction as for the hypotheses) into generate-<subset>.ref.unit and
    ref_wav/<n>_pred.wav, laid out as .unit and pred_wav/ are (a line / a number per sample id; a sample without spoken reference has
    an empty line and no file).
    ctc_beam / ctc_beam_cand / ctc_nbest (--ctc-beam K, --ctc-beam-cand C, --ctc-nbest N): one CTC prefix beam search per text head
    after each batch's encoder (batch_ctc_beam: beam K, C candidates per frame -- default engine.ctc_beam_default_cand -- the N <= K
    best, default K); writes generate-<subset>.asr.nbest and .st.nbest (id, rank, score in natural log, n_tokens, text; N rows per
    id in rank order, a slot without hypothesis as score -inf, 0 tokens and no text) and changes no other file: the `A-` / `S-`
    lines stay the arg-max.
    ctc_lm / ctc_lm_weight / ctc_word_score (--ctc-lm-asr FILE, --ctc-lm-st FILE, --ctc-lm-weight A, --ctc-word-score B; with
    ctc_beam): {"asr": an ngram.NgramLM over source_unigram, "st": one over ctc_target_unigram}, either or both -- that head's
    search ranks its hypotheses by log p_ctc + A log p_lm + B n_tokens (batch_ctc_beam(lm=)), `score` in its .nbest file is that
    fused score, and its lines get two more columns behind it, ctc_score and lm_score (natural logs; an empty slot -inf and 0).
    A head without a model, and every other file, is what it is without them.
    ctc_bias / ctc_bias_scale (--ctc-hotwords-asr FILE, --ctc-hotwords-st FILE, --ctc-hotword-boost S; with ctc_beam): {"asr": a
    hotwords.CtcBias over source_unigram, "st": one over ctc_target_unigram}, either or both -- that head's search is biased
    towards the set's phrases (batch_ctc_beam(bias=), with the head's model when it has one), and its .nbest lines are id, rank,
    score, ctc_score, lm_score (0 without a model), bias_score, n_tokens, text.  A head without hotwords, and every other file,
    is what it is without them.
    constraints (--constraints with --constraints-file): {sample id: phrases as ids of target_unigram} -- every hypothesis of that
    sample contains its phrases, in order (fairseq's --constraints, ordered; batch_mt_beam(constraints=), at beam_mt = 1 too).  A
    `C-<id>` line per phrase goes to the log in front of the sample's `D-` line, as fairseq-generate prints them, and
    generate-<subset>.mt.constraints holds a line per phrase: id, phrase, met 0 / 1, the position of its first token in the `D-`
    hypothesis (-1 when not met).  The `D-` text, the units and the waveform follow from the constrained hypothesis; not with
    sampling.
    ctc_keywords (--ctc-keywords-asr FILE, --ctc-keywords-st FILE, --ctc-keyword-threshold T; no ctc_beam needed): {"asr": a
    keywords.CtcKeywords over source_unigram, "st": one over ctc_target_unigram}, either or both -- ONE keyword-spotting call per
    head and batch after the encoder (batch_ctc_spot, at most ctc_keyword_max_hits hits per utterance), and
    generate-<subset>.asr.hits / .st.hits hold a line per occurrence: id, phrase, start_ms, end_ms, score, norm (= score per label;
    times as the .words files place words).  It reads the encoder rows and changes no other file."""
    from .engine import check_search_options, sampling_from_fairseq
    if constraints is not None and sampling:
        raise ValueError("constraints cannot be combined with sampling: the sampling search does not support them")
    met: Dict[int, list] = {}
    nbest_ctc: Dict[str, Dict[int, list]] = {"asr": {}, "st": {}}
    if ctc_beam:
        ctc_nbest = int(ctc_beam) if ctc_nbest is None else int(ctc_nbest)
    ctc_lm = {k: v for k, v in (ctc_lm or {}).items() if v is not None}
    if ctc_lm and not ctc_beam:
        raise ValueError("ctc_lm needs ctc_beam: the model is fused into the CTC prefix beam search")
    ctc_bias = {k: v for k, v in (ctc_bias or {}).items() if v is not None}
    if ctc_bias and not ctc_beam:
        raise ValueError("ctc_bias needs ctc_beam: the hotword set biases the CTC prefix beam search")
    ctc_keywords = {k: v for k, v in (ctc_keywords or {}).items() if v is not None}
    kw_hits: Dict[str, Dict[int, list]] = {"asr": {}, "st": {}}
    sampler = sampling_from_fairseq(sampling, sampling_topk, sampling_topp, seed)
    samples: Dict[int, list] = {}
    if spoken_words and not dump_wav:
        raise ValueError("spoken_words needs the vocoder's durations: it cannot be combined with dump_wav=False (--no-wav)")
    if speak_reference and mt_references is None:
        raise ValueError("speak_reference needs the reference translations (mt_references)")
    search = {}
    if check_search_options(len_penalty, temperature, no_repeat_ngram_size) is not None:
        search = {"len_penalty": float(len_penalty), "temperature": float(temperature),
                  "no_repeat_ngram_size": int(no_repeat_ngram_size)}
    n_spk = int(getattr(vocoder, "num_speakers", 0) or 0)
    if n_spk and not -1 <= speaker_id < n_spk:
        raise ValueError(f"--speaker-id {speaker_id} is outside the vocoder's {n_spk} speakers (-1: a random one per utterance)")
    cfg = model.cfg
    os.makedirs(results_path, exist_ok=True)
    log_f = log or open(os.path.join(results_path, f"generate-{subset}.log"), "w", encoding="utf-8")
    res_f = open(os.path.join(results_path, f"generate-{subset}.txt"), "w", encoding="utf-8")
    hyps: Dict[int, Dict] = {}
    words: Dict[str, Dict[int, list]] = {"asr": {}, "st": {}, "mt": {}}
    spoken: Dict[int, object] = {}
    ref_words: Dict[str, Dict[int, list]] = {"asr": {}, "st": {}}
    ref_scores: Dict[Tuple[int, str], Tuple[int, float, float, str]] = {}
    mt_ref: Dict[int, Dict] = {}
    if features:
        for sid, f in items:
            if f.dim() != 2 or f.shape[1] != 80 or f.dtype != torch.float32:
                raise ValueError(f"sample {sid}: feature items are float32 [T, 80] tensors, not {f.dtype} {tuple(f.shape)}")
    lens = [int(p.shape[0]) if features else int(p.numel()) for _, p in items]
    min_len = 1 if features else 400
    for k, (sid, pcm) in enumerate(items):      # shorter than one 25-ms fbank window: nothing to decode
        if lens[k] < min_len:
            for tag in "ASD":
                print(f"{tag}-{sid}\t", file=log_f)
            print(f"H-{sid}\t0.0\t", file=res_f)
            print(f"D-{sid}\t0.0\t", file=res_f)
            hyps[sid] = {"asr": "", "st": "", "mt": "", "units": [], "wav": None}
    keep = [i for i in range(len(items)) if lens[i] >= min_len]
    for group_k in ordered_batches([lens[i] for i in keep], batch_size, max_tokens):
        group = [keep[j] for j in group_k]
        ids = [items[i][0] for i in group]
        if features:
            T = [lens[i] for i in group]
            feat = model.batch_cmvn(torch.cat([items[i][1] for i in group]).contiguous())
        else:
            pcm = torch.cat([items[i][1].reshape(-1) for i in group])
            feat, T = model.batch_fbank_cmvn(pcm, [lens[i] for i in group])
        enc, Tp = model.batch_encoder_forward(feat, T)
        if word_times:                          # the scored search: the same tokens first in each record, spans and scores behind
            asr = model.batch_ctc_greedy(0, enc, Tp, return_scores=True)
            st = model.batch_ctc_greedy(1, enc, Tp, return_scores=True)
            for b, sid in enumerate(ids):
                for key, rec, name in (("asr", asr[b], "source_unigram"), ("st", st[b], "ctc_target_unigram")):
                    words[key][sid] = words_from_ctc(rec[0], rec[1], rec[2], rec[3], dicts[name], finished=True)
        else:
            asr = model.batch_ctc_greedy(0, enc, Tp)
            st = model.batch_ctc_greedy(1, enc, Tp)
        if references is not None:
            _align_references(model, enc, Tp, ids, references, dicts, ref_words, ref_scores)
        if ctc_beam:
            for hd, key in ((0, "asr"), (1, "st")):
                fuse = {"lm": ctc_lm[key], "lm_weight": ctc_lm_weight, "word_score": ctc_word_score} if key in ctc_lm else {}
                if key in ctc_bias:
                    fuse.update(bias=ctc_bias[key], bias_scale=ctc_bias_scale)
                for sid, lst in zip(ids, model.batch_ctc_beam(hd, enc, Tp, ctc_beam, ctc_beam_cand, ctc_nbest, **fuse)):
                    nbest_ctc[key][sid] = lst
        for hd, key in ((0, "asr"), (1, "st")):
            if key in ctc_keywords:
                for sid, lst in zip(ids, model.batch_ctc_spot(hd, enc, Tp, ctc_keywords[key], ctc_keyword_max_hits)):
                    kw_hits[key][sid] = lst
        # first-pass text search: max_len = min(int(max_len_a_mt * src_len + max_len_b_mt), max positions - 1) with
        # the task's defaults 0 / 200 (tasks/speech_to_speech_ctc.py:39-40 -> sequence_generator_multi_decoder_ctc.py
        # :130-131); src_len is the fbank frame count.  --max-len-a/-b configure the (NAR) unit generator, which has
        # no length search here.
        mx = [min(int(max_len_a_mt * t + max_len_b_mt), cfg.max_target_positions - 1) for t in T]
        if sampler is not None:
            nbest, feats, n = model.batch_mt_sample(enc, Tp, mx, beam_mt, [int(i) for i in ids], min_len=1, unk_penalty=unk_penalty,
                                                    normalize=normalize, **sampler.kwargs(), **search)
            toks = [h[0]["tokens"] if h else [] for h in nbest]
            for b, sid in enumerate(ids):
                samples[sid] = [(h["score"], detok([dicts["target_unigram"][c] for c in h["tokens"] if c != cfg.eos])) for h in nbest[b]]
        elif constraints is not None:
            nbest, feats, n = model.batch_mt_beam(enc, Tp, mx, beam_mt, 1, unk_penalty, normalize,
                                                  constraints=[constraints.get(sid) or [] for sid in ids], **search)
            toks = [h[0]["tokens"] if h else [] for h in nbest]
        elif beam_mt > 1 or search:
            # --beam-mt k: the reference's beam search (generator_mt with beam_size_mt = k, --unkpen, --unnormalized); the D- text
            # and the T2U input are hypothesis 0 of each n-best list (sequence_generator_multi_decoder_ctc.py:265-300)
            nbest, feats, n = model.batch_mt_beam(enc, Tp, mx, beam_mt, 1, unk_penalty, normalize, **search)
            toks = [h[0]["tokens"] if h else [] for h in nbest]
        else:
            toks, feats, n = model.batch_mt_greedy(enc, Tp, mx)
        if spoken_words:
            unit_toks, raw_dev = model.batch_t2u_units(feats, n, t2u_causal=t2u_causal, mask_eos=True, keep_raw=True)
        else:
            unit_toks = model.batch_t2u_units(feats, n, t2u_causal=t2u_causal, mask_eos=True)
        codes = [units_from_tokens(t, cfg) for t in unit_toks]
        if mt_alignment:                        # after the search and the unit pass: nothing of this batch reads the MT scratch any more
            mts = [[t for t in toks[b] if t != cfg.eos] for b in range(len(ids))]
            rows = [b for b in range(len(ids)) if mts[b]]
            off = [0]
            for t in Tp:
                off.append(off[-1] + int(t))
            if rows:
                enc_r = enc if len(rows) == len(ids) else torch.cat([enc[off[b]:off[b + 1]] for b in rows], 0)
                att = model.batch_mt_attention(enc_r, [Tp[b] for b in rows], [mts[b][:-1] for b in rows], want_matrix=False)
                for b, (_, peak, prob, _, _) in zip(rows, att):
                    words["mt"][ids[b]] = words_from_attention(mts[b], peak.tolist(), prob.tolist(), dicts["target_unigram"],
                                                               eos=cfg.eos)
        if mt_references is not None:           # here for the same reason: the pass rewrites the MT scratch of this batch
            _score_references(model, vocoder, enc, Tp, ids, mt_references, dicts, mt_ref, speak_reference, t2u_causal, dur_prediction,
                              n_spk, speaker_id)
        have = [b for b, c in enumerate(codes) if len(c) > 0]
        wavs: Dict[int, torch.Tensor] = {}
        if dump_wav and have:
            spk = {}
            if n_spk:                           # one pack, a voice per row
                spk["speakers"] = [speaker_id if speaker_id >= 0 else random.randint(0, n_spk - 1) for _ in have]
                for b, k in zip(have, spk["speakers"]):
                    print(f"K-{ids[b]}\t{k}", file=log_f)
            w, dur_dev, _ = vocoder.batch_forward([codes[b] for b in have], dur_prediction=dur_prediction, **spk)
            wavs = {b: w[j] for j, b in enumerate(have)}
            if spoken_words:                    # one spans call per batch: the unit pass's ids and the vocoder call's durations, where they lie
                up, off = cfg.ctc_upsample, [0]
                for x in n:
                    off.append(off[-1] + int(x))
                raw_h = raw_dev if len(have) == len(ids) else torch.cat([raw_dev[off[b] * up: off[b + 1] * up] for b in have], 0)
                spans = model.batch_unit_spans(raw_h, [n[b] for b in have], [len(codes[b]) for b in have], dur_dev)
                for b, sp in zip(have, spans):
                    spoken[ids[b]] = spoken_from_segments(toks[b], segments_from_spans(sp, 0), dicts["target_unigram"], eos=cfg.eos)
            if pcm16_out:
                pcm16 = _pack_batch(model, [wavs[b] for b in have])
                pcm16 = {b: pcm16[j] for j, b in enumerate(have)}
        for b, sid in enumerate(ids):
            a_txt = detok([dicts["source_unigram"][c] for c in asr[b][0]])
            s_txt = detok([dicts["ctc_target_unigram"][c] for c in st[b][0]])
            mt = [t for t in toks[b] if t != cfg.eos]
            d_txt = detok([dicts["target_unigram"][c] for c in mt])
            print(f"A-{sid}\t{a_txt}", file=log_f)
            print(f"S-{sid}\t{s_txt}", file=log_f)
            if constraints is not None:
                met[sid] = []
                for p, at in zip(constraints.get(sid) or [], phrase_positions(mt, constraints.get(sid) or [])):
                    p_txt = detok([dicts["target_unigram"][c] for c in p])
                    print(f"C-{sid}\t{p_txt}", file=log_f)
                    met[sid].append((p_txt, at))
            print(f"D-{sid}\t{d_txt}", file=log_f)
            unit_str = " ".join(str(u) for u in codes[b])
            score, pos = 0.0, None
            if scores:
                score, pos = _unit_scores(model, feats[b][: n[b]], t2u_causal)
            if targets is not None and sid in targets:
                print(f"T-{sid}\t" + " ".join(str(u) for u in targets[sid]), file=res_f)
            print(f"H-{sid}\t{score}\t{unit_str}", file=res_f)
            print(f"D-{sid}\t{score}\t{unit_str}", file=res_f)
            if pos is not None:
                print(f"P-{sid}\t" + " ".join("{:.4f}".format(x) for x in pos), file=res_f)
            hyps[sid] = {"asr": a_txt, "st": s_txt, "mt": d_txt, "units": codes[b], "wav": wavs.get(b)}
            if spoken_words:
                hyps[sid]["spoken"] = spoken.get(sid)
            if pcm16_out and dump_wav and have:
                hyps[sid]["pcm16"] = pcm16.get(b)
    res_f.close()
    if log is None:
        log_f.close()
    _cut_files(hyps, results_path, subset, dump_wav)
    if word_times:
        for key in ("asr", "st"):
            with open(os.path.join(results_path, f"generate-{subset}.{key}.words"), "w", encoding="utf-8") as f:
                for sid in sorted(words[key]):
                    for w in words[key][sid]:
                        print(f"{sid}\t{w.text}\t{w.start_ms}\t{w.end_ms}\t{w.confidence:.6g}", file=f)
    if references is not None:
        for key in ("asr", "st"):
            with open(os.path.join(results_path, f"generate-{subset}.{key}.ref.words"), "w", encoding="utf-8") as f:
                for sid in sorted(ref_words[key]):
                    for w in ref_words[key][sid]:
                        print(f"{sid}\t{w.text}\t{w.start_ms}\t{w.end_ms}\t{w.confidence:.6g}", file=f)
        with open(os.path.join(results_path, f"generate-{subset}.ref.scores"), "w", encoding="utf-8") as f:
            for sid, _ in items:
                for key in ("asr", "st"):
                    ref = references.get(key, {}).get(sid)
                    n, score, vit, status = ref_scores.get((sid, key), (0 if ref is None else len(ref), float("nan"), float("nan"),
                                                                       "no_reference" if ref is None else "no_audio"))
                    print(f"{sid}\t{key}\t{n}\t{score:.6f}\t{vit:.6f}\t{status}", file=f)
    if ctc_beam:
        for key, name in (("asr", "source_unigram"), ("st", "ctc_target_unigram")):
            with open(os.path.join(results_path, f"generate-{subset}.{key}.nbest"), "w", encoding="utf-8") as f:
                for sid in sorted(hyps):
                    lst = nbest_ctc[key].get(sid, [])
                    for rank in range(ctc_nbest):
                        if rank < len(lst):
                            text = detok([dicts[name][c] for c in lst[rank].tokens])
                            more = f"\t{lst[rank].ctc_score:.6f}\t{lst[rank].lm_score:.6f}" if key in ctc_lm else ""
                            if key in ctc_bias:
                                more = f"\t{lst[rank].ctc_score:.6f}\t{lst[rank].lm_score or 0.0:.6f}\t{lst[rank].bias_score:.6f}"
                            print(f"{sid}\t{rank}\t{lst[rank].score:.6f}{more}\t{len(lst[rank].tokens)}\t{text}", file=f)
                        else:
                            more = "\t-inf\t0\t0" if key in ctc_bias else "\t-inf\t0" if key in ctc_lm else ""
                            print(f"{sid}\t{rank}\t-inf{more}\t0\t", file=f)
    for key in ("asr", "st"):
        if key in ctc_keywords:
            with open(os.path.join(results_path, f"generate-{subset}.{key}.hits"), "w", encoding="utf-8") as f:
                for sid in sorted(kw_hits[key]):
                    for h in kw_hits[key][sid]:
                        print(f"{sid}\t{ctc_keywords[key].texts[h.keyword]}\t{h.start * FRAME_MS}\t{(h.end + 1) * FRAME_MS}\t"
                              f"{h.score:.6f}\t{h.norm:.6f}", file=f)
    if spoken_words:
        with open(os.path.join(results_path, f"generate-{subset}.spoken.words"), "w", encoding="utf-8") as f:
            for sid in sorted(spoken):
                for w in spoken[sid].words:
                    print(f"{sid}\t{w.text}\t{w.start_ms}\t{w.end_ms}\t{w.n_units}", file=f)
                if spoken[sid].tail_ms > 0:
                    t = spoken[sid]
                    print(f"{sid}\t</s>\t{t.total_ms - t.tail_ms}\t{t.total_ms}\t0", file=f)
    if sampler is not None:
        with open(os.path.join(results_path, f"generate-{subset}.mt.samples"), "w", encoding="utf-8") as f:
            for sid in sorted(samples):
                for rank, (score, text) in enumerate(samples[sid]):
                    print(f"{sid}\t{rank}\t{score:.6f}\t{text}", file=f)
    if constraints is not None:
        with open(os.path.join(results_path, f"generate-{subset}.mt.constraints"), "w", encoding="utf-8") as f:
            for sid in sorted(met):
                for p_txt, at in met[sid]:
                    print(f"{sid}\t{p_txt}\t{0 if at is None else 1}\t{-1 if at is None else at}", file=f)
    if mt_alignment:
        with open(os.path.join(results_path, f"generate-{subset}.mt.words"), "w", encoding="utf-8") as f:
            for sid in sorted(words["mt"]):
                for w in words["mt"][sid]:
                    print(f"{sid}\t{w.text}\t{w.start_ms}\t{w.end_ms}\t{w.focus:.6g}", file=f)
    if mt_references is not None:
        nan = float("nan")
        with open(os.path.join(results_path, f"generate-{subset}.mt.ref.scores"), "w", encoding="utf-8") as f:
            for sid, _ in items:
                ref = mt_references.get(sid)
                r = mt_ref.get(sid) or {"n": 0 if ref is None else len(ref) + 1, "score": nan, "sum": nan, "accuracy": nan,
                                        "status": "no_reference" if ref is None else "no_audio"}
                print(f"{sid}\t{r['n']}\t{r['score']:.6f}\t{r['sum']:.6f}\t{r['accuracy']:.6f}\t{r['status']}", file=f)
        with open(os.path.join(results_path, f"generate-{subset}.mt.ref.words"), "w", encoding="utf-8") as f:
            for sid in sorted(mt_ref):
                for w in mt_ref[sid].get("words", ()):
                    print(f"{sid}\t{w.text}\t{w.pieces}\t{w.lprob:.6f}\t{w.confidence:.6g}\t{w.min_lprob:.6f}\t{w.not_top}", file=f)
        if speak_reference:
            ids_all = sorted(hyps)              # the lines of .unit and the numbers of pred_wav/ (_cut_files)
            with open(os.path.join(results_path, f"generate-{subset}.ref.unit"), "w", encoding="utf-8") as f:
                for i in ids_all:
                    print(" ".join(str(u) for u in mt_ref.get(i, {}).get("units", ())), file=f)
            wdir = os.path.join(results_path, "ref_wav")
            os.makedirs(wdir, exist_ok=True)
            for k, i in enumerate(ids_all):
                w = mt_ref.get(i, {}).get("wav")
                if w is not None:
                    frontend.write_wav(os.path.join(wdir, f"{k}_pred.wav"), w.detach().cpu().numpy(), 16000)
    return hyps


ALIGN_STATUS = ("aligned", "infeasible", "nan")


def _align_references(model, enc, Tp, ids, references, dicts, ref_words, ref_scores):
    """One batch_ctc_align per text head over the rows of this batch that have a usable reference.  A reference the library would
    refuse the whole call for (a blank, pad or out-of-vocabulary id; more labels than its limit) is recorded and left out."""
    from .lib import CTC_ALIGN_MAX_FRAMES, CTC_ALIGN_MAX_LABELS
    off = [0]
    for t in Tp:
        off.append(off[-1] + int(t))
    nan = float("nan")
    for head, (key, name) in enumerate((("asr", "source_unigram"), ("st", "ctc_target_unigram"))):
        refs = references.get(key, {})
        V, pad = (model.cfg.src_vocab, model.cfg.tgt_vocab)[head], model.cfg.pad      # the library's own refusals
        rows = []
        for b, sid in enumerate(ids):
            if sid not in refs:
                continue
            y = [int(v) for v in refs[sid]]
            if any(v <= 0 or v == pad or v >= V for v in y):
                ref_scores[(sid, key)] = (len(y), nan, nan, "invalid_label")
            elif len(y) > CTC_ALIGN_MAX_LABELS or int(Tp[b]) > CTC_ALIGN_MAX_FRAMES:
                ref_scores[(sid, key)] = (len(y), nan, nan, "too_long")
            else:
                rows.append((b, y))
        if not rows:
            continue
        enc_r = enc if len(rows) == len(ids) else torch.cat([enc[off[b]:off[b + 1]] for b, _ in rows], 0).contiguous()
        got = model.batch_ctc_align(head, enc_r, [Tp[b] for b, _ in rows], [y for _, y in rows], want_path=False)
        for (b, y), a in zip(rows, got):
            ref_scores[(ids[b], key)] = (len(y), a.score, a.viterbi_score, ALIGN_STATUS[a.status])
            if a.status == 0:
                ref_words[key][ids[b]] = words_from_ctc(y, a.first, a.last, a.tok_lprob, dicts[name], finished=True)


def _score_references(model, vocoder, enc, Tp, ids, mt_references, dicts, mt_ref, speak, t2u_causal, dur_prediction, n_spk,
                      speaker_id):
    """One batch_mt_score over the rows of this batch that have a usable reference translation; with `speak` their decoder states go
    on through the unit pass and the vocoder.  A reference the library would refuse the whole call for (an id outside the
    dictionary, <pad>; more positions than the decoder has) is recorded and left out."""
    cfg = model.cfg
    nan = float("nan")
    max_pos = int(getattr(model, "max_tgt_pos", cfg.max_target_positions + 2))
    off = [0]
    for t in Tp:
        off.append(off[-1] + int(t))
    rows = []
    for b, sid in enumerate(ids):
        if sid not in mt_references:
            continue
        y = [int(v) for v in mt_references[sid]]
        bad = {"n": len(y) + 1, "score": nan, "sum": nan, "accuracy": nan}
        if any(v < 0 or v >= cfg.tgt_vocab or v == cfg.pad for v in y):
            mt_ref[sid] = dict(bad, status="invalid_label")
        elif len(y) + 3 > max_pos:              # the library's position bound: 1 + n fed positions + 2
            mt_ref[sid] = dict(bad, status="too_long")
        else:
            rows.append((b, y))
    if not rows:
        return
    enc_r = enc if len(rows) == len(ids) else torch.cat([enc[off[b]:off[b + 1]] for b, _ in rows], 0).contiguous()
    got = model.batch_mt_score(enc_r, [Tp[b] for b, _ in rows], [y for _, y in rows], want_feats=speak)
    for (b, y), r in zip(rows, got):
        pos, rank = r["positional_scores"].tolist(), r["rank"].tolist()
        total = math.fsum(pos)
        mt_ref[ids[b]] = {"n": len(pos), "score": total / len(pos), "sum": total,
                          "accuracy": sum(1 for k in rank if k == 0) / len(rank), "status": "scored",
                          "words": words_from_scores(y + [cfg.eos], pos, rank, dicts["target_unigram"], eos=cfg.eos)}
    if not speak:
        return
    n = [len(y) + 1 for _, y in rows]
    feats = torch.nn.utils.rnn.pad_sequence([r["feats"] for r in got], batch_first=True).contiguous()
    codes = [units_from_tokens(t, cfg) for t in model.batch_t2u_units(feats, n, t2u_causal=t2u_causal, mask_eos=True)]
    for (b, _), c in zip(rows, codes):
        mt_ref[ids[b]]["units"] = c
    have = [j for j, c in enumerate(codes) if len(c) > 0]
    if not have:
        return
    spk = {}
    if n_spk:                                   # -1: a voice per sample from a generator of its own, seeded by the sample id -- the
        spk["speakers"] = [speaker_id if speaker_id >= 0 else random.Random(ids[rows[j][0]]).randint(0, n_spk - 1)
                           for j in have]       # hypotheses' draws (and so pred_wav/ and the log) stay what they are without the flag
    w, _, _ = vocoder.batch_forward([codes[j] for j in have], dur_prediction=dur_prediction, **spk)
    for k, j in enumerate(have):
        mt_ref[ids[rows[j][0]]]["wav"] = w[k]


def multitask_text_dir(data_root: str, multitask_yaml: Optional[str], task: str) -> Optional[str]:
    """The directory of a multitask task's text manifests: the `data:` entry of the task in the multitask YAML, or, where that path
    does not exist here, `<data_root>/<its last component>` (as load_dictionaries resolves `dict:`).  None: the YAML names none."""
    import yaml
    from pathlib import Path
    if multitask_yaml is None:
        return None
    mpath = multitask_yaml if os.path.isabs(multitask_yaml) else os.path.join(data_root, multitask_yaml)
    if not os.path.exists(mpath):
        return None
    with open(mpath) as f:
        cfg = yaml.load(f, Loader=yaml.BaseLoader) or {}
    path = (cfg.get(task) or {}).get("data")
    if not path:
        return None
    if not os.path.isdir(path):
        path = os.path.join(data_root, Path(path).parts[-1])
    return path


def load_multitask_text(directory: str, subset: str) -> Dict[str, List[str]]:
    """`<directory>/<subset>.tsv` of a multitask task (fairseq TextTargetMultitaskData: columns `id` and `tgt_text`, read as the
    recipe's manifests are -- tab-separated, no quoting) -> {id: the pre-tokenised subwords of tgt_text}."""
    import csv
    out = {}
    with open(os.path.join(directory, subset + ".tsv"), encoding="utf-8", newline="") as f:
        for row in csv.DictReader(f, delimiter="\t", quotechar=None, doublequote=False, lineterminator="\n", quoting=csv.QUOTE_NONE):
            out[row["id"]] = (row["tgt_text"] or "").split()
    return out


def load_manifest_ids(path: str) -> Dict[int, str]:
    """{row index (the sample id load_manifest gives): the row's `id` cell} of a manifest."""
    out = {}
    with open(path, encoding="utf-8") as f:
        header = f.readline().rstrip("\n").split("\t")
        col = header.index("id")
        for i, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) > col:
                out[i] = parts[col]
    return out


def load_references(data_root: str, multitask_yaml: Optional[str], subset: str, dicts) -> Optional[Dict[str, Dict[int, List[int]]]]:
    """--align-reference: the reference label ids of both text heads per sample id, from the multitask manifests of `source_unigram`
    and `ctc_target_unigram` joined with the manifest's `id` column; a piece the dictionary does not hold becomes <unk>.  None when
    the YAML names no data directory for either task."""
    dirs = {key: multitask_text_dir(data_root, multitask_yaml, name)
            for key, name in (("asr", "source_unigram"), ("st", "ctc_target_unigram"))}
    if not any(dirs.values()):
        return None
    names = load_manifest_ids(os.path.join(data_root, subset + ".tsv"))
    out: Dict[str, Dict[int, List[int]]] = {"asr": {}, "st": {}}
    for key, name in (("asr", "source_unigram"), ("st", "ctc_target_unigram")):
        if dirs[key] is None:
            continue
        text = load_multitask_text(dirs[key], subset)
        out[key] = {i: [dicts[name].index(p) for p in text[n]] for i, n in names.items() if n in text}
    return out


def load_mt_references(data_root: str, multitask_yaml: Optional[str], subset: str, dicts) -> Optional[Dict[int, List[int]]]:
    """--score-reference: the reference translation per sample id as ids of `target_unigram` (without </s>), from that task's
    multitask manifest joined with the manifest's `id` column; a piece the dictionary does not hold becomes <unk>.  None when the
    YAML names no data directory for the task."""
    directory = multitask_text_dir(data_root, multitask_yaml, "target_unigram")
    if directory is None:
        return None
    names = load_manifest_ids(os.path.join(data_root, subset + ".tsv"))
    text = load_multitask_text(directory, subset)
    return {i: [dicts["target_unigram"].index(p) for p in text[n]] for i, n in names.items() if n in text}


def phrase_positions(tokens: Sequence[int], phrases: Sequence[Sequence[int]]) -> List[Optional[int]]:
    """Where each phrase starts in tokens, the phrases matched left to right one after the other; None from the first that is
    missing."""
    tokens, out, start = [int(t) for t in tokens], [], 0
    for p in phrases:
        p = [int(t) for t in p]
        hit = next((i for i in range(start, len(tokens) - len(p) + 1) if tokens[i:i + len(p)] == p), None)
        if hit is None:
            break
        out.append(hit)
        start = hit + len(p)
    return out + [None] * (len(phrases) - len(out))


def parse_constraints_file(lines, dictionary) -> Dict[int, List[List[int]]]:
    """--constraints-file: lines `id<TAB>phrase<TAB>phrase...`, a phrase being the space-separated pieces of the target dictionary
    (as the multitask manifests spell the reference text) -> {sample id: phrases as ids}.  Blank lines are skipped; an id may stand
    on several lines.  An id that is no integer, an empty phrase, or a piece the dictionary does not hold is a ValueError naming the
    id."""
    out: Dict[int, List[List[int]]] = {}
    unk, index = dictionary.unk(), {}
    for i in range(len(dictionary)):
        index.setdefault(dictionary[i], i)
    for ln in lines:
        ln = ln.rstrip("\r\n")
        if not ln.strip():
            continue
        cells = ln.split("\t")
        try:
            sid = int(cells[0])
        except ValueError:
            raise ValueError(f"constraints file: {cells[0]!r} is not a sample id") from None
        for cell in cells[1:]:
            pieces = cell.split()
            if not pieces:
                raise ValueError(f"constraints file, id {sid}: an empty phrase")
            ids = [index.get(p, unk) for p in pieces]
            bad = [p for p, i in zip(pieces, ids) if i == unk]
            if bad:
                raise ValueError(f"constraints file, id {sid}: {bad[0]!r} is not in the target dictionary")
            out.setdefault(sid, []).append(ids)
    return out


def _pack_batch(model, wavs: List[torch.Tensor]):
    """The waveforms of one batch -> int16 NumPy arrays: one ss_pcm_pack_s16 launch over all of them, one download."""
    n = [int(w.numel()) for w in wavs]
    src = torch.cat([w.reshape(-1) for w in wavs], 0)
    out = torch.empty((max(sum(n), 1),), dtype=torch.int16, device=src.device)
    if sum(n):
        model.pcm_pack_s16(src, out[:sum(n)])
    host = out[:sum(n)].cpu().numpy()
    res, off = [], 0
    for k in n:
        res.append(host[off:off + k])
        off += k
    return res


def stage_wavs_pcm16(model, raws, device):
    """--pcm16-io: [(raw 16-bit frames, channels, sample rate, frames)] -> [(float32 mono tensor on the device, sample rate)], read_wav's
    bits.  The raw bytes of all files go into one pinned arena, are uploaded ONCE and decoded by ONE ss_pcm_scatter launch into one
    packed float32 buffer, of which the results are views."""
    from .pcm import SS_PCM_S16LE, PcmArena
    arena = PcmArena(device, capacity=sum(len(r[0]) for r in raws) + 16 * len(raws) + 16)
    segs, at = [], 0
    for raw, nch, _, n in raws:
        segs.append((arena.add(raw), at, n, SS_PCM_S16LE, nch, 0))
        at += n
    packed = torch.empty((max(at, 1),), dtype=torch.float32, device=device)
    stage, nbytes = arena.upload()
    if nbytes:
        model.pcm_scatter(stage, nbytes, segs, [packed])
    arena.clear()                                 # waits for the upload: the arena goes away with this call
    out, at = [], 0
    for _, _, sr, n in raws:
        out.append((packed[at:at + n], sr))
        at += n
    return out


def _unit_scores(model, feats: torch.Tensor, t2u_causal: bool):
    """Sum / per-position max log-probabilities in base 2 (generate.py:274,289), pad / unk / eos masked as in
    ctc_generator.py:55-59.  The log-softmax + max runs in the engine (HIP: ss_row_max_logprob); the base change and the
    sum (a float64 host sum like `scores[b].sum()` -> utils.item) are glue."""
    best = model.unit_scores(feats.contiguous(), t2u_causal=t2u_causal).double() / math.log(2)
    return float(best.sum()), best.tolist()


def _cut_files(hyps: Dict[int, Dict], results_path: str, subset: str, dump_wav: bool):
    """What pred.offline-s2st.sh greps/sorts/cuts out of the two generate files, and the wav dump of
    generate_waveform_from_code.py (file name = line number in the sorted .unit file)."""
    ids = sorted(hyps)
    for ext, key in ((".asr", "asr"), (".tgt", "mt")):
        with open(os.path.join(results_path, f"generate-{subset}{ext}"), "w", encoding="utf-8") as f:
            for i in ids:
                print(hyps[i][key], file=f)
    with open(os.path.join(results_path, f"generate-{subset}.unit"), "w", encoding="utf-8") as f:
        for i in ids:
            print(" ".join(str(u) for u in hyps[i]["units"]), file=f)
    if dump_wav:
        wdir = os.path.join(results_path, "pred_wav")
        os.makedirs(wdir, exist_ok=True)
        for n, i in enumerate(ids):
            w = hyps[i]["wav"]
            if hyps[i].get("pcm16") is not None:
                frontend.write_wav_pcm16(os.path.join(wdir, f"{n}_pred.wav"), hyps[i]["pcm16"], 16000)
            elif w is not None:
                frontend.write_wav(os.path.join(wdir, f"{n}_pred.wav"), w.detach().cpu().numpy(), 16000)


def load_manifest(path: str, targets: Optional[Dict[int, List[int]]] = None) -> List[Tuple[int, str]]:
    """fairseq S2T/S2S manifest (TSV with header, columns `id` and `audio` = src_audio): one cell per row -- a WAV, FLAC, MP3 or .npy
    path, or `<zip>:<offset>:<length>` into a stored zip of such members (frontend.parse_audio_cell).
    The sample id fairseq prints is the row index.  With `targets` given, the target units of the `tgt_audio` column
    (space-separated ids, SpeechToSpeechDataset: fairseq/data/audio/speech_to_speech_dataset.py) are collected per id."""
    rows = []
    with open(path, encoding="utf-8") as f:
        header = f.readline().rstrip("\n").split("\t")
        col = header.index("src_audio") if "src_audio" in header else header.index("audio")
        tcol = header.index("tgt_audio") if "tgt_audio" in header else -1
        for i, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) > col and parts[col]:
                rows.append((i, parts[col]))
                if targets is not None and 0 <= tcol < len(parts):
                    try:
                        targets[i] = [int(u) for u in parts[tcol].split()]
                    except ValueError:      # a wav path, not units (S2ST with spectrogram targets)
                        pass
    return rows


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("data", nargs="?", default=None, help="data root holding <gen-subset>.tsv and the config yamls")
    ap.add_argument("--gen-subset", default="test")
    ap.add_argument("--path", required=True, help="checkpoint (.pt) or synthetic:<seed>")
    ap.add_argument("--vocoder", required=True)
    ap.add_argument("--vocoder-cfg", default=None)
    ap.add_argument("--config-yaml", default=None)
    ap.add_argument("--multitask-config-yaml", default=None)
    ap.add_argument("--results-path", required=True)
    ap.add_argument("--wav-list", default=None, help="text file with one WAV / FLAC / MP3 path per line (instead of a manifest)")
    ap.add_argument("--synthetic", type=int, default=0, help="N synthetic utterances instead of files")
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--max-tokens", type=int, default=0)
    ap.add_argument("--max-len-a", type=float, default=0.0, help="unit generator (kept for CLI parity; the NAR decoder has no length search)")
    ap.add_argument("--max-len-b", type=int, default=200)
    ap.add_argument("--max-len-a-mt", type=float, default=0.0, help="first-pass text search: max_len = a * src_len + b")
    ap.add_argument("--max-len-b-mt", type=int, default=200)
    ap.add_argument("--dur-prediction", action="store_true")
    ap.add_argument("--vocoder-fp16", action="store_true",
                    help="run the vocoder's 64- to 256-channel ResBlock convs on FP16 matrix cores (f32 accumulation; waveform within "
                         "1e-3 RMS, unit ids and durations unchanged); default: exact f32")
    ap.add_argument("--speaker-id", type=int, default=-1,
                    help="multi-speaker vocoders: the voice of every utterance; -1 (default, as generate_waveform_from_code.py) draws "
                         "a random speaker per utterance and logs it; ignored by a single-speaker vocoder")
    ap.add_argument("--no-wav", action="store_true")
    ap.add_argument("--scores", action="store_true")
    ap.add_argument("--word-times", action="store_true",
                    help="also write generate-<subset>.asr.words and .st.words: id, word, start_ms, end_ms, confidence per word of the two CTC heads")
    ap.add_argument("--mt-alignment", action="store_true",
                    help="also write generate-<subset>.mt.words: id, word, start_ms, end_ms, focus per word of the D- hypothesis, placed in "
                         "source time by the arg-max of the text decoder's cross-attention (one extra decoder pass per batch)")
    ap.add_argument("--spoken-words", action="store_true",
                    help="also write generate-<subset>.spoken.words: id, word, start_ms, end_ms, n_units per word of the D- hypothesis, "
                         "the time span it is spoken at in the utterance's pred_wav (exact: from the unit decoder's arg-max and the "
                         "predicted durations; one small extra launch per batch), plus an `</s>` line for speech that belongs to no "
                         "word; not with --no-wav")
    ap.add_argument("--align-reference", action="store_true",
                    help="also align the recipe's reference text (the multitask manifests <task data>/<gen-subset>.tsv of source_unigram "
                         "and ctc_target_unigram) to the audio on both CTC heads: writes generate-<subset>.asr.ref.words / .st.ref.words "
                         "(id, word, start_ms, end_ms, confidence) and generate-<subset>.ref.scores (id, head, n_tokens, log_likelihood, "
                         "viterbi_score, status); needs a manifest")
    ap.add_argument("--ctc-beam", type=int, default=0,
                    help="also run a CTC prefix beam search of this beam (1 .. 32) on both CTC heads: writes generate-<subset>.asr.nbest "
                         "and .st.nbest (id, rank, score, n_tokens, text), the most likely texts summed over their alignments; the "
                         "A- / S- lines stay the arg-max (0 = off)")
    ap.add_argument("--ctc-beam-cand", type=int, default=None,
                    help="with --ctc-beam: tokens a prefix is extended by per frame (1 .. 32; default beam + 1, at most 32)")
    ap.add_argument("--ctc-nbest", type=int, default=None, help="with --ctc-beam: hypotheses written per id (1 .. beam; default the beam)")
    ap.add_argument("--ctc-lm-asr", default=None, metavar="FILE",
                    help="with --ctc-beam: an ARPA n-gram model (.arpa / .arpa.gz) over source_unigram, fused into the ASR head's search: "
                         "its .nbest lines are ranked by log p_ctc + A log p_lm + B n_tokens and get the columns ctc_score and lm_score "
                         "after score")
    ap.add_argument("--ctc-lm-st", default=None, metavar="FILE",
                    help="the same for the ST head, a model over ctc_target_unigram")
    ap.add_argument("--ctc-lm-weight", type=float, default=0.5, help="A, the weight of the n-gram model's log-probability (default 0.5)")
    ap.add_argument("--ctc-word-score", type=float, default=0.0, help="B, added per token of a hypothesis (default 0)")
    ap.add_argument("--ctc-hotwords-asr", default=None, metavar="FILE",
                    help="with --ctc-beam: bias the ASR head's search towards the phrases of FILE -- one per line as space-separated "
                         "pieces of source_unigram, optionally a tab and the phrase's per-token boost; its .nbest lines become id, "
                         "rank, score, ctc_score, lm_score, bias_score, n_tokens, text")
    ap.add_argument("--ctc-hotwords-st", default=None, metavar="FILE",
                    help="the same for the ST head, phrases over ctc_target_unigram")
    ap.add_argument("--ctc-hotword-boost", type=float, default=1.5,
                    help="S, the per-token boost (natural-log units) of a hotword line that names none (default 1.5)")
    ap.add_argument("--ctc-keywords-asr", default=None, metavar="FILE",
                    help="spot the phrases of FILE on the ASR head -- one per line as space-separated pieces of source_unigram, optionally "
                         "a tab and the phrase's threshold; writes generate-<subset>.asr.hits (id, phrase, start_ms, end_ms, score, norm); "
                         "needs no --ctc-beam, every other file as without the flag")
    ap.add_argument("--ctc-keywords-st", default=None, metavar="FILE",
                    help="the same for the ST head, phrases over ctc_target_unigram: generate-<subset>.st.hits")
    ap.add_argument("--ctc-keyword-threshold", type=float, default=1.0,
                    help="T, the threshold (natural-log units per label) of a keyword line that names none (default 1.0: a starting "
                         "point, not tuned on a trained checkpoint)")
    ap.add_argument("--score-reference", action="store_true",
                    help="also score the recipe's reference translation (the multitask manifest <task data>/<gen-subset>.tsv of "
                         "target_unigram) with the first-pass text decoder, teacher-forced, as fairseq's --score-reference does: writes "
                         "generate-<subset>.mt.ref.scores (id, n_tokens, score, sum, accuracy, status) and generate-<subset>.mt.ref.words "
                         "(id, word, pieces, lprob, confidence, min_lprob, not_top), natural logs; needs a manifest")
    ap.add_argument("--speak-reference", action="store_true",
                    help="implies --score-reference; also speaks the reference translation through the unit pass and the vocoder: "
                         "writes generate-<subset>.ref.unit and ref_wav/<n>_pred.wav (the second pass on oracle text)")
    ap.add_argument("--num-shards", type=int, default=int(os.environ.get("WORLD_SIZE", "1")))
    ap.add_argument("--shard-id", type=int, default=int(os.environ.get("RANK", "0")))
    ap.add_argument("--device", default="cuda:%s" % os.environ.get("LOCAL_RANK", "0"))
    # search options of pred.offline-s2st.sh: --beam-mt runs the first-pass text search as a beam search; --beam configures the
    # unit generator, a CTC decoder without a search, so (as in the reference) it changes nothing
    ap.add_argument("--beam-mt", type=int, default=1, help="beam of the first-pass text search (1 = greedy; at most 32)")
    ap.add_argument("--beam", type=int, default=1, help="unit generator beam (accepted for parity; the CTC unit decoder has no search)")
    ap.add_argument("--unkpen", type=float, default=0.0, help="subtracted from the <unk> log-probability of the text search")
    ap.add_argument("--unnormalized", action="store_true", help="text search: do not divide hypothesis scores by their length")
    ap.add_argument("--lenpen", type=float, default=1.0,
                    help="text search: a finished hypothesis' score is divided by length ** lenpen (1 = the plain length)")
    ap.add_argument("--no-repeat-ngram-size", type=int, default=0,
                    help="text search: no n-gram of this size occurs twice in a hypothesis (0 = off; 2 .. 32).  Either of these two "
                         "off its default runs the beam search at --beam-mt 1 too")
    ap.add_argument("--sampling", action="store_true",
                    help="text search: draw --beam-mt independent samples per utterance instead of searching; the best-scoring one "
                         "is spoken, all are written to generate-<subset>.mt.samples (id, rank, score, text)")
    ap.add_argument("--sampling-topk", type=int, default=-1, help="with --sampling: sample from the k most likely tokens (-1 = off)")
    ap.add_argument("--sampling-topp", type=float, default=-1.0,
                    help="with --sampling: sample from the smallest set of tokens whose mass reaches p (-1 = off; not with top-k)")
    ap.add_argument("--seed", type=int, default=1, help="seed of --sampling; an utterance's stream key is its sample id")
    ap.add_argument("--constraints", nargs="?", const="ordered", default=None, choices=["ordered", "unordered"],
                    help="text search: lexically constrained beam search (fairseq's --constraints): every phrase of "
                         "--constraints-file stands in the translation, in the order given.  Only `ordered` is implemented")
    ap.add_argument("--constraints-file", default=None,
                    help="with --constraints: lines `id<TAB>phrase<TAB>phrase...`, phrases as space-separated pieces of the "
                         "target_unigram dictionary; writes C-<id> lines and generate-<subset>.mt.constraints")
    ap.add_argument("--pcm16-io", action="store_true",
                    help="16-bit WAV sources are staged as raw frames, uploaded once and decoded on the device, and pred_wav/ is "
                         "written from 16-bit PCM packed on the device (one download per batch); the same files as without it")
    return ap


def main(argv: Optional[List[str]] = None):
    from .agent import StreamSpeechS2STAgent
    from .modules import CodeHiFiGANVocoderWithDur, StreamSpeechModel, load_model_state
    ap = build_parser()
    a = ap.parse_args(argv)
    if not 1 <= a.beam_mt <= 32:
        ap.error("--beam-mt must be in [1, 32]")
    from .engine import check_search_options
    try:
        check_search_options(a.lenpen, 1.0, a.no_repeat_ngram_size)
        from .engine import sampling_from_fairseq
        sampling_from_fairseq(a.sampling, a.sampling_topk, a.sampling_topp, a.seed)
    except ValueError as e:
        ap.error(str(e))
    if a.constraints == "unordered":
        ap.error("--constraints unordered is not implemented: only the ordered representation (fairseq's default) is")
    if bool(a.constraints) != bool(a.constraints_file):
        ap.error("--constraints and --constraints-file go together")
    if a.constraints and a.sampling:
        ap.error("--constraints cannot be combined with --sampling")
    if a.ctc_beam:
        from .lib import CTC_BEAM_MAX_BEAM, CTC_BEAM_MAX_CAND
        if not 1 <= a.ctc_beam <= CTC_BEAM_MAX_BEAM:
            ap.error(f"--ctc-beam must be in [1, {CTC_BEAM_MAX_BEAM}]")
        if a.ctc_beam_cand is not None and not 1 <= a.ctc_beam_cand <= CTC_BEAM_MAX_CAND:
            ap.error(f"--ctc-beam-cand must be in [1, {CTC_BEAM_MAX_CAND}]")
        if a.ctc_nbest is not None and not 1 <= a.ctc_nbest <= a.ctc_beam:
            ap.error("--ctc-nbest must be in [1, --ctc-beam]")
    elif a.ctc_beam_cand is not None or a.ctc_nbest is not None:
        ap.error("--ctc-beam-cand and --ctc-nbest need --ctc-beam")
    if not a.ctc_beam and (a.ctc_lm_asr or a.ctc_lm_st or a.ctc_lm_weight != 0.5 or a.ctc_word_score != 0.0):
        ap.error("--ctc-lm-asr, --ctc-lm-st, --ctc-lm-weight and --ctc-word-score need --ctc-beam")
    if not (math.isfinite(a.ctc_lm_weight) and math.isfinite(a.ctc_word_score)):
        ap.error("--ctc-lm-weight and --ctc-word-score must be finite")
    if not (a.ctc_keywords_asr or a.ctc_keywords_st) and a.ctc_keyword_threshold != 1.0:
        ap.error("--ctc-keyword-threshold needs --ctc-keywords-asr or --ctc-keywords-st")
    if not a.ctc_keyword_threshold >= 0.0 or a.ctc_keyword_threshold == float("inf"):
        ap.error("--ctc-keyword-threshold must be a finite number >= 0")
    if not a.ctc_beam and (a.ctc_hotwords_asr or a.ctc_hotwords_st or a.ctc_hotword_boost != 1.5):
        ap.error("--ctc-hotwords-asr, --ctc-hotwords-st and --ctc-hotword-boost need --ctc-beam")
    if not math.isfinite(a.ctc_hotword_boost):
        ap.error("--ctc-hotword-boost must be finite")
    if a.spoken_words and a.no_wav:
        ap.error("--spoken-words needs the durations the vocoder predicts: it cannot be combined with --no-wav")
    if a.align_reference and (a.wav_list or a.synthetic > 0 or not a.data):
        ap.error("--align-reference needs the manifest's ids: it cannot be combined with --wav-list or --synthetic")
    if a.align_reference and not any(multitask_text_dir(a.data, a.multitask_config_yaml, t) for t in ("source_unigram", "ctc_target_unigram")):
        ap.error("--align-reference: the multitask YAML names no `data:` directory for source_unigram or ctc_target_unigram")

    if a.speak_reference:
        a.score_reference = True
    if a.score_reference and (a.wav_list or a.synthetic > 0 or not a.data):
        ap.error("--score-reference needs the manifest's ids: it cannot be combined with --wav-list or --synthetic")
    if a.score_reference and not multitask_text_dir(a.data, a.multitask_config_yaml, "target_unigram"):
        ap.error("--score-reference: the multitask YAML names no `data:` directory for target_unigram")
    if a.speak_reference and a.no_wav:
        ap.error("--speak-reference runs the vocoder: it cannot be combined with --no-wav")

    # model / dictionaries / CMVN exactly as the agent loads them (agent :355-420)
    ns = argparse.Namespace(config_yaml=a.config_yaml, multitask_config_yaml=a.multitask_config_yaml,
                            data_bin=a.data or ".", model_path=a.path, global_stats=None, source_segment_size=999999 * 40,
                            shift_size=10, window_size=25, sample_rate=16000, feature_dim=80, full_recompute_encoder=True,
                            gen_subset=a.gen_subset)
    holder = argparse.Namespace(device=a.device)
    StreamSpeechS2STAgent.load_model_vocab(holder, ns)
    model = holder.model.hip
    vcfg = None
    if a.vocoder_cfg:
        import json
        with open(a.vocoder_cfg) as f:
            vcfg = json.load(f)
    voc = CodeHiFiGANVocoderWithDur(a.vocoder, vcfg, device=a.device).hip
    if a.vocoder_fp16:
        voc.set_fp16(True)

    targets: Dict[int, List[int]] = {}
    if a.synthetic > 0:
        from . import workload, synth
        utts = workload.make_utterances(a.synthetic)
        entries = [(u.idx, torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples))) for u in utts]
    else:
        if a.wav_list:
            with open(a.wav_list) as f:
                rows = [(i, ln.strip()) for i, ln in enumerate(f) if ln.strip()]
        else:
            rows = load_manifest(os.path.join(a.data, a.gen_subset + ".tsv"), targets)
        rows = rows[a.shard_id::a.num_shards]
        # MP3 and FLAC rows: batched decodes of up to 640 s of audio each, straight to the device (streamspeech_amd/mp3.py, flac.py);
        # stored-zip cells and .npy paths are read and sniffed (frontend.load_cells); WAV rows as before
        mp3_rows = [k for k, (_, path) in enumerate(rows) if frontend.is_mp3(path) or frontend.is_flac(path)]
        decoded = dict(zip(mp3_rows, frontend.load_audio_batch([rows[k][1] for k in mp3_rows], a.device))) if mp3_rows else {}
        cell_rows = [k for k, (_, path) in enumerate(rows)
                     if k not in decoded and (len(frontend.parse_audio_cell(path)) == 3 or path.lower().endswith(".npy"))]
        feats = {}
        if cell_rows:
            for k, (kind, x, sr) in zip(cell_rows, frontend.load_cells([rows[k][1] for k in cell_rows], a.device)):
                if kind == "feat":
                    feats[k] = x
                else:
                    decoded[k] = (x, sr)
        if feats and len(feats) != len(rows):
            k = next(k for k in range(len(rows)) if k not in feats)
            raise ValueError(f"the manifest mixes precomputed feature rows and audio rows (row {rows[k][0]}: {rows[k][1]!r} is audio); "
                             "a manifest holds one kind")
        if a.pcm16_io and not feats:                # 16-bit WAV rows: raw frames, one upload, one decode launch; others as before
            raw_rows, raws = [], []
            for k, (_, path) in enumerate(rows):
                if k not in decoded:
                    r = frontend.read_wav_raw16(path)
                    if r is not None:
                        raw_rows.append(k)
                        raws.append(r)
            if raws:
                decoded.update(zip(raw_rows, stage_wavs_pcm16(model, raws, a.device)))
        entries = []
        for k, (i, path) in enumerate(rows):
            if feats:
                entries.append((i, feats[k]))
                continue
            if k in decoded:
                x, sr = decoded[k]
            else:
                x, sr = frontend.read_wav(path)
                x = torch.from_numpy(x)
            entries.append((i, x, sr))
    if a.synthetic > 0:
        entries = entries[a.shard_id::a.num_shards]
    is_feat = a.synthetic <= 0 and bool(feats)
    items = []
    for e in entries:
        if is_feat:
            items.append((e[0], e[1].to(a.device)))
            continue
        pcm = e[1].to(a.device)
        if len(e) > 2 and e[2] != 16000:
            pcm = model.resample(pcm, e[2], 16000)
        items.append((e[0], pcm))
    references = load_references(a.data, a.multitask_config_yaml, a.gen_subset, holder.dict) if a.align_reference else None
    mt_references = load_mt_references(a.data, a.multitask_config_yaml, a.gen_subset, holder.dict) if a.score_reference else None
    glossary = None
    if a.constraints:
        with open(a.constraints_file, encoding="utf-8") as f:
            try:
                glossary = parse_constraints_file(f, holder.dict["target_unigram"])
            except ValueError as e:
                ap.error(str(e))
    ctc_lm = {}
    for key, path, name in (("asr", a.ctc_lm_asr, "source_unigram"), ("st", a.ctc_lm_st, "ctc_target_unigram")):
        if path:
            from .ngram import NgramLM, read_arpa
            try:
                arrays = read_arpa(path, holder.dict[name])
            except (OSError, ValueError) as e:
                ap.error(f"--ctc-lm-{key}: {e}")
            ctc_lm[key] = NgramLM(arrays)
            print(f"| --ctc-lm-{key}: order {ctc_lm[key].order}, {ctc_lm[key].entries - 1} n-grams, {arrays['dropped']} dropped (symbols "
                  f"not in {name}), {ctc_lm[key].device_bytes} bytes on the device", file=sys.stderr)
    ctc_bias = {}
    for key, path, name in (("asr", a.ctc_hotwords_asr, "source_unigram"), ("st", a.ctc_hotwords_st, "ctc_target_unigram")):
        if path:
            from .hotwords import CtcBias, read_hotwords
            from .lib import StreamSpeechHipError
            d = holder.dict[name]
            try:
                ctc_bias[key] = CtcBias(*read_hotwords(path, d, a.ctc_hotword_boost), len(d), d.pad(), d.unk())
            except (OSError, ValueError, StreamSpeechHipError) as e:
                ap.error(f"--ctc-hotwords-{key}: {e}")
            print(f"| --ctc-hotwords-{key}: {ctc_bias[key].n_phrases} phrases, {ctc_bias[key].states} states, "
                  f"{ctc_bias[key].device_bytes} bytes on the device", file=sys.stderr)
    ctc_keywords = {}
    for key, path, name in (("asr", a.ctc_keywords_asr, "source_unigram"), ("st", a.ctc_keywords_st, "ctc_target_unigram")):
        if path:
            from .keywords import CtcKeywords
            from .lib import StreamSpeechHipError
            try:
                ctc_keywords[key] = CtcKeywords.from_file(path, holder.dict[name], a.ctc_keyword_threshold)
            except (OSError, ValueError, StreamSpeechHipError) as e:
                ap.error(f"--ctc-keywords-{key}: {e}")
            print(f"| --ctc-keywords-{key}: {ctc_keywords[key].n_keywords} phrases, {ctc_keywords[key].states} states, "
                  f"{ctc_keywords[key].device_bytes} bytes on the device", file=sys.stderr)
    sub = a.gen_subset if a.num_shards == 1 else f"{a.gen_subset}.shard{a.shard_id}"
    hyps = generate(model, voc, items, holder.dict, a.results_path, sub, a.batch_size, a.max_tokens, a.max_len_a,
                    a.max_len_b, a.max_len_a_mt, a.max_len_b_mt, a.dur_prediction, not a.no_wav,
                    getattr(holder.model, "uni_encoder", False), a.scores, targets=targets or None, beam_mt=a.beam_mt,
                    unk_penalty=a.unkpen, normalize=not a.unnormalized,
                    **({"pcm16_out": True} if a.pcm16_io else {}), **({"speaker_id": a.speaker_id} if voc.num_speakers else {}),
                    **({"features": True} if is_feat else {}), **({"word_times": True} if a.word_times else {}),
                    **({"mt_alignment": True} if a.mt_alignment else {}), **({"spoken_words": True} if a.spoken_words else {}),
                    **({"references": references} if references is not None else {}),
                    **({"mt_references": mt_references} if mt_references is not None else {}),
                    **({"speak_reference": True} if a.speak_reference else {}),
                    **({"len_penalty": a.lenpen, "no_repeat_ngram_size": a.no_repeat_ngram_size}
                       if (a.lenpen, a.no_repeat_ngram_size) != (1.0, 0) else {}),
                    **({"sampling": True, "sampling_topk": a.sampling_topk, "sampling_topp": a.sampling_topp, "seed": a.seed}
                       if a.sampling else {}),
                    **({"ctc_beam": a.ctc_beam, "ctc_beam_cand": a.ctc_beam_cand, "ctc_nbest": a.ctc_nbest} if a.ctc_beam else {}),
                    **({"constraints": glossary} if glossary is not None else {}),
                    **({"ctc_lm": ctc_lm, "ctc_lm_weight": a.ctc_lm_weight, "ctc_word_score": a.ctc_word_score} if ctc_lm else {}),
                    **({"ctc_bias": ctc_bias} if ctc_bias else {}),
                    **({"ctc_keywords": ctc_keywords} if ctc_keywords else {}))
    for kw in ctc_keywords.values():
        kw.close()
    for lm in ctc_lm.values():
        lm.close()
    for bias in ctc_bias.values():
        bias.close()
    print(f"| generated {len(hyps)} utterances into {a.results_path}", file=sys.stderr)


if __name__ == "__main__":
    main()
