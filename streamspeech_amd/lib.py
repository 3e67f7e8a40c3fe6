"""ctypes binding of libstreamspeech_hip.so (include/streamspeech_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a symbol declared in
the header is not exported, import of the engine fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SS_HIP_LIB") or os.path.join(_HERE, "libstreamspeech_hip.so")   # env override: tuning builds (tools/)


class SSConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "input_feat", "conv_channels", "conv_kernel", "enc_dim", "enc_ffn", "enc_heads", "enc_layers",
        "dw_kernel", "src_vocab", "tgt_vocab", "mt_layers", "dec_dim", "dec_ffn", "dec_heads",
        "t2u_layers", "unit_layers", "unit_vocab", "ctc_upsample", "pad", "eos", "unk",
        "max_rel_pos", "max_tgt_pos")]


class SSVocoderConfig(C.Structure):
    _fields_ = [
        ("num_embeddings", C.c_int32), ("embedding_dim", C.c_int32), ("model_in_dim", C.c_int32),
        ("upsample_initial_channel", C.c_int32),
        ("n_up", C.c_int32), ("upsample_rates", C.c_int32 * 8), ("upsample_kernel_sizes", C.c_int32 * 8),
        ("n_res", C.c_int32), ("resblock_kernel_sizes", C.c_int32 * 4), ("resblock_dilations", (C.c_int32 * 3) * 4),
        ("dur_hidden", C.c_int32), ("dur_kernel", C.c_int32)]


_vp, _i, _f, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64


class SSPcmSeg(C.Structure):
    """ss_pcm_seg: one chunk of a ss_pcm_scatter call (32 bytes)."""
    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("frames", C.c_int32), ("fmt", C.c_int32),
                ("channels", C.c_int32), ("dst", C.c_int32)]


class SSPcmEmitSeg(C.Structure):
    """ss_pcm_emit_seg: one session of a ss_pcm_emit call (88 bytes)."""
    _fields_ = [("carry", _vp), ("tail", _vp), ("taps", _vp), ("n_before", C.c_int64), ("k0", C.c_int64), ("k1", C.c_int64),
                ("out_offset", C.c_int64), ("carry_len", C.c_int32), ("n_new", C.c_int32), ("up", C.c_int32), ("down", C.c_int32),
                ("half", C.c_int32), ("fmt", C.c_int32), ("finished", C.c_int32), ("reserved", C.c_int32)]


class SSVadState(C.Structure):
    """ss_vad_state: a session's scan state between ss_vad_scan calls (40 bytes); all zero = a fresh stream."""
    _fields_ = [("onset", C.c_int64), ("last_speech", C.c_int64), ("utt_first_frame", C.c_int64), ("floor", C.c_float),
                ("mode", C.c_int32), ("run", C.c_int32), ("reserved", C.c_int32)]


class SSVadSeg(C.Structure):
    """ss_vad_seg: one session of a ss_vad_scan call (96 bytes)."""
    _fields_ = [("hist", _vp), ("state", _vp), ("powers", _vp), ("hist_first", C.c_int64), ("n_hist", C.c_int64),
                ("first_frame", C.c_int64), ("n_frames", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("p_abs", C.c_float), ("p_min", C.c_float), ("snr", C.c_float), ("rise", C.c_float),
                ("min_speech", C.c_int32), ("end_silence", C.c_int32), ("post_roll", C.c_int32), ("max_frames", C.c_int32),
                ("reserved", C.c_int32)]


class SSVadResult(C.Structure):
    """ss_vad_result: what a ss_vad_scan call reports per session (40 bytes)."""
    _fields_ = [("consumed", C.c_int64), ("start_frame", C.c_int64), ("cut_sample", C.c_int64), ("last_speech", C.c_int64),
                ("events", C.c_int32), ("mode", C.c_int32)]


class SSCtcAlignResult(C.Structure):
    """ss_ctc_align_result: what a forced alignment reports per utterance (24 bytes)."""
    _fields_ = [("score", C.c_double), ("viterbi", C.c_double), ("status", C.c_int32), ("n_tokens", C.c_int32)]


CTC_ALIGN_MAX_FRAMES = 1500     # SS_CTC_ALIGN_MAX_FRAMES / SS_CTC_ALIGN_MAX_LABELS of the header
CTC_ALIGN_MAX_LABELS = 1500


class SSCtcBeamHyp(C.Structure):
    """ss_ctc_beam_hyp: one hypothesis of the CTC prefix beam search (16 bytes)."""
    _fields_ = [("score", C.c_double), ("n_tokens", C.c_int32), ("status", C.c_int32)]


class SSCtcBeamLmHyp(C.Structure):
    """ss_ctc_beam_lm_hyp: one hypothesis of the CTC prefix beam search with an n-gram model (32 bytes)."""
    _fields_ = [("score", C.c_double), ("ctc_score", C.c_double), ("lm_score", C.c_double), ("n_tokens", C.c_int32),
                ("status", C.c_int32)]


class SSCtcStreamPart(C.Structure):
    """ss_ctc_stream_part: what one advance of the resumable CTC prefix beam search reports per session (16 bytes)."""
    _fields_ = [("frames", C.c_int32), ("n_stable", C.c_int32), ("n_alive", C.c_int32), ("status", C.c_int32)]


class SSCtcLmOpts(C.Structure):
    """ss_ctc_lm_opts: the weights of the fusion."""
    _fields_ = [("lm_weight", C.c_double), ("word_score", C.c_double), ("eos_term", C.c_int32)]


class SSCtcBiasOpts(C.Structure):
    """ss_ctc_bias_opts: the weight of a hotword set in the search's order, and whether the finish term applies (16 bytes)."""
    _fields_ = [("scale", C.c_double), ("finish", C.c_int32), ("reserved", C.c_int32)]


class SSCtcBeamBiasHyp(C.Structure):
    """ss_ctc_beam_bias_hyp: one hypothesis of the CTC prefix beam search with a hotword set (40 bytes)."""
    _fields_ = [("score", C.c_double), ("ctc_score", C.c_double), ("lm_score", C.c_double), ("bias_score", C.c_double),
                ("n_tokens", C.c_int32), ("status", C.c_int32)]


class SSCtcHit(C.Structure):
    """ss_ctc_hit: one occurrence of a keyword (24 bytes)."""
    _fields_ = [("keyword", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("n_labels", C.c_int32), ("score", C.c_double)]


class SSCtcSpotCount(C.Structure):
    """ss_ctc_spot_count: what a keyword-spotting call reports per utterance or session (16 bytes)."""
    _fields_ = [("n_hits", C.c_int32), ("status", C.c_int32), ("overflow", C.c_int32), ("frames", C.c_int32)]


CTC_SPOT_MAX_LABELS = 32        # SS_CTC_SPOT_MAX_LABELS / _KEYWORDS / _HITS of the header
CTC_SPOT_MAX_KEYWORDS = 65536
CTC_SPOT_MAX_HITS = 16384
CTC_BIAS_MAX_LEN = 32           # SS_CTC_BIAS_MAX_LEN / _PHRASES of the header
CTC_BIAS_MAX_PHRASES = 4096
NGRAM_MAX_ORDER = 6             # SS_NGRAM_MAX_ORDER of the header
CTC_BEAM_MAX_BEAM = 32          # SS_CTC_BEAM_MAX_BEAM / _CAND / _FRAMES of the header
CTC_BEAM_MAX_CAND = 32
CTC_BEAM_MAX_FRAMES = 1500


class SSOpAttnArgs(C.Structure):
    """ss_op_attn_args: AttnArgs (csrc/attention.hpp) field for field, pointers as device addresses."""
    _fields_ = [
        ("Q", _vp), ("K", _vp), ("V", _vp), ("O", _vp),
        ("ldq", C.c_int32), ("ldk", C.c_int32), ("ldv", C.c_int32), ("ldo", C.c_int32),
        ("Tq", C.c_int32), ("Tk", C.c_int32), ("H", C.c_int32),
        ("scale", _f),
        ("causal", C.c_int32), ("chunk", C.c_int32), ("q0", C.c_int32), ("k_mask_tail", C.c_int32),
        ("P", _vp), ("ldp", C.c_int32),
        ("bias_u", _vp), ("bias_v", _vp),
        ("segs", _vp), ("nseg", C.c_int32), ("max_q", C.c_int32), ("p_tmax", C.c_int32),
        ("seg_tail", _vp),
        ("no_decode_kernel", C.c_int32),
        ("anc", _vp), ("anc_ld", C.c_int32), ("anc_slots", C.c_int32),
        ("use_split", C.c_int32)]


class SSOpConvArgs(C.Structure):
    """ss_op_conv_args: the GemmArgs fields (csrc/gemm.hpp) a caller of the conv launcher can set, pointers as device addresses."""
    _fields_ = [
        ("A", _vp), ("W", _vp), ("bias", _vp), ("R", _vp), ("R2", _vp), ("C", _vp), ("C2", _vp),
        ("lda", C.c_int32), ("ldc", C.c_int32), ("ldr", C.c_int32), ("ldr2", C.c_int32), ("ldc2", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("Cin", C.c_int32), ("taps", C.c_int32), ("dil", C.c_int32), ("stride", C.c_int32),
        ("pad", C.c_int32), ("in_len", C.c_int32), ("chunk", C.c_int32),
        ("in_act", C.c_int32), ("in_slope", _f),
        ("act", C.c_int32), ("act_slope", _f), ("alpha", _f), ("div", _f), ("c2_slope", _f),
        ("glu", C.c_int32),
        ("segs", _vp), ("nseg", C.c_int32), ("max_seg_out", C.c_int32),
        ("same_rows", C.c_int32)]


class SSOpPoolAttnArgs(C.Structure):
    """ss_op_pool_attn_args: PoolAttnArgs (csrc/attention.hpp) field for field."""
    _fields_ = [
        ("Qs", _vp), ("cache", _vp), ("O", _vp),
        ("ld", C.c_int32), ("ldo", C.c_int32), ("slot_rows", C.c_int32),
        ("P", _vp), ("ldp", C.c_int32), ("p_tmax", C.c_int32),
        ("bias_u", _vp), ("bias_v", _vp),
        ("sess", _vp), ("qt_pre", _vp),
        ("nsess", C.c_int32), ("qtiles", C.c_int32), ("H", C.c_int32),
        ("scale", _f)]

class SSOpAttnProbsArgs(C.Structure):
    """ss_op_attn_probs_args: AttnProbsArgs (csrc/attn_probs.hpp) field for field, pointers as device addresses."""
    _fields_ = [
        ("Q", _vp), ("K", _vp),
        ("ldq", C.c_int32), ("ldk", C.c_int32), ("H", C.c_int32),
        ("scale", _f),
        ("segs", _vp), ("nseg", C.c_int32),
        ("q_first", _vp), ("row_off", _vp), ("p_off", _vp),
        ("P", _vp), ("peak", _vp), ("stat", _vp),
        ("max_rows", C.c_int32)]


class SSOpBeamState(C.Structure):
    """ss_op_beam_state: BeamState (csrc/beam.hpp) field for field, pointers as device addresses."""
    _fields_ = [(n, _vp) for n in (
        "tok", "cum", "anc", "cand_s", "cand_t", "ignore", "done", "max_len", "npre",
        "fin_cnt", "fin_score", "fin_len", "fin_tok", "fin_pos", "fin_anc")]


class SSMtSearchOpts(C.Structure):
    """ss_mt_search_opts: the search controls beyond beam / unk_penalty / normalize."""
    _fields_ = [("size", C.c_int32), ("no_repeat_ngram", C.c_int32), ("len_penalty", _f), ("temperature", _f)]


def search_opts(len_penalty: float = 1.0, temperature: float = 1.0, no_repeat_ngram_size: int = 0):
    """The ss_mt_search_opts of the three controls, or None when all are at their defaults (the call without options)."""
    if float(len_penalty) == 1.0 and float(temperature) == 1.0 and int(no_repeat_ngram_size) == 0:
        return None
    return SSMtSearchOpts(C.sizeof(SSMtSearchOpts), int(no_repeat_ngram_size), float(len_penalty), float(temperature))


class SSMtSampleOpts(C.Structure):
    """ss_mt_sample_opts: top-k / top-p and the seed of the sampling search."""
    _fields_ = [("size", C.c_int32), ("topk", C.c_int32), ("topp", _f), ("reserved", C.c_int32), ("seed", C.c_uint64)]


def sample_opts(topk: int = 0, topp: float = 0.0, seed: int = 1):
    """The ss_mt_sample_opts of a sampling call (0 = the control is off)."""
    return SSMtSampleOpts(C.sizeof(SSMtSampleOpts), int(topk), float(topp), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)


MT_CONS_MAX_TOKENS = 64  # SS_MT_CONS_MAX_TOKENS / SS_MT_CONS_TABLE_LD of the header
MT_CONS_TABLE_LD = MT_CONS_MAX_TOKENS + 4


def pack_constraints(constraints, B: int):
    """Per-utterance phrase lists -> the (tokens, offsets [B + 1], end markers) int32 arrays of ss_batch_mt_beam_cons.
    ``constraints[b]`` is a list of phrases, each a non-empty list of token ids; None stands for no phrases."""
    import numpy as np
    if len(constraints) != B:
        raise ValueError(f"constraints for {len(constraints)} utterances, batch of {B}")
    toks, ends, off = [], [], [0]
    for b, phrases in enumerate(constraints):
        for p in (phrases or []):
            p = [int(x) for x in p]
            if not p:
                raise ValueError(f"utterance {b}: an empty constraint phrase")
            toks += p
            ends += [0] * (len(p) - 1) + [1]
        off.append(len(toks))
    return (np.asarray(toks or [0], np.int32), np.asarray(off, np.int32), np.asarray(ends or [0], np.int32))


SS_OP_BEAM_CAND = 64     # row stride of the candidate lists of ss_op_beam_topk / ss_op_beam_merge

# symbol -> (restype, argtypes); must list every function include/streamspeech_hip.h declares
SIGNATURES = {
    "ss_abi_version": (_i, []),
    "ss_error_string": (C.c_char_p, [_i]),
    "ss_model_create": (_i, [C.POINTER(SSConfig), _vp, C.c_size_t, C.POINTER(C.c_char_p), C.POINTER(_i64),
                             C.POINTER(_i64), _i, C.POINTER(_vp)]),
    "ss_model_destroy": (None, [_vp]),
    "ss_scratch_create": (_i, [C.POINTER(_vp)]),
    "ss_scratch_destroy": (None, [_vp]),
    "ss_scratch_set_cap": (_i, [_vp, C.c_size_t]),
    "ss_scratch_trim": (_i, [_vp, C.c_size_t]),
    "ss_scratch_bytes": (C.c_size_t, [_vp]),
    "ss_model_bind_scratch": (_i, [_vp, _vp]),
    "ss_vocoder_bind_scratch": (_i, [_vp, _vp]),
    "ss_fbank_num_frames": (_i, [_i]),
    "ss_fbank_cmvn": (_i, [_vp, _vp, _vp, _i, _f, _vp, C.POINTER(_i)]),
    "ss_encoder_out_len": (_i, [_i]),
    "ss_resample": (_i, [_vp, _vp, _i64, _i, _i, _vp, _i, _vp, _i64]),
    "ss_mp3_probe": (_i, [_vp, C.c_size_t, _vp]),
    "ss_mp3_unpack": (_i, [_vp, C.c_size_t, _i64, _vp, _vp, _vp]),
    "ss_mp3_synthesize": (_i, [_vp, _vp, _vp, _i64, _vp, _i, _i, _vp, _i64, _vp, C.POINTER(C.c_size_t)]),
    "ss_mp3_stream_create": (_i, [_i, C.POINTER(_vp)]),
    "ss_mp3_stream_destroy": (None, [_vp]),
    "ss_mp3_stream_reset": (_i, [_vp]),
    "ss_mp3_stream_bound": (_i64, [_vp, C.c_size_t]),
    "ss_mp3_stream_push": (_i, [_vp, _vp, C.c_size_t, _i, _i64, _vp, _vp, _vp, C.POINTER(_i64), _vp]),
    "ss_mp3_stream_query": (_i, [_vp, _vp]),
    "ss_mp3_stream_copy": (_i, [_vp, _vp]),
    "ss_mp3_stream_synthesize": (_i, [_vp, _vp, _vp, _i64, _vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i64), _i, _i, _vp,
                                      C.POINTER(C.c_size_t)]),
    "ss_flac_streaminfo": (_i, [_vp, C.c_size_t, _vp]),
    "ss_flac_probe": (_i, [_vp, C.c_size_t, _vp]),
    "ss_flac_unpack": (_i, [_vp, C.c_size_t, _i64, _vp, _vp, _i64, _vp]),
    "ss_flac_restore_host": (_i, [_vp, _vp, _i64, _vp, _i, _i, _vp, _vp]),
    "ss_flac_restore": (_i, [_vp, _vp, _vp, _i64, _i64, _vp, _i, _i, _vp, _i64, _vp, C.POINTER(C.c_size_t)]),
    "ss_pcm_scatter": (_i, [_vp, _vp, _i64, _vp, _i, C.POINTER(_vp), C.POINTER(_i64), _i]),
    "ss_pcm_pack_s16": (_i, [_vp, _vp, _i64, _vp]),
    "ss_pcm_decode_host": (_i, [_vp, _i, _i, _i64, _vp]),
    "ss_pcm_pack_s16_host": (_i, [_vp, _i64, _vp]),
    "ss_pcm_emit_count": (_i64, [_i64, _i, _i, _i, _i]),
    "ss_pcm_emit": (_i, [_vp, _vp, _i, _vp, _i64]),
    "ss_pcm_emit_host": (_i, [_vp, _i, _vp, _i64]),
    "ss_pcm_encode_host": (_i, [_vp, _i64, _i, _vp]),
    "ss_vad_scan": (_i, [_vp, _vp, _i, _vp]),
    "ss_vad_scan_host": (_i, [_vp, _i, _vp]),
    "ss_row_max_logprob": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "ss_log_softmax": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "ss_encoder_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "ss_encoder_stream_reset": (_i, [_vp]),
    "ss_encoder_stream_set_tail": (_i, [_vp, _i]),
    "ss_encoder_stream_set_deferred": (_i, [_vp, _i]),
    "ss_encoder_stream_status": (_i, [_vp, _vp, _vp]),
    "ss_debug_enc_step_inject_timeout": (_i, [_vp]),
    "ss_encoder_stream_forward": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ss_ctc_greedy_scored": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ss_ctc_greedy": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "ss_stream_pool_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "ss_stream_pool_destroy": (None, [_vp]),
    "ss_stream_pool_reset": (_i, [_vp, _i]),
    "ss_stream_pool_set_tail": (_i, [_vp, _i, _i]),
    "ss_encoder_stream_forward_batch": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int32), C.POINTER(_vp), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]),
    "ss_stream_pool_set_scores": (_i, [_vp, _i]),
    "ss_stream_pool_ctc_scored": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ss_stream_pool_ctc": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp]),
    "ss_stream_pool_stats": (_i, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "ss_mt_begin": (_i, [_vp, _vp, _vp, _i]),
    "ss_mt_set_persistent": (_i, [_vp, _i]),
    "ss_model_set_pack_invariant": (_i, [_vp, _i]),
    "ss_model_get_pack_invariant": (_i, [_vp]),
    "ss_debug_canon": (_i, [_i]),
    "ss_mt_get_persistent": (_i, [_vp]),
    "ss_debug_mt_inject_timeout": (_i, [_vp]),
    "ss_mt_append": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i]),
    "ss_mt_truncate": (_i, [_vp, _i]),
    "ss_mt_greedy": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int32), _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(_i),
                          _vp, C.POINTER(_i)]),
    "ss_t2u_units": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i]),
    "ss_vocoder_create": (_i, [C.POINTER(SSVocoderConfig), _vp, C.c_size_t, C.POINTER(C.c_char_p),
                               C.POINTER(_i64), C.POINTER(_i64), _i, C.POINTER(_vp)]),
    "ss_vocoder_destroy": (None, [_vp]),
    "ss_vocoder_set_bf16x3": (_i, [_vp, _i]),
    "ss_vocoder_set_f16": (_i, [_vp, _i]),
    "ss_vocoder_forward": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i64, _vp, C.POINTER(_i64)]),
    "ss_vocoder_num_speakers": (_i, [_vp]),
    "ss_vocoder_forward_spkr": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i64, _vp, C.POINTER(_i64), C.c_int32]),
    "ss_batch_vocoder_forward_spkr": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), _i, _vp, _vp, _i64, _vp,
                                           C.POINTER(_i64), C.POINTER(_i64), C.POINTER(C.c_int32)]),
    "ss_batch_vocoder_tail_spkr": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), _i, _vp, _i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(_i64), C.POINTER(_i64), C.POINTER(C.c_int32)]),
    "ss_batch_fbank_cmvn": (_i, [_vp, _vp, _i, _vp, C.POINTER(_i64), C.POINTER(C.c_int32), _f, _vp, C.POINTER(C.c_int32)]),
    "ss_batch_cmvn": (_i, [_vp, _vp, _vp, _i64, _vp]),
    "ss_batch_encoder_forward": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), _i, _i, _vp, C.POINTER(C.c_int32)]),
    "ss_batch_ctc_greedy_scored": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ss_batch_ctc_greedy": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp]),
    "ss_batch_ctc_align": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp,
                                _vp, _vp]),
    "ss_ctc_align_host": (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp,
                               _vp, _vp, _vp]),
    "ss_batch_ctc_beam": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i]),
    "ss_ctc_beam_host": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "ss_ngram_lm_create": (_i, [_i, C.POINTER(C.c_int64), _vp, _vp, _vp, _i, _i, _i, _i, _f, C.POINTER(_vp)]),
    "ss_ngram_lm_destroy": (None, [_vp]),
    "ss_ngram_lm_info": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ss_ngram_score_host": (_i, [_vp, _i, _vp, C.POINTER(C.c_int32), _i, _vp, _vp]),
    "ss_batch_ctc_beam_lm": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, C.POINTER(SSCtcLmOpts)]),
    "ss_ctc_beam_lm_host": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp,
                                 C.POINTER(SSCtcLmOpts)]),
    "ss_ctc_bias_create": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, C.POINTER(_vp)]),
    "ss_ctc_bias_destroy": (None, [_vp]),
    "ss_ctc_bias_info": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ss_ctc_bias_score_host": (_i, [_vp, _i, _vp, C.POINTER(C.c_int32), _i, _vp, _vp, _vp]),
    "ss_batch_ctc_beam_bias": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, C.POINTER(SSCtcLmOpts),
                                    _vp, C.POINTER(SSCtcBiasOpts)]),
    "ss_ctc_beam_bias_host": (_i, [_vp, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp,
                                   C.POINTER(SSCtcLmOpts), _vp, C.POINTER(SSCtcBiasOpts)]),
    "ss_ctc_stream_create_bias": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, C.POINTER(SSCtcLmOpts), _vp, C.POINTER(SSCtcBiasOpts),
                                       C.POINTER(_vp)]),
    "ss_ctc_stream_create": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, C.POINTER(SSCtcLmOpts), C.POINTER(_vp)]),
    "ss_ctc_stream_destroy": (None, [_vp]),
    "ss_ctc_stream_reset": (_i, [_vp, _i]),
    "ss_ctc_stream_advance": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), _vp, _vp, _i, _vp]),
    "ss_ctc_stream_advance_host": (_i, [_vp, _i, C.POINTER(C.c_int32), _vp, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp,
                                        _i, _vp]),
    "ss_ctc_spot_set_create": (_i, [_i, _vp, _vp, _vp, _i, _i, _i, C.POINTER(_vp)]),
    "ss_ctc_spot_set_destroy": (None, [_vp]),
    "ss_ctc_spot_set_info": (_i, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int64)]),
    "ss_batch_ctc_spot": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), _vp, _i, _vp, _vp]),
    "ss_ctc_spot_host": (_i, [_vp, _i, _i, C.POINTER(C.c_int32), _vp, _i, _vp, _vp]),
    "ss_ctc_spot_stream_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "ss_ctc_spot_stream_destroy": (None, [_vp]),
    "ss_ctc_spot_stream_reset": (_i, [_vp, _i]),
    "ss_ctc_spot_stream_advance": (_i, [_vp, _vp, _vp, _i, C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), _i, _vp, _vp]),
    "ss_ctc_spot_stream_advance_host": (_i, [_vp, _i, C.POINTER(C.c_int32), _vp, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i,
                                             _vp, _vp]),
    "ss_batch_mt_greedy": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i,
                                C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _vp, _i]),
    "ss_batch_mt_beam": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _f, _i,
                              C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(_f), C.POINTER(_f), _vp, _i]),
    "ss_batch_mt_continue": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), _vp, _i,
                                  C.POINTER(C.c_int32)]),
    "ss_batch_mt_continue_plan": (_i, [_i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       _i64, C.POINTER(_i64)]),
    "ss_batch_mt_beam_continue": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), _i, _f, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32),
                                       C.POINTER(_f), C.POINTER(_f), _vp, _i]),
    "ss_batch_mt_beam_continue_plan": (_i, [_i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), _i64, C.POINTER(_i64)]),
    "ss_batch_mt_beam_opts": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _f, _i,
                                   C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(_f), C.POINTER(_f), _vp, _i,
                                   C.POINTER(SSMtSearchOpts)]),
    "ss_batch_mt_beam_continue_opts": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_int32), _i, _f, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32),
                                            C.POINTER(_f), C.POINTER(_f), _vp, _i, C.POINTER(SSMtSearchOpts)]),
    "ss_batch_mt_beam_continue_plan_opts": (_i, [_i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_int32), _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_int32), _i64, C.POINTER(_i64), C.POINTER(SSMtSearchOpts)]),
    "ss_batch_mt_sample": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _f, _i,
                                C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(_f), C.POINTER(_f), _vp, _i,
                                C.POINTER(SSMtSearchOpts), C.POINTER(_i64), C.POINTER(SSMtSampleOpts)]),
    "ss_batch_mt_sample_continue": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), _i, _f, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32),
                                         C.POINTER(_f), C.POINTER(_f), _vp, _i, C.POINTER(SSMtSearchOpts), C.POINTER(_i64),
                                         C.POINTER(SSMtSampleOpts)]),
    "ss_mt_cons_table_host": (_i, [_i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _i, _i,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ss_batch_mt_beam_cons": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _f, _i,
                                   C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(_f), C.POINTER(_f), _vp, _i,
                                   C.POINTER(SSMtSearchOpts), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ss_mt_cons_select_host": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "ss_batch_fbank_frames": (_i, [_vp, _vp, _i, C.POINTER(_vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _f,
                                   C.POINTER(_vp)]),
    "ss_batch_fbank_frames_sr": (_i, [_vp, _vp, _i, C.POINTER(_vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                      C.POINTER(_vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _f,
                                      C.POINTER(_vp)]),
    "ss_fbank_sr_rows": (_i, [_i64, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ss_batch_t2u_units": (_i, [_vp, _vp, _i, _vp, _i, C.POINTER(C.c_int32), _i, _i, _vp, _vp, _vp]),
    "ss_batch_vocoder_forward": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), _i, _vp, _vp, _i64, _vp,
                                      C.POINTER(_i64), C.POINTER(_i64)]),
    "ss_batch_t2u_units_pad": (_i, [_vp, _vp, _i, _vp, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i, _i, _vp, _vp, _vp]),
    "ss_batch_mt_features": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_int32), _vp, _i]),
    "ss_batch_mt_attention": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), _vp, _i, _vp, C.POINTER(_i64), _i64, _vp, _vp]),
    "ss_batch_mt_score": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                               C.POINTER(C.c_int32), _vp, _i, _vp, _vp]),
    "ss_batch_vocoder_tail": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), _i, _vp, _i64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(_i64), C.POINTER(_i64)]),
    "ss_batch_unit_spans": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_int32), _vp, _vp, _vp, _vp]),
    "ss_unit_spans_host": (_i, [_i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp,
                                _i, _i, _i, _i, _i, _vp, _vp]),
    "ss_op_unit_spans": (_i, [_vp, _i, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                              _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "ss_prof_enable": (_i, [_i]),
    "ss_prof_enable_hi": (_i, [_i]),
    "ss_prof_reset": (_i, []),
    "ss_prof_read": (_i, [_i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i64), C.POINTER(C.c_double)]),
    "ss_prof_totals": (_i, [_i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i64)]),
    "ss_prof_read_issued": (_i, [_i, C.POINTER(C.c_double)]),
    "ss_prof_shape_log": (_i, [_i]),
    "ss_prof_shape_dump": (_i, [C.c_char_p, _i]),
    "ss_prof_num_classes": (_i, []),
    "ss_prof_class_name": (C.c_char_p, [_i]),
    "ss_debug_force_tile": (_i, [_i, _i, _i]),
    "ss_op_ffn_fused": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _i, _i, _i]),
    "ss_debug_ffn": (_i, [_i, _i, _i]),
    "ss_debug_rtlin": (_i, [_i, _i]),
    "ss_debug_rtlin_kb": (_i, [_i, _i]),
    "ss_debug_rtlin_kb_last": (_i, [C.POINTER(C.c_int32)]),
    "ss_debug_unit_l0_distinct": (_i, [_i]),
    "ss_debug_fbank_dense": (_i, [_i]),
    "ss_fbank_mel_ranges": (_i, [_vp, _i, _i, C.POINTER(C.c_int32)]),
    "ss_debug_conv_c64": (_i, [_i]),
    "ss_debug_conv_c256_rows": (_i, [_i]),
    "ss_debug_conv_c32": (_i, [_i]),
    "ss_debug_conv_c16": (_i, [_i]),
    "ss_debug_enc_step_launches": (_i64, []),
    "ss_debug_scratch_audit": (_i, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "ss_op_ln_linear": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _i]),
    "ss_op_ln_linear_ex": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _i, _i]),
    "ss_debug_last_logits": (_i, [_vp, _vp, _vp, _i64, C.POINTER(_i), C.POINTER(_i)]),
    "ss_debug_sk_errors": (_i, []),
    "ss_debug_attention_split": (_i, [_i]),
    "ss_debug_attention_q16": (_i, [_i]),
    "ss_op_conv_gemm": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i,
                             _i, _f, _i, _f, _f, _i]),
    "ss_op_conv_gemm_ex": (_i, [_vp, C.POINTER(SSOpConvArgs)]),
    "ss_op_conv_gemm_rows": (_i, [_vp, C.POINTER(SSOpConvArgs), _i, _vp, _vp, _i]),
    "ss_op_conv_pair": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _f, _vp, _i, _f, _i, _i, _i, _i, _i, _f, _vp, _i]),
    "ss_op_resblock_fused": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _f, _i, _i, _i, _f, _vp, _i]),
    "ss_debug_slab": (_i, [_i, C.c_longlong]),
    "ss_op_conv_f16": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _f, _vp, _i]),
    "ss_op_layernorm": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _f]),
    "ss_op_attention": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _f, _i, _i, _vp, _i, _vp, _vp]),
    "ss_op_attention_ex": (_i, [_vp, C.POINTER(SSOpAttnArgs)]),
    "ss_op_attention_probs": (_i, [_vp, C.POINTER(SSOpAttnProbsArgs)]),
    "ss_op_attention_pool": (_i, [_vp, C.POINTER(SSOpPoolAttnArgs)]),
    "ss_debug_attention_no_mfma": (_i, [_i]),
    "ss_op_dwconv_bn_silu": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _i]),
    "ss_op_dwconv_bn_silu_ex": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _f, _i, _i, _i, _vp, _i, _i]),
    "ss_op_pool_dwconv": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _f, _i, _vp, _i, _i]),
    "ss_op_pool_gather_rows": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i]),
    "ss_op_pool_gather_ids": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i]),
    "ss_op_pool_stack_rows": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i]),
    "ss_op_masked_argmax": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _i]),
    "ss_op_ctc_collapse": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i]),
    "ss_op_masked_argmax_lprob": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "ss_op_mt_token_scores": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ss_debug_mt_score_form": (_i, [_i]),
    "ss_op_ctc_collapse_spans": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "ss_op_ctc_align": (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp,
                             _vp, _vp, _vp]),
    "ss_op_ctc_beam": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    "ss_debug_ctc_beam_host_max": (_i, [_i]),
    "ss_op_ctc_beam_lm": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp,
                               C.POINTER(SSCtcLmOpts)]),
    "ss_debug_ctc_stream_create": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.POINTER(SSCtcLmOpts), C.POINTER(_vp)]),
    "ss_op_ctc_stream_advance": (_i, [_vp, _vp, _i, C.POINTER(C.c_int32), _vp, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp,
                                      _vp, _i, _vp]),
    "ss_op_ctc_beam_bias": (_i, [_vp, _vp, _i, _i, _i, _i, _i, C.POINTER(C.c_int32), _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp,
                                 C.POINTER(SSCtcLmOpts), _vp, C.POINTER(SSCtcBiasOpts)]),
    "ss_debug_ctc_stream_create_bias": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, C.POINTER(SSCtcLmOpts), _vp,
                                             C.POINTER(SSCtcBiasOpts), C.POINTER(_vp)]),
    "ss_op_ctc_bias_score": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), _i, _vp, _vp, _vp]),
    "ss_op_ctc_spot": (_i, [_vp, _vp, _i, _i, C.POINTER(C.c_int32), _vp, _i, _vp, _vp]),
    "ss_debug_ctc_spot_phases": (_i, [_i]),
    "ss_debug_ctc_spot_trace_host": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "ss_debug_ctc_spot_stream_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "ss_op_ctc_spot_stream_advance": (_i, [_vp, _vp, _i, C.POINTER(C.c_int32), _vp, _i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _i,
                                           _vp, _vp]),
    "ss_op_ngram_score": (_i, [_vp, _vp, _i, _vp, C.POINTER(C.c_int32), _i, _vp, _vp]),
    "ss_op_dur_predict": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i]),
    "ss_op_repeat_rows": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _vp, _i]),
    "ss_op_embed_tokens": (_i, [_vp, _vp, _vp, _vp, _f, _i, _vp, _i, _i, _i, _i, _i]),
    "ss_op_embed_tokens_rows": (_i, [_vp, _vp, _vp, _vp, _i, _f, _i, _vp, _vp, _i, _i, _i, _i]),
    "ss_op_upsample_add_pos": (_i, [_vp, _vp, _i, _i, _vp, _f, _vp, _i]),
    "ss_op_gather_rows": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i]),
    "ss_op_scatter_rows": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i]),
    "ss_op_conv_post_tanh": (_i, [_vp, _vp, _i, _i, _vp, _vp, _f, _vp, _vp, _i]),
    "ss_op_conv_post_tanh_crop": (_i, [_vp, _vp, _i, _vp, _vp, _f, _vp, _vp, _i, _i]),
    "ss_op_spkr_pre_add": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _f]),
    "ss_op_beam_topk": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp]),
    "ss_op_beam_merge": (_i, [_vp, C.POINTER(SSOpBeamState), _i, _i, _i, _i, _i, _i, _i, _i]),
    "ss_op_beam_prefix_score": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _vp]),
    "ss_op_beam_prefix_chain": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ss_op_beam_topk_opts": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _f, _i, _vp, _vp, _i, _i,
                                  _vp, _vp, _vp]),
    "ss_op_beam_merge_opts": (_i, [_vp, C.POINTER(SSOpBeamState), _i, _i, _i, _i, _i, _i, _i, _i, _f]),
    "ss_op_beam_prefix_score_opts": (_i, [_vp, _vp, _i, _i, _vp, _i, _i, _f, _vp, _f]),
    "ss_op_beam_cons_select": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ss_op_sample_step": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp,
                               C.POINTER(SSMtSampleOpts), _vp, _vp, _vp, _vp]),
    "ss_op_sample_uniform": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
}

_lib = None


# return codes of the C ABI that callers act on (the full list: include/streamspeech_hip.h)
SS_ERR_ARG = 2
SS_ERR_CAPACITY = 4
SS_ERR_SCRATCH_CAP = 5
SS_ERR_STREAM_REPEAT = 8


class StreamSpeechHipError(RuntimeError):
    """A failed library call; ``code`` is its SS_ERR_* return code (None for errors raised on the Python side)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def load():
    """dlopen the HIP library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StreamSpeechHipError(
            f"{LIB_PATH} not found: build it with streamspeech_amd/csrc/build.sh "
            "(or __graft_entry__.build()).  There is no CPU fallback for the product path.")
    # torch FIRST: its wheel carries its own HIP runtime; libstreamspeech_hip.so must bind to the runtime torch initialised (device
    # memory, streams and events cross the boundary), not bring up /opt/rocm's copy before torch loads -- a process that dlopen-ed this
    # library and only then imported torch (`__graft_entry__.build()` followed by `smoke()` in one process) got "no ROCm-capable device"
    # from hipMalloc inside ss_model_create (profiles/r05_smoke_load_order.log).
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise StreamSpeechHipError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.ss_abi_version() != 2:
        raise StreamSpeechHipError("ABI version mismatch")
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().ss_error_string(rc).decode()
        raise StreamSpeechHipError(f"{what} failed: {msg} (code {rc})", rc)
