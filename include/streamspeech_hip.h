/* streamspeech_hip.h -- C ABI of the MI355X-native StreamSpeech S2ST forward pass.
 *
 * Drop-in boundary: the reference has no FFI -- its S2ST path is torch modules
 * called from the SimulEval agent -- so each entry point below replaces one module call the agent
 * makes (reference agent/speech_to_speech.streamspeech.agent.py, cited per function).  Signatures
 * carry only plain pointers and sizes: `d_*` arguments are DEVICE (HBM) pointers, `h_*` are host
 * pointers, `stream` is a hipStream_t passed as void*.  Every call is stream-ordered unless it
 * says "synchronises".  All arithmetic is FP32.  Return value: 0 = ok, non-zero = SS_ERR_*:
 * 1 HIP runtime error, 2 invalid argument, 3 weight slot missing or wrong size, 4 output capacity
 * too small, 5 SS_ERR_SCRATCH_CAP (ss_scratch_set_cap), 6 SS_ERR_BITSTREAM and 7 SS_ERR_UNSUPPORTED
 * (ss_mp3_*, ss_flac_*), 8 SS_ERR_STREAM_REPEAT (ss_encoder_stream_forward).
 * Additions since ABI 2 was cut (no existing signature changed): ss_flac_streaminfo, ss_flac_probe, ss_flac_unpack,
 * ss_flac_restore_host, ss_flac_restore (FLAC ingest), ss_batch_cmvn (precomputed fbank rows), ss_batch_mt_attention and
 * ss_op_attention_probs (cross-attention of the first-pass text decoder), ss_batch_unit_spans, ss_unit_spans_host and
 * ss_op_unit_spans (where each text-decoder state is spoken in the output speech), ss_batch_mt_score, ss_op_mt_token_scores and
 * ss_debug_mt_score_form (the text decoder's score of a given translation), ss_ctc_spot_set_*, ss_batch_ctc_spot, ss_ctc_spot_host,
 * ss_op_ctc_spot, ss_ctc_spot_stream_*, ss_debug_ctc_spot_stream_create and ss_op_ctc_spot_stream_advance (keyword spotting on the
 * text CTC heads).
 *
 * Weight ownership: the caller owns one packed FP32 weight blob in HBM (built once from a fairseq
 * state dict by streamspeech_amd/weights.py) and lends it to ss_model_create(); the library keeps
 * borrowed pointers into it; scratch / caches live in scratch sets (ss_scratch_*, hipMalloc).
 */
#ifndef STREAMSPEECH_HIP_H
#define STREAMSPEECH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SS_ABI_VERSION 2              /* 2 (round 6): scratch sets are objects of their own (ss_scratch_*), SS_ERR_SCRATCH_CAP */

typedef struct ss_model ss_model;      /* StreamSpeechModel replacement (encoder + CTC + MT + T2U + unit decoder): WEIGHTS of one language */
typedef struct ss_vocoder ss_vocoder;  /* CodeHiFiGANVocoderWithDur replacement: WEIGHTS */
typedef struct ss_scratch ss_scratch;  /* everything a call mutates: activations, KV caches, stream-K hand-off state, streaming state */
typedef struct ss_stream_pool ss_stream_pool;  /* incremental-encoder state of many concurrent streams (ss_stream_pool_*) */

/* Architecture hyper-parameters (reference researches/ctc_unity/models/streamspeech_model.py:418-430
 * and train_scripts/train.offline-s2st.sh). */
typedef struct ss_config {
  int32_t input_feat, conv_channels, conv_kernel;
  int32_t enc_dim, enc_ffn, enc_heads, enc_layers, dw_kernel;
  int32_t src_vocab, tgt_vocab;
  int32_t mt_layers, dec_dim, dec_ffn, dec_heads;
  int32_t t2u_layers, unit_layers, unit_vocab, ctc_upsample;
  int32_t pad, eos, unk;
  int32_t max_rel_pos;     /* Tmax: the projected rel-pos table covers offsets -(Tmax-1)..Tmax-1 */
  int32_t max_tgt_pos;     /* rows in the MT sinusoid table */
} ss_config;

typedef struct ss_vocoder_config {
  int32_t num_embeddings, embedding_dim, model_in_dim, upsample_initial_channel;
  int32_t n_up;  int32_t upsample_rates[8];  int32_t upsample_kernel_sizes[8];
  int32_t n_res; int32_t resblock_kernel_sizes[4]; int32_t resblock_dilations[4][3];
  int32_t dur_hidden, dur_kernel;
} ss_vocoder_config;

int ss_abi_version(void);
const char* ss_error_string(int code);

/* ---- model lifetime ------------------------------------------------------------------------
 * names[i] / offsets[i] / numels[i]: slot i of the packed blob starts offsets[i] floats into
 * d_blob and holds numels[i] floats.  Replaces load_model_ensemble + model.cuda()
 * (agent :355-420).  Synchronises (builds the per-layer projected rel-pos tables). */
int ss_model_create(const ss_config* cfg, const float* d_blob, size_t blob_floats,
                    const char* const* names, const int64_t* offsets, const int64_t* numels,
                    int n_slots, ss_model** out);
void ss_model_destroy(ss_model* m);

/* ---- scratch sets -----------------------------------------------------------------------------
 * The reference loads one model per language directory (configs/{fr,es,de}-en/, agent :357-401) and PyTorch's caching allocator
 * holds the activations of whatever runs.  Here a weight handle (ss_model / ss_vocoder: borrowed pointers into the blob -- a few KB;
 * the projected rel-pos table and the Winograd weight forms are shared per blob) is separate from a SCRATCH SET, which owns
 * everything a call mutates.  A handle runs on the scratch set it is bound to: its own (made by ss_*_create, empty until used)
 * or, after ss_model_bind_scratch / ss_vocoder_bind_scratch, a shared one -- so L languages on S concurrent streams need S scratch
 * sets and L x S handles, not L x S scratch sets.  Rules: a scratch set (and every handle bound to it) is driven by ONE host
 * thread at a time; a stateful sequence (ss_mt_begin ... ss_mt_append / ss_mt_truncate, ss_encoder_stream_*) stays on one (handle,
 * scratch) pair from start to end; between sequences any handle bound to the set may use it.  Ref-counted: the memory goes when
 * ss_scratch_destroy has been called AND every handle bound to the set is destroyed or re-bound.
 * Buffers grow on demand and never shrink by themselves: ss_scratch_set_cap bounds their sum (a call that would pass it returns
 * SS_ERR_SCRATCH_CAP and leaves the set as it was; 0 = no cap), ss_scratch_trim synchronises the device and lets the largest
 * re-sizable buffers go until at most keep_bytes are held (fixed pieces -- MT cache, token chain, zero-initialised counters -- stay),
 * ss_scratch_bytes reports what is held.  Every device buffer of the set is counted and capped, the streaming encoder's per-layer
 * state included (a grow of it holds the old and the new buffers at once, and the cap sees both).  (The stream-K hand-off
 * workspace, 32 MB + flags per set, is not counted.)
 * Both ss_scratch_trim and ss_model_bind_scratch (for the set the handle LEAVES) end a streaming-encoder sequence on that set: the
 * next ss_encoder_stream_forward starts a fresh stream.  A deferred time-out check still outstanding there (ss_encoder_stream_set_deferred)
 * is settled first -- the device is synchronised, a real time-out is counted and the set leaves the persistent form -- and its
 * verdict is dropped, since the stream starts over anyway: nothing of the unchecked call survives. */
int ss_scratch_create(ss_scratch** out);
void ss_scratch_destroy(ss_scratch* sc);
int ss_scratch_set_cap(ss_scratch* sc, size_t max_bytes);
int ss_scratch_trim(ss_scratch* sc, size_t keep_bytes);
size_t ss_scratch_bytes(ss_scratch* sc);
int ss_model_bind_scratch(ss_model* m, ss_scratch* sc);
int ss_vocoder_bind_scratch(ss_vocoder* v, ss_scratch* sc);

/* ---- a1: OnlineFeatureExtractor.__call__ (agent :66-98) on 16 kHz PCM already in HBM.
 * d_feat must hold ss_fbank_num_frames(n_samples)*80 floats. */
int ss_fbank_num_frames(int n_samples);
int ss_fbank_cmvn(ss_model* m, void* stream, const float* d_pcm16k, int n_samples, float pcm_scale,
                  float* d_feat, int* h_n_frames);

/* Waveform front-end: rational polyphase resampling on the device, standing in for
 * the sox `rate` effect of convert_waveform (fairseq/data/audio/audio_utils.py:53-62; third-party
 * arithmetic outside the fbank-input parity contract).  d_out[k] = sum_m d_in[m] *
 * d_taps[half_len + k*down - m*up] for k < n_out; n_out is normally ceil(n_in*up/down), up/down in
 * lowest terms, d_taps [2*half_len+1] is the host-designed low-pass with gain `up`
 * (streamspeech_amd/frontend.py design_filter).
 * A STREAMING source at another rate than 16 kHz does not go through ss_resample + ss_fbank_cmvn over its growing history: the
 * rows that can still change are made from the source-rate history in one launch for any number of sessions, with this
 * resampler's sum inside the fbank row's workgroup (ss_batch_fbank_frames_sr and ss_fbank_sr_rows, with the ragged-batch calls
 * below). */
int ss_resample(void* stream, const float* d_in, int64_t n_in, int up, int down, const float* d_taps,
                int half_len, float* d_out, int64_t n_out);

/* MP3 ingest: MPEG-1 / MPEG-2 LSF / MPEG-2.5 Layer III sources, standing in for the soundfile.read the
 * reference's loaders call on `.mp3` paths (SimulEval/simuleval/data/dataloader/s2t_dataloader.py:62-63,
 * fairseq/data/audio/audio_utils.py:69-110).  Two stages: the serial bitstream part (headers, side info, bit reservoir,
 * scalefactors, Huffman) runs on the host -- no global mutable state, no HIP runtime call, safe from many threads at once --
 * and writes one ss_mp3_granule record plus int16 q[576] per granule-channel; the numeric part (requantisation, MS stereo,
 * alias reduction, IMDCT, overlap-add, polyphase synthesis) runs on the device over a ragged batch of files.
 * Container: ID3v2 (with footer), trailing ID3v1 and APEv2 tags are skipped; a header is taken only when the next frame's
 * header agrees with it (resynchronisation over garbage); CRC words are skipped unchecked; a Xing / Info frame is not audio,
 * and a LAME tag in it sets the gapless trim (delay + 529 samples at the start, padding - 529 at the end; no tag: no trim).
 * Refused: intensity stereo, free-format bitrate, Layers I / II and reserved header fields (SS_ERR_UNSUPPORTED = 7); corrupt or
 * inconsistent data, including Huffman data that overruns part2_3_length (SS_ERR_BITSTREAM = 6).  A truncated last frame is
 * dropped.  A file whose first audio frame points back into the bit reservoir (main_data_begin > 0: cut at the front) is refused
 * with SS_ERR_BITSTREAM by the whole-file calls, where some decoders output silence for the granules they cannot decode and go on;
 * a stream captured mid-stream is what ss_mp3_stream with join != 0 is for (below).  Nothing is read outside
 * [h_data, h_data + n_bytes). */
typedef struct ss_mp3_info {
  int32_t version;           /* 1 = MPEG-1, 2 = MPEG-2 LSF, 25 = MPEG-2.5 */
  int32_t sample_rate, channels;
  int32_t frames;            /* audio frames (a Xing / Info frame is not counted) */
  int32_t granules;          /* granules per channel: frames x (2 for MPEG-1, 1 otherwise); 576 samples each */
  int32_t granule_channels;  /* records ss_mp3_unpack writes: granules x channels */
  int64_t samples;           /* per channel, after the gapless trim */
  int32_t delay, padding;    /* from the LAME tag; -1 without one */
  int32_t skip;              /* samples trimmed at the start */
  int32_t sr_index;          /* 0..8: 44.1, 48, 32, 22.05, 24, 16, 11.025, 12, 8 kHz */
} ss_mp3_info;

/* One granule-channel: everything the device stage needs besides q[576].  Records are ordered (granule, channel). */
typedef struct ss_mp3_granule {
  int16_t global_gain;
  int16_t nz;                /* lines [nz, 576) of q are zero */
  uint8_t scalefac_scale, preflag, block_type, mixed;
  uint8_t ms;                /* MS stereo in this granule */
  uint8_t sr_index;
  uint8_t subblock_gain[3];
  uint8_t pad0[3];
  uint8_t sf_l[22];          /* long-block scalefactors (band 21: 0) */
  uint8_t sf_s[13][3];       /* short-block scalefactors [band][window] (band 12: 0) */
  uint8_t pad1[3];
} ss_mp3_granule;            /* 80 bytes */

/* One file of a ss_mp3_synthesize batch. */
typedef struct ss_mp3_file {
  int64_t rec_offset;        /* index of the file's first record in d_q / d_rec */
  int64_t out_offset;        /* first float of the file's output in d_out */
  int32_t granules;          /* granules per channel (ss_mp3_info.granules) */
  int32_t channels;          /* 1 or 2 */
  int32_t skip;              /* samples dropped at the start (ss_mp3_info.skip) */
  int32_t n_out;             /* samples written per channel (ss_mp3_info.samples) */
} ss_mp3_file;               /* 32 bytes */

/* Parse the container and every frame header (no Huffman decoding).  Host only. */
int ss_mp3_probe(const uint8_t* h_data, size_t n_bytes, ss_mp3_info* h_info);
/* Decode the bitstream: h_q [granule_channels][576] quantised lines, h_rec [granule_channels] records, h_bits (may be NULL)
 * [granule_channels] bits of main data each granule-channel consumed (scalefactors + Huffman; <= its part2_3_length).
 * cap = records the buffers hold (SS_ERR_CAPACITY if fewer than the stream has).  Host only. */
int ss_mp3_unpack(const uint8_t* h_data, size_t n_bytes, int64_t cap, int16_t* h_q, ss_mp3_granule* h_rec, int32_t* h_bits);
/* Device stage over a ragged batch: d_q / d_rec hold n_rec records of all files, h_files [n_files] (host, read before the call
 * returns) says where each file's records start and where its float32 PCM goes: planar [channels][n_out] at out_offset, or with
 * mono != 0 the channel mean [n_out].  Not clipped, not rounded.  Each file's synthesis history starts at zero, so a file
 * decodes to the same bits alone or in any batch.  d_work: caller-allocated workspace; with d_work == NULL only *work_bytes is
 * set (the size query).  Stream-ordered, two kernels, no host round trip. */
int ss_mp3_synthesize(void* stream, const int16_t* d_q, const ss_mp3_granule* d_rec, int64_t n_rec,
                      const ss_mp3_file* h_files, int n_files, int mono, float* d_out, int64_t out_floats,
                      void* d_work, size_t* work_bytes);

/* MP3 streams (streamspeech_amd/mp3.py Mp3StreamDecoder): the decoder above, resumable.  A service that takes
 * compressed audio off a socket pushes the bytes as they arrive, in chunks of any size (0 and 1 byte included); every frame a chunk
 * completes comes out as the records and q rows ss_mp3_unpack would have written for it, in the same order, and the device stage
 * synthesises them against two granules of IMDCT blocks carried per stream -- so the PCM of a stream fed in any chunking is, bit for
 * bit, the PCM of the whole-file calls on the same bytes.  ss_mp3_probe and ss_mp3_unpack run on the same core (one pass with
 * finished = 1), so the acceptance rules cannot drift:
 *   - ID3v2 tags (+ footer) at the start are skipped, across pushes; a header is taken only when the next frame's header agrees, so a
 *     frame is released once 4 bytes past its end have arrived, or at `finished` (a complete last frame is accepted without
 *     look-ahead, a truncated one is dropped); resynchronisation over garbage is byte by byte; CRC words are skipped; a Xing / Info
 *     first frame is not audio and its LAME tag sets the gapless trim; the refusals are those of the whole-file calls.
 *   - TRAILING tags (ID3v1, APEv2) are not recognised in a stream: finding them needs the end of the file.  Their bytes go through
 *     resynchronisation like any garbage, and a last frame directly followed by one fails its look-ahead.  The bit identity with the
 *     whole-file calls holds for inputs whose end the whole-file scan does not cut.
 *   - State is bounded whatever the stream length: fewer than one maximal frame (1441 bytes) + 4 unconsumed bytes, the last 511 bytes
 *     of main data, the previous granule's scalefactors, the first accepted header, the LAME delay / padding and the count of ID3v2
 *     bytes still to skip.  ss_mp3_stream_info.buffered reports the unconsumed bytes.
 *   - A push is a transaction: one that fails (SS_ERR_BITSTREAM, SS_ERR_UNSUPPORTED, or SS_ERR_CAPACITY because `cap` records are too
 *     few) leaves the object exactly as it was, so the same bytes can be pushed again with larger buffers, or other bytes instead.
 *     ss_mp3_stream_bound gives a `cap` that always suffices for a chunk of n_bytes.
 *   - join != 0 at create: a frame whose main_data_begin reaches back before the first main-data byte this object received is not
 *     decoded and yields no records (its main data still enters the reservoir; skipped_frames counts it); decoding starts at the
 *     first frame that is wholly decodable.  With join == 0 such a stream is refused with SS_ERR_BITSTREAM, as by the whole-file calls.
 *   - Gapless: with a LAME tag the first delay + 529 decoded samples are never released and the last max(0, padding - 529) decoded so
 *     far are held back (at `finished` they are the encoder's padding and are dropped); without a tag nothing is trimmed or held.
 *     `samples` counts the released ones: at `finished` it equals ss_mp3_info.samples of the same bytes.
 * Host only, no HIP call, no global mutable state; one object is driven by one thread at a time.  After a push with finished != 0
 * the object takes no more data until it is reset (SS_ERR_ARG). */
typedef struct ss_mp3_stream ss_mp3_stream;

typedef struct ss_mp3_stream_info {
  int32_t version;           /* as ss_mp3_info, of the first accepted header; 0 before one was accepted */
  int32_t sample_rate, channels, sr_index;
  int32_t delay, padding;    /* from the LAME tag; -1 without one */
  int32_t skip;              /* decoded samples never released at the start: delay + 529, or 0 */
  int32_t hold;              /* decoded samples held back at the end: max(0, padding - 529), or 0 */
  int32_t buffered;          /* unconsumed bytes the object keeps (< 1441 + 4) */
  int32_t finished;
  int64_t frames;            /* audio frames decoded so far */
  int64_t granules;          /* granules per channel decoded so far; 576 samples each */
  int64_t samples;           /* per channel, released so far: max(0, 576 granules - skip - hold) */
  int64_t skipped_frames;    /* join: frames passed over because their main data began before the stream was joined */
  int64_t bytes_in;          /* bytes of all successful pushes */
} ss_mp3_stream_info;        /* 80 bytes */

int ss_mp3_stream_create(int join, ss_mp3_stream** out);
void ss_mp3_stream_destroy(ss_mp3_stream* s);
int ss_mp3_stream_reset(ss_mp3_stream* s);                   /* a fresh stream; join stays as created */
/* Records a push of n_bytes can write at most, given what the object holds now (2 records per 24 bytes: the shortest frame). */
int64_t ss_mp3_stream_bound(const ss_mp3_stream* s, size_t n_bytes);
/* Consume h_data [n_bytes] (may be NULL when n_bytes == 0) and write the records of every frame the chunk completes: h_q [cap][576],
 * h_rec [cap], h_bits [cap] (may be NULL), *n_rec of them, ordered and laid out as by ss_mp3_unpack.  h_info (may be NULL): the state
 * after the push, or the unchanged state when it fails. */
int ss_mp3_stream_push(ss_mp3_stream* s, const uint8_t* h_data, size_t n_bytes, int finished, int64_t cap, int16_t* h_q,
                       ss_mp3_granule* h_rec, int32_t* h_bits, int64_t* n_rec, ss_mp3_stream_info* h_info);
int ss_mp3_stream_query(const ss_mp3_stream* s, ss_mp3_stream_info* h_info);
/* dst becomes an exact copy of src's state (under 2.5 KB): a caller that may have to take a SUCCESSFUL push back -- a session pool
 * that learns only from the push how many samples it releases, and then refuses it for capacity -- copies first and copies back. */
int ss_mp3_stream_copy(ss_mp3_stream* dst, const ss_mp3_stream* src);

/* One stream's share of a ss_mp3_stream_synthesize call: `granules` new granules (x channels records from rec_offset on). */
typedef struct ss_mp3_stream_seg {
  int64_t rec_offset;        /* index of the segment's first record in d_q / d_rec */
  int64_t dst_offset;        /* samples into destination h_dst[dst] where the first written sample goes */
  int64_t ch_stride;         /* planar output (mono == 0): channel c is written ch_stride floats after channel 0 */
  int32_t granules;          /* new granules per channel; 0: the segment costs nothing and changes nothing */
  int32_t channels;          /* 1 or 2 */
  int32_t skip;              /* samples of these granules dropped at the front (what is left of the gapless skip), <= 576 granules */
  int32_t history;           /* granules the stream decoded before these, saturated at 2: how much of d_state is read */
  int32_t dst;               /* index into h_dst */
  int32_t pad0;
} ss_mp3_stream_seg;         /* 48 bytes */

/* Device stage of the streams of one step, a ragged batch: requantisation ... IMDCT of the new granules (the kernel of
 * ss_mp3_synthesize), then synthesis of each against its stream's carried blocks, then the carried blocks move on -- three launches
 * and one table upload whatever n_segs is, stream-ordered, no host round trip.  h_state[i] is segment i's device state, [2][channels]
 * [1152] floats: the IMDCT blocks of the stream's last two granules (older first), which the synthesis of a granule overlap-adds
 * and whose last 15 time slots stand in front of it; only `history` of them are read, so a new stream's state need not be zeroed and
 * a first granule is formed exactly as the whole-file kernel forms it (no 0 + -0).  After the call the state holds the blocks of the
 * last two granules again ({old last, new} after a single new granule).  Two segments must not share a state.  Segment i writes
 * samples [dst_offset, dst_offset + 576 granules - skip) of h_dst[dst] -- the channel mean with mono != 0, else planar with ch_stride
 * -- and nothing else; h_dst_cap[i] is the capacity of h_dst[i] in floats.  Per sample the arithmetic is that of ss_mp3_synthesize
 * (one device function serves both kernels), so a stream decodes to the same bits in any chunking, alone or in any batch.
 * h_segs, h_state, h_dst and h_dst_cap are host memory read before the call returns.  d_work as for ss_mp3_synthesize.  Every refusal
 * is made before any HIP call, for the whole call: SS_ERR_ARG for a negative count, channels not 1 or 2, history outside [0, 2], skip
 * outside [0, 576 granules], a negative offset or stride, dst outside [0, n_dst), records past n_rec, a NULL state of a segment with
 * granules, a NULL destination of a segment that writes; then SS_ERR_CAPACITY for a destination range past h_dst_cap[dst]. */
int ss_mp3_stream_synthesize(void* stream, const int16_t* d_q, const ss_mp3_granule* d_rec, int64_t n_rec,
                             const ss_mp3_stream_seg* h_segs, int n_segs, float* const* h_state, float* const* h_dst,
                             const int64_t* h_dst_cap, int n_dst, int mono, void* d_work, size_t* work_bytes);

/* FLAC ingest: the audio format of every fairseq S2T / S2S preparation script (`sf.write(..., ".flac")`,
 * the members of src_flac.zip).  Two stages, split as the MP3 ingest is: the host stage (csrc/flac_host.hip) reads the container, the
 * metadata chain, every frame header (CRC-8 checked) and every subframe (Rice / escape residuals; frame CRC-16 checked) and writes one
 * ss_flac_subframe record per subframe, ordered (frame, channel), plus one int32 per sample into h_res; the device stage
 * (csrc/flac.hip) undoes the predictor, the wasted-bits shift and the inter-channel decorrelation and writes float32 PCM,
 * float(s) * 2^-(bps-1): for a 16-bit file frontend.read_wav's bits on the same samples.  ss_flac_restore_host is the device stage's
 * arithmetic on the host (csrc/flac.hpp holds what both share).
 * h_res of a subframe (block_size places from res_offset): warm-up samples in the first `order` places, residuals after them; a
 * constant subframe's value at place 0 (the other places are zero); verbatim samples whole.
 * Refused with SS_ERR_BITSTREAM (6): a CRC mismatch, lost sync, an order above the block size, a partition order that does not divide the
 * block or leaves the first partition shorter than the order, a negative qlp shift, reserved codes, a frame that disagrees with
 * STREAMINFO on rate, channels or depth, a missing or misplaced STREAMINFO.  SS_ERR_UNSUPPORTED (7): more than 24 bits per sample, Ogg
 * encapsulation.  A truncated last frame is dropped; fewer frames than STREAMINFO declares are accepted and the counted samples win.
 * The host stage has no global mutable state, makes no HIP call and reads nothing outside [h_data, h_data + n_bytes). */
typedef struct ss_flac_info {
  int32_t sample_rate, channels, bits_per_sample;
  int32_t frames;            /* complete frames */
  int64_t subframes;         /* records ss_flac_unpack writes: the sum of the frames' channels */
  int64_t samples;           /* per channel, counted from the frames */
  int64_t total_samples;     /* STREAMINFO's declared total; 0 = unknown */
  int32_t min_block, max_block;  /* STREAMINFO */
  uint8_t md5[16];           /* STREAMINFO: MD5 of the interleaved little-endian PCM; all zero = not set */
} ss_flac_info;              /* 64 bytes */

enum { SS_FLAC_CONSTANT = 0, SS_FLAC_VERBATIM = 1, SS_FLAC_FIXED = 2, SS_FLAC_LPC = 3 };
enum { SS_FLAC_INDEPENDENT = 0, SS_FLAC_LEFT_SIDE = 1, SS_FLAC_RIGHT_SIDE = 2, SS_FLAC_MID_SIDE = 3 };

typedef struct ss_flac_subframe {
  int64_t res_offset;        /* int32 places into h_res / d_res */
  int64_t sample_start;      /* the frame's first sample in its file (per channel), counted */
  int32_t block_size;
  uint8_t type;              /* SS_FLAC_CONSTANT .. SS_FLAC_LPC */
  uint8_t order;             /* 0-4 fixed, 1-32 lpc, 0 otherwise */
  uint8_t bps;               /* the subframe's bits per sample: the frame's, + 1 for a side channel (wasted bits not taken off) */
  uint8_t wasted;
  uint8_t shift;             /* qlp shift (0 for fixed) */
  uint8_t assignment;        /* SS_FLAC_INDEPENDENT .. SS_FLAC_MID_SIDE, of the frame */
  uint8_t precision;         /* bits of a coefficient (lpc: as coded; fixed: 4) */
  uint8_t channel;
  int32_t reserved;
  int16_t coef[32];          /* lpc: as coded; fixed: the binomial taps of the order; zero past `order` */
} ss_flac_subframe;          /* 96 bytes */

/* One file of a ss_flac_restore batch. */
typedef struct ss_flac_file {
  int64_t rec_offset;        /* first record of the file in d_rec */
  int64_t out_offset;        /* first float of the file in d_out */
  int32_t frames;            /* frames (channels records each) */
  int32_t channels;          /* 1-8 */
  int32_t bps;               /* bits per sample of the file, 4-24 */
  int32_t n_out;             /* samples written per channel (ss_flac_info.samples) */
} ss_flac_file;              /* 32 bytes */

/* STREAMINFO only (marker, ID3v2 skip, first metadata block): frames / subframes / samples are left 0.  Host only. */
int ss_flac_streaminfo(const uint8_t* h_data, size_t n_bytes, ss_flac_info* h_info);
/* The whole container: metadata chain and every frame, as ss_flac_unpack walks them, without output.  Host only. */
int ss_flac_probe(const uint8_t* h_data, size_t n_bytes, ss_flac_info* h_info);
/* h_rec [cap] and h_res [res_cap] (SS_ERR_CAPACITY if the stream has more subframes than cap or more samples x channels than
 * res_cap).  h_info may be NULL.  Host only. */
int ss_flac_unpack(const uint8_t* h_data, size_t n_bytes, int64_t cap, int32_t* h_res, ss_flac_subframe* h_rec, int64_t res_cap,
                   ss_flac_info* h_info);
/* The device stage's arithmetic on the host.  h_out (may be NULL): as d_out of ss_flac_restore.  h_pcm (may be NULL): the exact
 * integer PCM, planar [channels][n_out] per file, the files one after another in order (what a caller hashes).  Host only. */
int ss_flac_restore_host(const int32_t* h_res, const ss_flac_subframe* h_rec, int64_t n_rec, const ss_flac_file* h_files, int n_files,
                         int mono, float* h_out, int32_t* h_pcm);
/* A ragged batch of files in ONE launch, stream-ordered, no host round trip: file i writes d_out[out_offset ..): planar
 * [channels][n_out], or with mono != 0 [n_out], the ascending-channel float32 sum times 1 / channels ((l + r) * 0.5f for stereo).
 * Integer results are those of exact integer arithmetic: a 32-bit accumulator only where bps - wasted + precision + ceil(log2(order))
 * <= 32 proves it equal (libFLAC's rule), 64 bits otherwise.  d_work == NULL: *work_bytes = the workspace the call needs, nothing
 * else happens; otherwise *work_bytes is the size of d_work (SS_ERR_CAPACITY if too small).  h_files is read before the call returns.
 * Refusals before any HIP call: SS_ERR_ARG for channels outside [1, 8], bps outside [4, 24], negative counts or offsets, records past
 * n_rec; SS_ERR_CAPACITY for an output range past out_floats.  Records are checked on the device: a record whose block does not fit
 * its file (sample_start + block_size > n_out), or whose order exceeds 32 or its block, writes nothing. */
int ss_flac_restore(void* stream, const int32_t* d_res, const ss_flac_subframe* d_rec, int64_t n_rec, int64_t n_res,
                    const ss_flac_file* h_files, int n_files, int mono, float* d_out, int64_t out_floats,
                    void* d_work, size_t* work_bytes);

/* Binary PCM in and out of the session pools (streamspeech_amd/pcm.py): a service that takes audio off a socket
 * holds 16-bit PCM, float32 or G.711 bytes, not SimulEval's lists of Python floats.  A pool step copies every chunk it was pushed into
 * ONE pinned staging buffer, uploads that once, and ss_pcm_scatter decodes all chunks into the sessions' float32 sample histories in
 * one launch; ss_pcm_pack_s16 turns the step's synthesised speech into 16-bit PCM in one launch, for one download.
 * Conversions (one inline function each, csrc/pcm.hpp, shared by the kernels and the host entry points; all little-endian):
 *   s16le   mono (float)s * 2^-15; stereo ((float)l + (float)r) * 2^-16 -- frontend.read_wav's bits, channel mean included
 *   f32le   mono: the bits are copied (NaN payloads, -0.0, denormals); stereo (l + r) * 0.5f
 *   ulaw / alaw   the G.711 expansion to the 16-bit linear value (mu-law 0x00 -> -32124, A-law 0x2A -> -32256), then as s16le
 *   pack    NaN -> 0, else rintf(fminf(fmaxf(x, -1), 1) * 32767), half to even -- frontend.write_wav's bits */
enum { SS_PCM_F32LE = 0, SS_PCM_S16LE = 1, SS_PCM_ULAW = 2, SS_PCM_ALAW = 3 };

/* One chunk of a ss_pcm_scatter call. */
typedef struct ss_pcm_seg {
  int64_t src_offset;        /* bytes into the staging buffer, a multiple of 16 */
  int64_t dst_offset;        /* samples into destination h_dst[dst] */
  int32_t frames;            /* sample frames (per channel) */
  int32_t fmt, channels, dst; /* SS_PCM_*; 1 or 2, interleaved; index into h_dst */
} ss_pcm_seg;                /* 32 bytes */

/* Decode n_segs chunks of the device staging buffer d_stage [stage_bytes] into the device float32 buffers h_dst[0 .. n_dst) (capacity
 * h_dst_cap[i] samples each): segment i writes samples [dst_offset, dst_offset + frames) of h_dst[dst] and nothing else.  h_segs,
 * h_dst and h_dst_cap are host memory read before the call returns.  One launch, stream-ordered, no host round trip; the device copy
 * of the table is a buffer the library keeps per stream.  Every refusal is made before any HIP call, for the whole call: first, over
 * all segments in order, SS_ERR_ARG for n_segs < 0, a fmt outside the enum, channels not 1 or 2, frames < 0, src_offset negative or
 * not a multiple of 16, dst outside [0, n_dst), dst_offset < 0; then, over all segments in order, SS_ERR_CAPACITY for a source range
 * past stage_bytes or a destination range past h_dst_cap[dst].  n_segs == 0: SS_OK, no launch. */
int ss_pcm_scatter(void* stream, const void* d_stage, int64_t stage_bytes, const ss_pcm_seg* h_segs, int n_segs,
                   float* const* h_dst, const int64_t* h_dst_cap, int n_dst);
/* d_out[i] = 16-bit PCM of d_src[i], i < n (device buffers).  One launch, stream-ordered.  n < 0: SS_ERR_ARG; n == 0: SS_OK, no launch. */
int ss_pcm_pack_s16(void* stream, const float* d_src, int64_t n, int16_t* d_out);
/* The conversions on the host, from the same inline functions: `frames` frames at h_src -> h_dst [frames].  Host only, no HIP call. */
int ss_pcm_decode_host(const void* h_src, int fmt, int channels, int64_t frames, float* h_dst);
int ss_pcm_pack_s16_host(const float* h_src, int64_t n, int16_t* h_out);

/* Speech OUT at the caller's sample rate and format (streamspeech_amd/pcm.py PcmOut): the streaming output
 * resampler.  A session's 16-kHz float32 output of the current utterance is y[0 .. N); z = ss_resample(y) by up / down (lowest
 * terms, taps [2 * half + 1] = design_filter(up, down), half = 10 * max(up, down)) is its output at the caller's rate.  Output
 * sample k is settled once its FIR window no longer reaches past y, so after N samples an unfinished utterance has emitted the
 * first K(N) = 0 if N * up - 1 - half < 0, else (N * up - 1 - half) / down + 1 samples of z, and a finished one all
 * ceil(N * up / down), zero-padded past N as ss_resample pads.  Every sample is resample_sample's own sum (csrc/fbank.hpp: taps in
 * ascending m, one fmaf each), so the concatenated output of a stream cut anywhere is encode(ss_resample(y)) byte for byte.  Between
 * calls a session keeps the last min((2 * half) / up, N) samples of y in a device carry buffer; with up == down nothing is
 * filtered and nothing is kept.  Encodings (csrc/pcm.hpp): s16le the pack above; f32le the float's bits, unclipped; ulaw / alaw
 * the pack, then the ITU-T G.711 compression of that 16-bit value (the codes of CPython's audioop.lin2ulaw / lin2alaw). */
typedef struct ss_pcm_emit_seg {
  float* carry;              /* the session's carry buffer, room for (2 * half) / up samples: read, then rewritten by the call */
  const float* tail;         /* the n_new samples y[n_before .. n_before + n_new), where they lie */
  const float* taps;         /* [2 * half + 1]; not read when up == down */
  int64_t n_before;          /* N before this call */
  int64_t k0, k1;            /* the call writes samples [k0, k1) of z */
  int64_t out_offset;        /* bytes into the output buffer, a multiple of 16 */
  int32_t carry_len;         /* samples in carry on entry: min((2 * half) / up, n_before); 0 when up == down */
  int32_t n_new;
  int32_t up, down, half;
  int32_t fmt;               /* SS_PCM_* */
  int32_t finished;          /* != 0: the utterance ends with this call */
  int32_t reserved;          /* 0 */
} ss_pcm_emit_seg;           /* 88 bytes */

/* K: the samples of z settled after n samples of y (the formula above; `finished` != 0: ceil(n * up / down)).  Host only.
 * -1 for n < 0, up or down below 1, half < 0. */
int64_t ss_pcm_emit_count(int64_t n, int up, int down, int half, int finished);
/* One call per pool step for every session that answers at its own rate and format: segment i writes the (k1 - k0) *
 * sample_bytes(fmt) bytes of its samples [k0, k1) at d_out + out_offset and nothing else, and leaves in its carry buffer the last
 * min((2 * half) / up, n_before + n_new) samples of y.  Pointers of a segment are device memory; h_segs is host memory read before
 * the call returns.  Stream-ordered, no host round trip, no atomics; at most TWO launches whatever the number of segments and their
 * mix of ratios and formats: one grid computes and encodes (a workgroup owns a tile of one segment's samples, sized by the ratio,
 * and stages that segment's taps in LDS), and a second, one workgroup per segment, rewrites the carry buffers -- a launch of its
 * own because workgroups of the first still read the old carry.  The device copy of the table is a buffer the library keeps per
 * stream.  The segments' output ranges must not overlap (not checked).
 * Every refusal is made before any HIP call, for the whole call.  n_segs < 0 or a NULL h_segs: SS_ERR_ARG.  Then, over all segments
 * in order, SS_ERR_ARG for: a fmt outside the enum; up or down below 1, or (when up != down) half < 1 or taps past 64 KB; n_before
 * or n_new negative, or n_before + n_new past 2^31 - 1; carry_len other than min((2 * half) / up, n_before); k0 below
 * ss_pcm_emit_count(n_before, unfinished) (history the carry no longer holds), k1 < k0, k1 past ss_pcm_emit_count(n_before + n_new,
 * finished), more than 2^30 - 1 samples; out_offset negative or not a multiple of 16; a NULL d_out with samples to write, a NULL tail with n_new > 0, NULL taps
 * with samples to write and up != down, a NULL carry with history to read or keep.  Then, over all segments in order,
 * SS_ERR_CAPACITY for an output range past out_bytes.  n_segs == 0: SS_OK, no launch. */
int ss_pcm_emit(void* stream, const ss_pcm_emit_seg* h_segs, int n_segs, void* d_out, int64_t out_bytes);
/* The same call on host buffers (every pointer host memory), from the same inline functions: the same bytes and carries.  Host
 * only, no HIP call; the same refusals in the same order. */
int ss_pcm_emit_host(const ss_pcm_emit_seg* h_segs, int n_segs, void* h_out, int64_t out_bytes);
/* The encodings alone: n float samples at h_src -> n * sample_bytes(fmt) bytes at h_out.  Host only. */
int ss_pcm_encode_host(const float* h_src, int64_t n, int fmt, void* h_out);

/* Endpointing of live PCM streams (streamspeech_amd/endpoint.py): an energy scan over the new frames of every
 * session of a pool step, on the device where the decoded samples already lie, that cuts a continuous stream into utterances.
 * Framing is the session's own fbank framing at its source rate: frame j of the stream (counted from the session's open or reset,
 * int64) covers samples [j H, j H + W) of the +-1-scaled float32 history.  The arithmetic (csrc/vad.hpp, one set of inline
 * functions for the kernel and the host twin; float32, no libm call but fmaf, no contraction the source does not spell):
 *   power   lane l of 64 adds x[l], x[l + 64], ... in ascending order; the 64 partial sums go through the tree
 *           p[l] += p[l + o], o = 32, 16, .. 1; m = sum * (1 / W); the second pass accumulates fmaf(x - m, x - m, acc) the same way,
 *           P = sum2 * (1 / W).  Two passes, so a DC offset is not speech.
 *   frame 0 of a stream: not speech, F = max(p_min, P).
 *   else    speech = P > max(p_abs, F * snr);  F = max(p_min, min(P, F * (speech ? 1 : rise))).
 *   IDLE    a speech frame extends run (onset = j where the run begins), another zeroes it; run >= min_speech: START at onset,
 *           mode = SPEECH, utt_first_frame = onset, last_speech = j, run = 0, and the scan goes on.
 *   SPEECH  a speech frame sets last_speech = j and zeroes run, another extends run.  run >= end_silence: END, cut sample
 *           (last_speech + 1 + post_roll) H + (W - H), mode = IDLE, run = 0, the scan stops.  Otherwise
 *           j + 1 - utt_first_frame >= max_frames (the frame of a START included): FORCED, cut sample (j + 1) H + (W - H), the mode
 *           stays SPEECH, utt_first_frame = j + 1, last_speech = j, run = 0 (the next utterance begins at the cut), the scan stops.
 * All thresholds are linear power ratios; the caller converts them from dB once. */
enum { SS_VAD_IDLE = 0, SS_VAD_SPEECH = 1 };
enum { SS_VAD_START = 1, SS_VAD_END = 2, SS_VAD_FORCED = 4 };

/* A session's scan state between calls (device memory for ss_vad_scan, host memory for ss_vad_scan_host); all zero = a fresh stream. */
typedef struct ss_vad_state {
  int64_t onset;             /* first frame of the current run of speech frames (IDLE) */
  int64_t last_speech;       /* last speech frame of the utterance (SPEECH) */
  int64_t utt_first_frame;   /* frame the utterance's length is counted from */
  float floor;               /* F after the last scanned frame */
  int32_t mode;              /* SS_VAD_IDLE / SS_VAD_SPEECH */
  int32_t run;               /* speech frames in a row (IDLE), other frames in a row (SPEECH) */
  int32_t reserved;          /* 0 */
} ss_vad_state;              /* 40 bytes */

/* One session of a ss_vad_scan call. */
typedef struct ss_vad_seg {
  const float* hist;         /* the sample history; hist[0] is sample hist_first of the stream */
  ss_vad_state* state;       /* read, then rewritten by the call */
  float* powers;             /* NULL, or n_frames floats that receive P of every frame the call scanned (tests, diagnostics) */
  int64_t hist_first;        /* absolute index of hist[0] */
  int64_t n_hist;            /* samples present */
  int64_t first_frame;       /* first frame to scan */
  int32_t n_frames;          /* frames to scan at most: the scan stops early at END / FORCED */
  int32_t H, W;              /* shift and window in samples */
  float p_abs, p_min, snr, rise;
  int32_t min_speech, end_silence, post_roll, max_frames;   /* in frames */
  int32_t reserved;          /* 0 */
} ss_vad_seg;                /* 96 bytes */

typedef struct ss_vad_result {
  int64_t consumed;          /* the first frame the call did not scan */
  int64_t start_frame;       /* onset of the START the call raised, else -1 */
  int64_t cut_sample;        /* cut of the END / FORCED the call raised, else -1 */
  int64_t last_speech;       /* the state's last_speech after the call (meaningful in SPEECH and with END) */
  int32_t events;            /* SS_VAD_START | SS_VAD_END or SS_VAD_FORCED: at most one START and one stopping event */
  int32_t mode;              /* the state's mode after the call */
} ss_vad_result;             /* 40 bytes */

/* One call per pool step for every endpointed session: segment i scans frames [first_frame, first_frame + n_frames) of its history,
 * or up to its first END / FORCED, rewrites its state record and writes d_results[i] (device memory, n_segs records) and, if asked,
 * its powers -- and nothing else.  Pointers of a segment are device memory; h_segs is host memory read before the call returns.
 * ONE launch whatever the number of segments, stream-ordered, no atomics, no host round trip: a workgroup owns a segment, its waves
 * compute frame powers in parallel, in batches that go through LDS, and after each batch one lane walks the state machine over it.
 * The device copy of the table is a buffer the library keeps per stream.
 * Every refusal is made before any HIP call, for the whole call.  n_segs < 0: SS_ERR_ARG.  n_segs == 0: SS_OK, no launch.  A NULL
 * h_segs or d_results: SS_ERR_ARG.  Then, over all segments in order, SS_ERR_ARG for: a NULL state or reserved != 0; H < 1, W < 1,
 * H > W or W past 2^20; min_speech < 1, end_silence < 1, post_roll < 0, post_roll > end_silence, max_frames < 1; p_abs or p_min negative or NaN,
 * snr or rise not positive (or NaN); n_frames, n_hist, first_frame or hist_first negative, or first_frame + n_frames past 2^40;
 * a frame range whose samples the history does not hold (first_frame H < hist_first, or (first_frame + n_frames - 1) H + W past
 * hist_first + n_hist); a NULL hist with frames to scan. */
int ss_vad_scan(void* stream, const ss_vad_seg* h_segs, int n_segs, ss_vad_result* d_results);
/* The same call on host buffers (every pointer host memory), from the same inline functions: the same powers, states and results,
 * bit for bit.  Host only, no HIP call; the same refusals in the same order. */
int ss_vad_scan_host(const ss_vad_seg* h_segs, int n_segs, ss_vad_result* h_results);

/* Offline driver only: d_out[r] = max over the vocabulary, ids mask0..2 skipped (< 0: none), of
 * log_softmax(d_logits[r, :]) -- the per-position score `lprobs.max(dim=2)` of the reference's offline unit search
 * (researches/ctc_unity/ctc_generator.py:55-63: pad / unk / eos set to -inf AFTER the softmax), which fairseq-generate
 * prints as `H-`/`D-` score (their sum) and `P-` positional scores (fairseq/fairseq_cli/generate.py:274-291).
 * d_logits [rows, vocab] dense, as ss_t2u_units returns them. */
int ss_row_max_logprob(void* stream, const float* d_logits, int rows, int vocab, int mask0, int mask1, int mask2,
                       float* d_out);

/* Normalised (log-)probabilities of dense logit rows [rows, vocab] -> d_out [rows, vocab]: log_softmax (as_probs = 0) or
 * softmax (as_probs = 1) over the vocabulary, then ids mask0 / mask1 (< 0: none) set to -inf (0 for probabilities) -- what
 * the reference forms with `model.get_normalized_probs` (researches/ctc_unity/models/streamspeech_model.py via
 * fairseq_model.py:60-77) and `lprobs[:, :, pad] = lprobs[:, :, unk] = -inf` (agent/ctc_decoder.py:52-60) when a caller
 * asks the CTC decoder for `lprobs`.  Off the timed path (the greedy searches never form log-probabilities). */
int ss_log_softmax(void* stream, const float* d_logits, int rows, int vocab, int mask0, int mask1, int as_probs,
                   float* d_out);

/* ---- a2-a7: model.encoder(src_tokens, src_lengths) for one utterance (agent :433-435 ->
 * chunk_unity/models/s2t_conformer.py:111-163).  d_fbank [T,80] -> d_enc_out [T',256].
 * attn_chunk = encoder.chunk_size, conv_chunk = ChunkCausalConv1d.chunk_size as the agent sets
 * them (:395-413); values >= 999 mean "offline" (no chunking). */
int ss_encoder_out_len(int T);
int ss_encoder_forward(ss_model* m, void* stream, const float* d_fbank, int T, int attn_chunk,
                       int conv_chunk, float* d_enc_out);

/* Incremental twin for streaming (replaces the full recompute of the encoder at
 * every policy() call, agent :425-435): same inputs and output as ss_encoder_forward for the
 * fbank of ALL audio received so far, but rows that were final at the previous call (nothing they
 * can see -- chunk attention, chunk-causal convs -- can still change) are served from the handle's
 * cache and only the remaining rows go through the conformer layers.  *n_final = rows final after
 * this call, *n_computed = rows recomputed by this call (either may be NULL).  The cache belongs to
 * the handle: one utterance at a time, ss_encoder_stream_reset between utterances (the agent's
 * reset()); a change of chunk sizes or a shorter input resets it implicitly. */
int ss_encoder_stream_reset(ss_model* m);
/* Trailing fbank frames whose values may still change when more audio arrives (default 0).  The agent's
 * front-end resamples the WHOLE sample history at every call (agent :86-89, convert_waveform); a zero-padded
 * FIR recomputes its last few output samples once the future exists, so with a non-16 kHz source the newest
 * fbank frame is not settled and rows whose cone reaches it must not be cached as final: set 1. */
int ss_encoder_stream_set_tail(ss_model* m, int unsettled_fbank_frames);
int ss_encoder_stream_forward(ss_model* m, void* stream, const float* d_fbank, int T, int attn_chunk,
                              int conv_chunk, float* d_enc_out, int32_t* n_final, int32_t* n_computed);
/* Deferred time-out check (off by default).  On a scratch set that runs the persistent forms (ss_mt_set_persistent), the call above ends
 * with a stream synchronisation: it must know that none of its persistent layer launches timed out before anybody reads d_enc_out.
 * A caller that queues more work behind the encoder anyway and synchronises once for all of it -- the agent's policy(): both CTC heads,
 * then one device-to-host copy -- switches the check to deferred (on = 1): ss_encoder_stream_forward then returns without waiting, and
 * ss_encoder_stream_status waits for the stream, sets *repeat = 1 if a launch timed out (the scratch set has then left the persistent
 * form and the failed call's rows are not final any more) and 0 otherwise.  With *repeat = 1 everything computed from d_enc_out since
 * the forward call is void: call ss_encoder_stream_forward again (it now runs one launch per op and waits) and recompute.  Until the
 * status call returns 0, d_enc_out must not be trusted.  A forward call with a check still outstanding (the status call was
 * skipped) settles it first; if that check finds a time-out, the forward returns SS_ERR_STREAM_REPEAT (8) without computing
 * anything: the unchecked call's output was void, its rows are not final any more, and the caller repeats the forward exactly as
 * after *repeat = 1 (and recomputes what it derived from the void output). */
int ss_encoder_stream_set_deferred(ss_model* m, int on);
int ss_encoder_stream_status(ss_model* m, void* stream, int32_t* repeat);

/* ---- concurrent streaming sessions: one batched encoder step for many streams -----------------------------------------------
 * A pool holds the incremental-encoder state of up to max_sessions independent streams in slots: per layer the q|k|v and GLU rows,
 * the final output rows (max_rows <= max_rel_pos rows per slot, ~50 KB per row at the default sizes), the chunk sizes, the unsettled
 * tail, and the raw per-frame arg-max of both CTC heads for rows that are final.  It is created against m's scratch set: its buffers
 * are booked there (ss_scratch_bytes reports them, ss_scratch_trim keeps them -- a fixed piece like the MT cache), a pool that would
 * pass ss_scratch_set_cap fails with SS_ERR_SCRATCH_CAP and leaves the set as it was, and session state is never re-allocated by a
 * call.  The set lives until the pool is destroyed.  A pool is driven by ONE host thread at a time, like a scratch set; any handle
 * bound to the pool's scratch set may drive it.
 * ss_stream_pool_reset: the slot starts a fresh utterance.  ss_stream_pool_set_tail: as ss_encoder_stream_set_tail, per slot. */
int ss_stream_pool_create(ss_model* m, int max_sessions, int max_rows, ss_stream_pool** out);
void ss_stream_pool_destroy(ss_stream_pool* p);
int ss_stream_pool_reset(ss_stream_pool* p, int slot);
int ss_stream_pool_set_tail(ss_stream_pool* p, int slot, int unsettled_fbank_frames);
/* One encoder step of n sessions (slots h_slots[i], distinct): per slot EXACTLY the semantics of ss_encoder_stream_forward -- session
 * i passes the fbank of all its audio so far (h_fbank[i]: device pointer, h_T[i] rows of 80), rows final at its previous call come
 * from the slot, n_final follows the same finality rule (its tail included), a change of chunk sizes or a shorter input resets the slot
 * implicitly.  Sessions of one call may differ in length, chunk sizes and tail.  d_enc_packed [sum T2_i, 256] gets every session's
 * output rows in call order (session 0's T2_0 rows, then session 1's, ...) -- the packed layout of ss_batch_ctc_greedy /
 * ss_batch_mt_greedy.  h_n_final[i] / h_n_computed[i] (host, may be NULL) as in ss_encoder_stream_forward.
 * The tail rows of all sessions go through the layers as ONE row pack, one launch per op per layer whatever n, with pack-invariant
 * arithmetic: a session's rows are the same bits alone, in any pack and at any position in it.  Ordinary launches only -- no
 * persistent form, no grid-wide waits, no time-out protocol.  Bad arguments, a duplicate slot or a session with more than max_rows
 * output rows refuse the WHOLE call with SS_ERR_ARG before anything is queued; no slot changes. */
int ss_encoder_stream_forward_batch(ss_model* m, void* stream, ss_stream_pool* p, int n, const int32_t* h_slots,
                                    const float* const* h_fbank, const int32_t* h_T, const int32_t* h_attn_chunk,
                                    const int32_t* h_conv_chunk, float* d_enc_packed, int32_t* h_n_final, int32_t* h_n_computed);
/* Both-head CTC greedy search of the last step's output (head 0 = ASR, 1 = ST), outputs as ss_batch_ctc_greedy: d_raw [sum T2_i] raw
 * arg-max, d_tokens / d_index [sum T2_i] collapsed tokens and their frame index at each session's packed offset, d_counts [n].  Slots
 * h_slots in the same order as the forward that wrote d_enc_packed (their T2 are the pool's).  Rows below a slot's n_final never
 * change, so their arg-max is kept in the slot: the head GEMM and arg-max run only over rows the slot does not hold yet. */
int ss_stream_pool_ctc(ss_model* m, void* stream, ss_stream_pool* p, int head, int n, const int32_t* h_slots,
                       const float* d_enc_packed, int32_t* d_raw, int32_t* d_tokens, int32_t* d_index, int32_t* d_counts);
/* Scores of the pool's CTC calls (off at creation).  on = 1 books a float cache [2 heads][max_sessions][max_rows] beside the arg-max
 * cache on the pool's scratch set (ss_scratch_bytes reports it, ss_scratch_trim keeps it): the log-probability of each final row's
 * arg-max, the per-frame `lprobs.max(dim=2)` of agent/ctc_decoder.py:52-61.  Past ss_scratch_set_cap it returns SS_ERR_SCRATCH_CAP and
 * leaves the set as it was; on = 0 gives the bytes back.  Allowed only while no slot holds rows (before the first forward, or with
 * every used slot reset), else SS_ERR_ARG: a slot's cached arg-max and its log-probability are filled together. */
int ss_stream_pool_set_scores(ss_stream_pool* p, int on);
/* ss_stream_pool_ctc with the scores of agent/ctc_decoder.py:52-62,104-105 (`positional_scores`): outputs as
 * ss_batch_ctc_greedy_scored -- d_lprob [sum T2_i] per frame, d_last / d_tok_lprob [sum T2_i] per collapsed token at each session's
 * packed offset.  As with the arg-max, rows below a slot's n_final take their log-probability from the slot (the bits they had when
 * they became final); only the rows the slot does not hold yet go through the head.  One launch more than ss_stream_pool_ctc,
 * whatever n.  SS_ERR_ARG unless ss_stream_pool_set_scores(p, 1). */
int ss_stream_pool_ctc_scored(ss_model* m, void* stream, ss_stream_pool* p, int head, int n, const int32_t* h_slots,
                              const float* d_enc_packed, int32_t* d_raw, int32_t* d_tokens, int32_t* d_index, int32_t* d_counts,
                              float* d_lprob, int32_t* d_last, float* d_tok_lprob);
/* Test hook: the pool's counters since its creation -- kernels its calls launched (its own kernels, plus the GEMM-family launches the
 * library's launch census saw during the call: meaningful while no other thread launches), rows its CTC calls ran through a head. */
int ss_stream_pool_stats(ss_stream_pool* p, int64_t* launches, int64_t* head_rows);

/* ---- a8: CTCDecoder.generate (agent/ctc_decoder.py:39-111): head 0 = source_unigram (ASR),
 * 1 = ctc_target_unigram (ST).  Outputs (device int32): raw argmax per frame [Tp], collapsed
 * tokens / frame index [<=Tp], *d_count.  d_logits may be NULL (else [Tp,vocab] is written). */
int ss_ctc_greedy(ss_model* m, void* stream, int head, const float* d_enc_out, int Tp,
                  int32_t* d_raw, int32_t* d_tokens, int32_t* d_index, int32_t* d_count,
                  float* d_logits);

/* The same search with the scores the reference's CTCDecoder.generate returns in every hypothesis (agent/ctc_decoder.py:52-62:
 * lprobs = log_softmax(logits), pad and unk set to -inf, `positional_scores = lprobs.max(dim=2)`; :104-105 `score` is their sum, taken
 * by the caller).  d_raw / d_tokens / d_index / d_count / d_logits exactly as ss_ctc_greedy.  d_lprob [Tp] float: the log-probability
 * of each frame's arg-max, NaN for a row that holds a NaN (as torch.log_softmax).  Per collapsed token j: d_last[j] (int32) the last
 * frame of the run of equal raw ids that starts at d_index[j], d_tok_lprob[j] (float) the sum of d_lprob over that run in ascending
 * frame order.  Same number of launches as ss_ctc_greedy. */
int ss_ctc_greedy_scored(ss_model* m, void* stream, int head, const float* d_enc_out, int Tp,
                         int32_t* d_raw, int32_t* d_tokens, int32_t* d_index, int32_t* d_count,
                         float* d_logits, float* d_lprob, int32_t* d_last, float* d_tok_lprob);

/* Decode-step form of this context (the n = 1 calls of ss_mt_append / the loop inside ss_mt_greedy; reference: one
 * EnsembleModel.forward_decoder call of agent/sequence_generator.py:592-673 per generated token).  workgroups = 0 (default, or
 * the SS_MT_PERSISTENT environment variable at context creation): one launch per op, 35 dependent kernels per token.
 * workgroups = 64 | 128 | 256: the whole step as ONE persistent launch (csrc/mt_step.hip: phases exchange their output vectors
 * through agent-scope {epoch, value} granules; every wait is bounded and counted by ss_debug_sk_errors).  All workgroups of a
 * launch must become resident: meant for a context that decodes one utterance at a time on an otherwise lightly loaded
 * device (the SimulEval agent), at most 8 such contexts concurrently at 64 workgroups.
 * The setting belongs to the SCRATCH SET the handle is bound to when this is called (the granule region lives there): a handle bound
 * to another set afterwards runs with that set's setting. */
int ss_mt_set_persistent(ss_model* m, int workgroups);
/* The current setting.  It drops to 0 by itself when a launch of the persistent step times out: the kernel then publishes -1
 * as the next token, ss_mt_greedy (which reads the token chain back anyway) repeats the whole search with one launch per op and
 * says so on stderr; callers of ss_mt_append that read *d_next < 0 do the same (engine.HipModel.mt_append). */
int ss_mt_get_persistent(ss_model* m);

/* ---- a9-a10: first-pass MT decoder with KV cache (the reference re-runs it on the whole prefix
 * every step, agent/sequence_generator.py:313-346; per-position results are identical).
 * ss_mt_begin: bind encoder output, project cross-attention K/V for all layers, reset the cache.
 * ss_mt_append: feed n tokens occupying positions pos0..pos0+n-1 (position 0 is the leading
 *   </s>); writes features (post final LayerNorm, = mt_decoder(..., features_only=True)) for
 *   those positions to d_feats [n,512] if non-NULL, and the greedy next token after the LAST fed
 *   position to *d_next: argmax over the vocabulary with `pad` never selected, `eos` banned when
 *   ban_eos, and forced to eos when force_eos (agent/sequence_generator.py:350-372 at beam 1). */
int ss_mt_begin(ss_model* m, void* stream, const float* d_enc_out, int Tp);
int ss_mt_append(ss_model* m, void* stream, const int32_t* d_tokens, int n, int pos0, int ban_eos,
                 int force_eos, float* d_feats, int32_t* d_next, int n_tail_pad);
/*   n_tail_pad: the last n_tail_pad fed tokens are <pad> (whole-word mode feeds one, agent :576-584):
 *   they take the zero positional row and are masked as keys (fairseq self_attn_padding_mask). */
/* The whole beam-1 search of SequenceGenerator.generate_decoder (agent/sequence_generator.py:165-582)
 * in one call: begin + prefix pass + autoregressive steps until </s> or max_len (forced </s>), with
 * the token chain kept on the device.  h_prefix [n_prefix] host ids (no leading </s>).
 * h_out_tokens (host, >= max_len+1-n_prefix ints) receives the tokens generated after the prefix,
 * including the final </s>; d_feats [max_len+2, dec_dim] receives the decoder states of every fed
 * position; *h_n_feats = number of valid rows = 1 + n_prefix + (*h_n_out - 1).  Synchronises. */
int ss_mt_greedy(ss_model* m, void* stream, const float* d_enc_out, int Tp, const int32_t* h_prefix,
                 int n_prefix, int max_len, int min_len, int32_t* h_out_tokens, int* h_n_out,
                 float* d_feats, int* h_n_feats);
/* Truncate the self-attention cache to `len` positions (whole-word rollback, agent :540-574). */
int ss_mt_truncate(ss_model* m, int len);

/* ---- a11-a13: synthesizer_encoder + CTCTransformerUnitDecoder + CTC unit search
 * (agent :661-717).  d_mt_feats [n,512] -> raw argmax [25n], collapsed unit-vocabulary tokens
 * (blank 1004 / pad dropped) and *d_count; d_logits optional [25n,1005].  t2u_causal = the
 * checkpoint's --uni-encoder flag; mask_eos = the offline generator's extra eos mask
 * (researches/ctc_unity/ctc_generator.py:58). */
int ss_t2u_units(ss_model* m, void* stream, const float* d_mt_feats, int n, int t2u_causal,
                 int mask_eos, int32_t* d_raw, int32_t* d_tokens, int32_t* d_count, float* d_logits,
                 int n_tail_pad);
/*   n_tail_pad: trailing rows of d_mt_feats that belong to <pad> tokens: masked as keys in the T2U
 *   encoder, the unit decoder's self-attention (25 positions each) and its cross-attention, but
 *   still decoded (the reference emits their units too, agent :661-717). */

/* ---- a14-a15: CodeHiFiGANVocoderWithDur.forward (agent/tts/vocoder.py:48-60). -------------- */
/* d_blob must be device-visible when this is called (the upload complete, not merely queued on some stream): the Winograd forms
 * of the ResBlock conv weights are made here on the null stream (once per blob and device -- later contexts over the same blob
 * borrow them) and the call returns with the device synchronised.  The same holds for ss_model_create (projected rel-pos table). */
int ss_vocoder_create(const ss_vocoder_config* cfg, const float* d_blob, size_t blob_floats,
                      const char* const* names, const int64_t* offsets, const int64_t* numels,
                      int n_slots, ss_vocoder** out);
void ss_vocoder_destroy(ss_vocoder* v);
/* Optional, OFF by default (the default path is exact f32, the reference's arithmetic).  on != 0: the C >= 64 generator
 * convs of this handle (hifigan.py:52-172) contract with three bf16 MFMAs per k-slice on operands split into
 * bf16(x) + bf16(x - bf16(x)) (16 significant bits), f32 accumulation -- waveform within 1e-3 RMS of the f32 path
 * (tests/test_bf16x3_gpu.py), durations untouched (the duration predictor and every argmax stage stay f32). */
int ss_vocoder_set_bf16x3(ss_vocoder* v, int on);
/* Optional, OFF by default; off is bit for bit the default exact-f32 path.  on != 0: every ResBlock conv of this handle's 64-, 128-
 * and 256-channel generator stages (54 convs per forward with the default plan) runs on the FP16 matrix cores (csrc/conv_f16.hip):
 * activations and weights rounded to FP16 (saturated to +-65504, never inf), f32 accumulation, f32 tensors in memory, at every row
 * count and in every entry point (single utterance, ragged batch, tail).  Stay f32: conv_pre, the up-convs, the 32- and 16-channel
 * stages, conv_post, the duration predictor (so durations are those of the f32 path) and everything upstream of the vocoder.
 * Bars: waveform within 1e-3 RMS of the f32 path and of the FP32 oracle (tests/test_vocoder_f16_gpu.py); an output row's bits depend
 * only on its receptive field, not on the pack.  FP16 wins over ss_vocoder_set_bf16x3 while both are on.  The first switch-on makes
 * the FP16 weight fragments (once per blob and device, shared like the Winograd forms): the pack runs on the null stream and the call
 * returns with the device synchronised.  SS_ERR_ARG (the handle unchanged) when a wide-stage ResBlock conv of the handle's plan does
 * not fit the kernel: (kernel size - 1) x dilation above 64. */
int ss_vocoder_set_f16(ss_vocoder* v, int on);
/* d_codes [K] int32 unit ids (0..999).  dur_prediction != 0 runs the duration predictor, else every
 * unit lasts one frame; d_forced_dur (may be NULL) overrides both.  d_wav must hold
 * wav_capacity floats; *h_n_samples = 320 * sum(dur).  d_dur [K] int32.  Synchronises once
 * (the frame count sizes the generator launches). */
int ss_vocoder_forward(ss_vocoder* v, void* stream, const int32_t* d_codes, int K, int dur_prediction,
                       const int32_t* d_forced_dur, float* d_wav, int64_t wav_capacity,
                       int32_t* d_dur, int64_t* h_n_samples);
/* ---- multi-speaker vocoders ("multispkr": true, agent/tts/codehifigan.py:13-19, 80-86) ---------------------------------------
 * The reference concatenates the chosen speaker's embedding, repeated over all frames, to the code embeddings in front of conv_pre
 * (2 x embedding_dim input channels).  The speaker vector is constant over time, so here conv_pre contracts the code half only
 * ("voc.pre.w", Cin = embedding_dim -- ss_vocoder_config.model_in_dim stays that width) and one more launch adds the speaker term
 * before the activation: slot "voc.spkr.table", [num_speakers][16][upsample_initial_channel] floats.  With W the weight-norm-folded
 * conv_pre weight [C0][2E][7], s the speaker's embedding and G[k][co] = sum_c W[co][E + c][k] * s[c], entry (lo, hi) of a speaker
 * holds G[lo] + G[lo + 1] + ... + G[hi] (ascending tap order, summed in float64 at packing time and rounded to float32 once) at
 * index 4 * lo + (hi - 3), lo in 0..3, hi in 3..6.  Row t of a segment of L frames takes lo = max(0, 3 - t), hi = min(6, L + 2 - t):
 * the taps of the 7-tap "same" conv that fall inside the segment.  Per row the device work is ONE float32 add of a table entry to
 * conv_pre's output (then the leaky-ReLU the first up-conv reads), so the path is as pack-invariant as the single-speaker one.
 * A handle is multi-speaker when its blob carries that slot; num_speakers = the slot's size / (16 x upsample_initial_channel).
 * The duration predictor does not see the speaker.
 * Refusals, all SS_ERR_ARG before any HIP call: a _spkr call with an id outside [0, num_speakers); a _spkr call on a single-speaker
 * handle; a no-speaker call (ss_vocoder_forward, ss_batch_vocoder_forward, ss_batch_vocoder_tail) on a multi-speaker handle (the
 * reference asserts 'require "spkr" input'). */
int ss_vocoder_num_speakers(const ss_vocoder* v);   /* 0: a single-speaker handle */
/* ss_vocoder_forward in the voice of speaker `spkr`. */
int ss_vocoder_forward_spkr(ss_vocoder* v, void* stream, const int32_t* d_codes, int K, int dur_prediction,
                            const int32_t* d_forced_dur, float* d_wav, int64_t wav_capacity,
                            int32_t* d_dur, int64_t* h_n_samples, int32_t spkr);

/* ---- ragged-batch twins (BASELINE.json configs[3]/[4]: many utterances per GPU) --------------
 * B independent utterances packed along the row axis (no padding; each keeps the B = 1 arithmetic
 * of the entry points above -- SURVEY.md H2b).  h_* arrays are host arrays of length B; packed
 * device buffers are the concatenation of the per-utterance arrays in batch order. */
/* ss_fbank_cmvn over a pack: utterance b is the h_n_samples[b] samples at d_pcm + h_pcm_start[b]; its h_T[b] =
 * ss_fbank_num_frames(h_n_samples[b]) rows follow those of utterance b - 1 in d_feat (an utterance of fewer than 400 samples has
 * none), each the same bits as ss_fbank_cmvn on that utterance alone.  Any B >= 1: the segment table is launched in slices of at
 * most 65535 utterances (the grid's y extent), so a pack past that is several launches on the stream, not a refusal.
 * SS_ERR_ARG, decided for the whole call before anything is launched or written (h_T included): B < 1; a null d_pcm, d_feat,
 * h_pcm_start, h_n_samples or h_T; a negative h_n_samples[b] or h_pcm_start[b]; an h_pcm_start[b] or a total row count past
 * 2^31 - 1 (the kernel's segment fields are ints). */
int ss_batch_fbank_cmvn(ss_model* m, void* stream, int B, const float* d_pcm, const int64_t* h_pcm_start,
                        const int32_t* h_n_samples, float pcm_scale, float* d_feat, int32_t* h_T);
/* Precomputed fbank rows (the recipe's src_fbank80.zip): d_out[r][c] = (d_in[r][c] - mean[c]) / std[c] over `rows` packed rows of 80
 * raw log-mel bins, written exactly as the last line of the fbank kernel, with the model's global-CMVN vectors (a model without
 * stats behaves as ss_batch_fbank_cmvn does without them).  One launch, stream-ordered; d_out may be d_in.  rows == 0: SS_OK. */
int ss_batch_cmvn(ss_model* m, void* stream, const float* d_in, int64_t rows, float* d_out);
int ss_batch_encoder_forward(ss_model* m, void* stream, int B, const float* d_fbank, const int32_t* h_T,
                             int attn_chunk, int conv_chunk, float* d_enc_out, int32_t* h_Tp);
int ss_batch_ctc_greedy(ss_model* m, void* stream, int head, int B, const float* d_enc_out,
                        const int32_t* h_Tp, int32_t* d_raw, int32_t* d_tokens, int32_t* d_index,
                        int32_t* d_counts);
/* ss_batch_ctc_greedy with the scores of ss_ctc_greedy_scored (agent/ctc_decoder.py:52-62), under the same pack-invariance setting:
 * d_lprob [sum Tp] per frame, d_last / d_tok_lprob [sum Tp] per collapsed token, packed like d_raw and d_tokens. */
int ss_batch_ctc_greedy_scored(ss_model* m, void* stream, int head, int B, const float* d_enc_out,
                               const int32_t* h_Tp, int32_t* d_raw, int32_t* d_tokens, int32_t* d_index,
                               int32_t* d_counts, float* d_lprob, int32_t* d_last, float* d_tok_lprob);
/* ---- CTC forced alignment and scoring of a GIVEN label sequence on a text head (csrc/ctc_align.hip): where do these labels lie in
 * this audio, and how likely does the model find them -- the CTC criterion's log p(y | x) (plain log_softmax, blank = 0, no pad / unk
 * masking, so a word mapped to <unk> can still be placed; fairseq criterions/ctc.py) and its best path.  The extended sequence is
 * [0, y0, 0, y1, ..., y(L-1), 0]; a path stays, advances by one state, or skips the blank between two different labels. ---- */
typedef struct ss_ctc_align_result {
  double score;      /* log p(y | x): the forward sum over every path, float64 state over the float32 per-frame log-softmax */
  double viterbi;    /* the log-probability of the best path, the one d_path / d_first / d_last describe */
  int32_t status;    /* 0 aligned; 1 infeasible (T' < L + number of adjacent equal labels, or every path has probability 0); 2 a NaN in
                      * a row of the utterance */
  int32_t n_tokens;  /* L */
} ss_ctc_align_result;
#define SS_CTC_ALIGN_MAX_FRAMES 1500    /* T' per utterance (max_source_positions = 6000 fbank frames) */
#define SS_CTC_ALIGN_MAX_LABELS 1500    /* L per utterance */
/* B utterances packed as ss_batch_ctc_greedy_scored takes them (the same head GEMM, pack-invariance setting and workspace), labels
 * h_targets packed in the same order, h_n_targets[b] of them for utterance b (0 is legal: the score is the all-blank path).  Device
 * outputs: d_results [B]; d_path [sum Tp] the token id of the best path per frame, 0 = blank (may be NULL); per label j, packed like
 * h_targets: d_first[j] / d_last[j] the first and last frame of its run on the path (relative to its utterance), d_tok_lprob[j] the
 * float32 sum of the per-frame log-probability over that run in ascending frame order (the promise of ss_ctc_greedy_scored's
 * d_tok_lprob).  Ties: stay beats advance beats skip; at the end the trailing blank beats the last label.  status 1: score = viterbi
 * = -inf, path / first / last -1, tok_lprob NaN; status 2: the scores NaN, the rest as status 1.  An utterance's outputs are the same
 * bits alone and in any pack, in any order.  SS_ERR_ARG, with nothing launched or written: a label that is blank (0), pad, negative
 * or >= the head's vocabulary, an n_targets outside [0, SS_CTC_ALIGN_MAX_LABELS], a Tp outside [1, SS_CTC_ALIGN_MAX_FRAMES], B <= 0,
 * head outside {0, 1}, a missing pointer (d_first / d_last / d_tok_lprob / h_targets may be NULL only when there is no label at all).
 * The per-frame values and the back-pointers are booked on the context's scratch set: sum Tp_b * (n_b + 1) floats and
 * sum Tp_b * ceil((2 n_b + 1) / 4) bytes. */
int ss_batch_ctc_align(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp,
                       const int32_t* h_targets, const int32_t* h_n_targets, ss_ctc_align_result* d_results, int32_t* d_path,
                       int32_t* d_first, int32_t* d_last, float* d_tok_lprob);
/* The plain-C++ twin of the two kernels on host logits [sum T][ld] (V columns read; pad < 0: no pad id): the same transition code,
 * record layout, refusals and edge cases, every pointer a HOST pointer.  h_frame_lprob [sum T] (may be NULL): the per-frame
 * log-probability of the path's state, NaN where there is no path. */
int ss_ctc_align_host(const float* h_logits, int ld, int V, int pad, int B, const int32_t* h_T, const int32_t* h_targets,
                      const int32_t* h_n_targets, ss_ctc_align_result* h_results, int32_t* h_path, int32_t* h_first, int32_t* h_last,
                      float* h_tok_lprob, float* h_frame_lprob);
/* ---- CTC prefix beam search on a text head (csrc/ctc_beam.hip; the search and its order: csrc/ctc_beam.hpp): the most likely TEXT --
 * the labelling whose probability, summed over all its alignments, is highest -- and its runners-up, where ss_batch_ctc_greedy gives
 * the most likely frame path.  Blank = 0; per frame lp = log_softmax(row) with the greedy search's denominator, pad and unk then
 * -inf (agent/ctc_decoder.py:52-60), so a hypothesis never holds blank, pad or unk (it may hold </s>).  Per frame a prefix is
 * extended by the `cand` unmasked non-blank columns with the largest float32 logits (the lower id on a tie; a -inf logit never),
 * and keeps its own last label at that label's true lp.  State: float64 log-probabilities (ending in blank, ending in the last
 * label); a prefix IS its label string, whichever route led to it and whether or not it stayed in the beam in between.  After each
 * frame the `beam` prefixes with the largest total stay (a -inf total never).  Ties: the entries of a frame are ordered by (rank
 * of the source prefix in the entering beam; the prefix itself, then its extensions in candidate order), and the earlier of two
 * equal totals comes first.  score is on the scale of ss_ctc_align_result.score, log p(y | x): exact when nothing was pruned,
 * otherwise a lower bound of the aligner's score for the same labels. ---- */
typedef struct ss_ctc_beam_hyp {
  double score;      /* log of the summed probability of the alignments the search kept for these labels */
  int32_t n_tokens;
  int32_t status;    /* 0 a hypothesis; 1 an empty slot (fewer prefixes alive than nbest, or no labelling has probability > 0);
                      * 2 a NaN in a row of the utterance.  For 1 and 2: n_tokens = 0, score = -inf / NaN */
} ss_ctc_beam_hyp;
#define SS_CTC_BEAM_MAX_BEAM 32
#define SS_CTC_BEAM_MAX_CAND 32
#define SS_CTC_BEAM_MAX_FRAMES 1500     /* T' per utterance, as the aligner */
/* B utterances packed as ss_batch_ctc_greedy_scored takes them (the same head GEMM, pack-invariance setting and workspace), stream-
 * ordered.  Device outputs: d_hyps [B][nbest] best first, d_tokens [B][nbest][out_stride] (entries past n_tokens are left as they
 * were).  An utterance's outputs are the same bits alone and in any pack, in any order.  SS_ERR_ARG, with nothing launched or
 * written: beam outside [1, SS_CTC_BEAM_MAX_BEAM], cand outside [1, SS_CTC_BEAM_MAX_CAND], nbest outside [1, beam], a Tp outside
 * [1, SS_CTC_BEAM_MAX_FRAMES], out_stride < max Tp, B <= 0, head outside {0, 1}, a missing pointer.  Working memory, booked on the
 * context's scratch set (SS_ERR_SCRATCH_CAP past its cap): per utterance 8 (1 + beam Tp) bytes of trie, 12 bytes for each of the
 * child table's slots (the power of two >= 2 beam Tp) and Tp (8 + 4 cand) bytes of per-frame values -- under 56 beam Tp + 136 Tp. */
int ss_batch_ctc_beam(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int beam, int cand,
                      int nbest, ss_ctc_beam_hyp* d_hyps, int32_t* d_tokens, int out_stride);
/* The plain-C++ twin of the two kernels on host logits [sum T][ld] (V columns read; pad / unk < 0: no such id): the same step code,
 * record layout, refusals (and ld < V) and edge cases, every pointer a HOST pointer.  h_den [sum T][2] (the row's max and log-sum;
 * NaN for a row that holds a NaN) and h_cand_id [sum T][cand] (-1 where a row has fewer) may be NULL. */
int ss_ctc_beam_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                     int nbest, ss_ctc_beam_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den, int32_t* h_cand_id);
/* ---- A back-off n-gram language model on the device, and its shallow fusion into the CTC prefix beam search (csrc/ngram_lm.hpp,
 * ngram_lm.hip; the fused search: csrc/ctc_beam.hpp).  The model is a forward trie in one open-addressed table: entry 0 is the root
 * (the empty context), the n-gram (w1 .. wk) is the child (entry of (w1 .. wk-1), wk).  Values are natural logarithms, float32,
 * taken as given.  THE SCORING RULE lp(c | state), in float64: acc = 0; loop { (state, c) is an entry e: return acc + logp[e], the
 * new state is e's longest suffix of at most order - 1 tokens that is an entry; state is the root: leave; else acc +=
 * backoff[state] and state = its longest proper suffix that is an entry }; at the root without a unigram for c: acc + logp[unk]
 * (new state: from the unk unigram) when the model has a unigram for unk, else acc + oov_logp (new state: the root).  This is ARPA
 * back-off: the longest context first, a context's weight only where that context exists.  A sequence starts in the state reached
 * from the root by bos (bos >= 0 and the model has that unigram; else the root); the bos unigram's own value is never scored. ---- */
typedef struct ss_ngram_lm ss_ngram_lm;
#define SS_NGRAM_MAX_ORDER 6
/* Builds the table on the host (checks, trie, suffix links, slot placement); the one upload is made by the first device call that
 * uses the model, so creation needs no device; the table then lives on the device that was current at that call, and the object
 * serves that device.  The n-grams are grouped by order, ascending: order k holds h_counts[k - 1] rows of
 * k ids in h_tokens, and h_logp / h_backoff hold one value per n-gram in that order (backoff 0 where the file gives none).  bos /
 * eos / unk: ids, or -1 for none.  SS_ERR_ARG, with nothing allocated: an order outside [1, SS_NGRAM_MAX_ORDER], V <= 0, an id
 * outside [0, V) (bos / eos / unk outside [-1, V)), a duplicate n-gram, an n-gram whose context (itself minus its last token) is
 * not an entry, a non-finite logp / backoff / oov_logp, more than 2^30 entries, a missing pointer.  A missing SUFFIX is legal.
 * Read-only afterwards: one object serves every context and stream. */
int ss_ngram_lm_create(int order, const int64_t* h_counts, const int32_t* h_tokens, const float* h_logp, const float* h_backoff,
                       int V, int bos, int eos, int unk, float oov_logp, ss_ngram_lm** out);
void ss_ngram_lm_destroy(ss_ngram_lm* lm);
/* order, entries (the root included), slots of the table (the power of two >= 2 entries) and the bytes it takes on the device
 * (12 per slot + 16 per entry); each pointer may be NULL. */
int ss_ngram_lm_info(const ss_ngram_lm* lm, int32_t* order, int64_t* entries, int64_t* slots, int64_t* device_bytes);
/* The scoring rule in plain C++ on B packed sequences (h_n[b] tokens each), every one from the start state: h_lp receives per
 * token its float64 lp and, with with_eos, one more value per sequence, lp(eos | final state) -- h_n[b] + with_eos values per
 * sequence, packed; h_state (may be NULL) the state after each of them.  SS_ERR_ARG: a NULL lm, B <= 0, a negative count,
 * with_eos on a model without eos. */
int ss_ngram_score_host(const ss_ngram_lm* lm, int B, const int32_t* h_tokens, const int32_t* h_n, int with_eos, double* h_lp,
                        int32_t* h_state);
/* The LM form of the search above.  A prefix also carries its LM state, lm_sum (the sum of lp over its tokens) and bonus, fixed
 * when its trie node is made: the child by c with lp = lp(c | state of the parent) has bonus[parent] + ((lm_weight * lp) +
 * word_score), three rounded float64 operations.  A frame's entries are ordered by fused = tot + bonus in place of tot (ties as
 * above); pb / pnb / tot stay pure CTC quantities, an entry is alive when its tot is above -inf, and the candidates are chosen
 * by the acoustic logit alone.  At the end prefix r of the last beam gets fin = fused + lm_weight * lp(eos | its state) with
 * eos_term (fin = fused without; word_score is not applied to eos), and the n-best are the last beam by fin descending, the
 * earlier rank first on a tie. */
typedef struct ss_ctc_lm_opts {
  double lm_weight;
  double word_score;
  int32_t eos_term;    /* non-zero: the eos term (the model needs an eos id) */
} ss_ctc_lm_opts;
typedef struct ss_ctc_beam_lm_hyp {
  double score;        /* fin */
  double ctc_score;    /* tot: ss_ctc_beam_hyp.score, the aligner's scale */
  double lm_score;     /* lm_sum (with eos_term, the eos term included): natural log, unweighted */
  int32_t n_tokens;
  int32_t status;      /* as ss_ctc_beam_hyp; for 1 and 2: n_tokens = 0, score = ctc_score = -inf / NaN, lm_score = 0 */
} ss_ctc_beam_lm_hyp;
/* ss_batch_ctc_beam with a model: its arguments, outputs, refusals and pack invariance, and SS_ERR_ARG, with nothing launched
 * or written, for a NULL lm or opts, a model whose V is not the head's, a non-finite lm_weight / word_score, eos_term on a model
 * without eos.  Working memory: ss_batch_ctc_beam's plus 20 (1 + beam Tp) bytes per utterance -- under 76 beam Tp + 136 Tp. */
int ss_batch_ctc_beam_lm(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int beam, int cand,
                         int nbest, ss_ctc_beam_lm_hyp* d_hyps, int32_t* d_tokens, int out_stride, const ss_ngram_lm* lm,
                         const ss_ctc_lm_opts* opts);
/* The plain-C++ twin, as ss_ctc_beam_host is of the plain search. */
int ss_ctc_beam_lm_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                        int nbest, ss_ctc_beam_lm_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den, int32_t* h_cand_id,
                        const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts);
/* ---- Hotword biasing of the CTC prefix beam search (csrc/ctc_bias.hpp, ctc_bias.hip; the biased search: csrc/ctc_beam.hpp): a set of
 * phrases to prefer -- names, products, terms -- given per deployment, where an n-gram model is built offline from a corpus.  A
 * bias set is P phrases of 1 .. SS_CTC_BIAS_MAX_LEN token ids of the head's vocabulary, each with a boost: finite float32, natural
 * log units, earned per token, negative to discourage.  THE AUTOMATON: node 0 is the root (the empty string), one node per distinct
 * phrase prefix; a node's token boost is the largest boost of the phrases that pass through it; held[n] = held[parent] +
 * (double)boost[n], summed root-down in float64; floor[n] = held of the deepest node on the path root .. n (n included) that ends a
 * phrase, 0 if none.  THE SCORING RULE: the state of a string y is the longest suffix of y that is a node (Aho-Corasick goto with
 * fail links).  On token c state s moves to n and the string earns delta = held[n] - held[s] when n is s extended by c (a direct
 * move), else delta = (held[n] - held[s]) + floor[s]: two separately rounded float64 operations, in that order.  So a partial match
 * that breaks is paid back, what was earned up to the last completed phrase is kept, and the part of the suffix that still matches
 * keeps its credit.  With open(s) = held[s] - floor[s], the bias of a finished string is sum(delta) - open(state): an unfinished
 * phrase earns nothing.  A phrase may be a prefix of another ("new", "new york"); a phrase that occurs inside another at a
 * position other than its start is refused.  With that restriction the finished bias of y equals the sum of held[end(p)] over the
 * occurrences (p, i) of phrases in y that are not a proper prefix of another occurrence starting at the same i. ---- */
typedef struct ss_ctc_bias ss_ctc_bias;
#define SS_CTC_BIAS_MAX_LEN 32
#define SS_CTC_BIAS_MAX_PHRASES 4096
/* Builds the automaton on the host; the one upload is made by the first device call that uses the set, so creation needs no device;
 * the table then lives on the device that was current at that call.  Phrase p is h_tokens[h_off[p] .. h_off[p + 1]) with the per-token
 * boost h_boost[p]; h_off holds n_phrases + 1 ascending offsets from 0.  pad / unk: the head's ids, or -1 for none.  SS_ERR_ARG, with
 * nothing allocated: an empty phrase or one longer than SS_CTC_BIAS_MAX_LEN, an id outside [0, V), blank (0), pad or unk inside a
 * phrase, a duplicate phrase, a non-finite boost, more than SS_CTC_BIAS_MAX_PHRASES phrases (or fewer than 0), a phrase that occurs
 * inside another phrase at a position other than its start, V <= 0, pad / unk outside [-1, V), a missing pointer.  Read-only
 * afterwards: one object serves every context and stream. */
int ss_ctc_bias_create(int n_phrases, const int32_t* h_tokens, const int32_t* h_off, const float* h_boost, int V, int pad, int unk,
                       ss_ctc_bias** out);
void ss_ctc_bias_destroy(ss_ctc_bias* bias);
/* phrases, nodes (the root included), slots of the child table (the power of two >= 2 nodes) and the bytes it takes on the device
 * (12 per slot + 32 per node); each pointer may be NULL. */
int ss_ctc_bias_info(const ss_ctc_bias* bias, int32_t* n_phrases, int64_t* nodes, int64_t* slots, int64_t* device_bytes);
/* The scoring rule in plain C++ on B packed sequences (h_n[b] tokens each), every one from the root: h_delta receives per token its
 * float64 delta, h_state (may be NULL) the state after it, h_sum [B] the sum of a sequence's deltas in order, minus open(final
 * state) with `finish`.  A token no phrase holds leads to the root.  SS_ERR_ARG: a NULL bias, B <= 0, a negative count, a missing
 * pointer. */
int ss_ctc_bias_score_host(const ss_ctc_bias* bias, int B, const int32_t* h_tokens, const int32_t* h_n, int finish, double* h_delta,
                           int32_t* h_state, double* h_sum);
/* The bias form of the search above, with an n-gram model or without.  A prefix also carries b_state, the automaton's state of its
 * string, bias_sum, the unscaled sum of its tokens' deltas, and the LM form's bonus, fixed when its trie node is made: the child by
 * c has bonus = B1 + (scale * delta), the multiply and the add rounded separately, where B1 is the LM form's bonus of the child
 * with a model and bonus[parent] without.  A frame's entries are ordered by fused = tot + bonus; pb / pnb / tot stay pure CTC
 * quantities, the candidates are the `cand` largest acoustic logits, and the order of entries, the tie rule and pack invariance
 * are the plain search's.  At the end fin = fused [+ the eos term] - scale * open(b_state) with `finish`, and the n-best are the
 * last beam by fin descending, the earlier rank first on a tie. */
typedef struct ss_ctc_bias_opts {
  double scale;        /* the weight of the bias in the order (finite; 0: the plain order, or the LM form's) */
  int32_t finish;      /* non-zero: the finish term -- an unfinished phrase earns nothing */
  int32_t reserved;
} ss_ctc_bias_opts;
typedef struct ss_ctc_beam_bias_hyp {
  double score;        /* fin */
  double ctc_score;    /* tot: ss_ctc_beam_hyp.score */
  double lm_score;     /* as ss_ctc_beam_lm_hyp.lm_score; 0 without a model */
  double bias_score;   /* bias_sum, after the finish term: natural log, unscaled */
  int32_t n_tokens;
  int32_t status;      /* as ss_ctc_beam_hyp; for 1 and 2: n_tokens = 0, score = ctc_score = -inf / NaN, lm_score = bias_score = 0 */
} ss_ctc_beam_bias_hyp;
/* ss_batch_ctc_beam_lm with a hotword set: its arguments, outputs, refusals and pack invariance.  lm and opts may both be NULL:
 * bias alone.  SS_ERR_ARG, with nothing launched or written, also for a NULL bias or bias_opts, a set whose V, pad or unk are not
 * the head's, a non-finite scale, lm without opts or opts without lm.  Working memory: ss_batch_ctc_beam's plus 20 (1 + beam Tp)
 * bytes per utterance, 32 (1 + beam Tp) with a model. */
int ss_batch_ctc_beam_bias(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int beam, int cand,
                           int nbest, ss_ctc_beam_bias_hyp* d_hyps, int32_t* d_tokens, int out_stride, const ss_ngram_lm* lm,
                           const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias, const ss_ctc_bias_opts* bias_opts);
/* The plain-C++ twin, as ss_ctc_beam_host is of the plain search. */
int ss_ctc_beam_bias_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                          int nbest, ss_ctc_beam_bias_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den, int32_t* h_cand_id,
                          const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias,
                          const ss_ctc_bias_opts* bias_opts);
/* ---- The same search, resumable (csrc/ctc_stream.hip; the kernel: csrc/ctc_beam.hip): a device object holds, for max_sessions slots
 * of one text head, everything the search needs between launches -- per slot the frames consumed, a sticky "NaN seen" flag, the
 * beam that left the last frame (pb, pnb, tot, node, last, and bonus in the LM form), the trie, its child table and the LM fields
 * of its nodes.  The trie's node ids hold the absolute frame, so a search stopped after frame t and taken up at t + 1 IS the one-shot
 * search: the records of an utterance's last call are ss_batch_ctc_beam's (ss_batch_ctc_beam_lm's) on all its frames, byte for byte,
 * however the frames were split over the calls, and the records of any other call are those of the one-shot search on the frames
 * consumed so far (LM form: without the eos term).  Meant for the rows an incremental encoder reports as final (n_final): a final
 * row's bits never change, and under pack invariance its logits are the same bits whenever they are computed.
 * Fixed at creation: beam, cand, nbest, the model and its options (copied).  Memory, booked on m's scratch set in one piece of exact
 * size (SS_ERR_SCRATCH_CAP leaves the set as it was) and released at destroy, per slot, with nodes = 1 + beam * max_frames and
 * slots = the power of two >= 2 * beam * max_frames: 12 slots + 8 nodes + 40 beam + 8 bytes, and 20 nodes more in the LM form --
 * at beam 8 and max_frames 1500: 489552 bytes, with a model 729572.
 * SS_ERR_ARG at creation: head outside {0, 1}, max_sessions <= 0, max_frames outside [1, SS_CTC_BEAM_MAX_FRAMES], beam / cand / nbest
 * outside ss_batch_ctc_beam's limits, opts without lm or lm without opts, ss_batch_ctc_beam_lm's refusals of a model, a NULL
 * pointer. ---- */
typedef struct ss_ctc_stream ss_ctc_stream;
typedef struct ss_ctc_stream_part {
  int32_t frames;      /* frames the slot's search has consumed, this call included */
  int32_t n_stable;    /* length of the longest common prefix of ALL n_alive strings of the beam (not of the first nbest alone):
                        * every later beam entry is one of them or an extension of one, so these tokens can never change again */
  int32_t n_alive;     /* strings in the beam; 0 with status 2 */
  int32_t status;      /* 0, or 2 once a NaN row was seen (sticky until the slot is reset; the hypothesis records are then the
                        * batch call's NaN records) */
} ss_ctc_stream_part;
int ss_ctc_stream_create(ss_model* m, int head, int max_sessions, int max_frames, int beam, int cand, int nbest, const ss_ngram_lm* lm,
                         const ss_ctc_lm_opts* opts, ss_ctc_stream** out);
/* The same object for the bias form of the search (a hotword set, with a model or with lm and opts both NULL): ss_ctc_stream_advance
 * serves it and writes ss_ctc_beam_bias_hyp records, the finish term of bias_opts (copied) only in an utterance's last call, where
 * the eos term is applied; on any other call score = tot + bonus and bias_score = bias_sum, in beam order.  Per slot 20 bytes
 * per node more than the plain object, 32 with a model.  SS_ERR_ARG also for ss_batch_ctc_beam_bias's refusals of a set. */
int ss_ctc_stream_create_bias(ss_model* m, int head, int max_sessions, int max_frames, int beam, int cand, int nbest,
                              const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias,
                              const ss_ctc_bias_opts* bias_opts, ss_ctc_stream** out);
void ss_ctc_stream_destroy(ss_ctc_stream* cs);
/* A new utterance in `slot`.  Host-only: no stream, nothing launched; the slot's child table is cleared on the stream of its first
 * advance after the reset.  An input shorter than the frames consumed is a new utterance, and so is a change of the encoder's
 * chunk sizes (it restarts its finality): the caller resets first. */
int ss_ctc_stream_reset(ss_ctc_stream* cs, int slot);
/* One step for n sessions, stream-ordered.  Session i owns h_T[i] packed rows of d_enc_packed -- ALL its encoder output so far, as
 * ss_stream_pool_forward / ss_encoder_stream_forward return it -- and the search of slot h_slots[i] moves from the f frames it has
 * consumed to h_upto[i], f <= h_upto[i] <= h_T[i] (equal to f: the state is reported, nothing moves).  Only the rows [f, upto) of
 * each session are stacked and go through the head (ss_batch_ctc_beam's GEMM and pack-invariance setting), the candidate kernel and
 * ONE launch of the resumable search kernel, a workgroup per session.  h_final[i] non-zero: the utterance's last call -- the LM form
 * applies the eos term (with opts->eos_term) and ranks the beam by fin as ss_batch_ctc_beam_lm does, and the slot is reset by the
 * call itself.  Device outputs: d_hyps [n][nbest] (ss_ctc_beam_hyp; an object made with a model: ss_ctc_beam_lm_hyp, on a non-final
 * call score = tot + bonus and lm_score = lm_sum, both without eos, in beam order), d_tokens [n][nbest][out_stride], d_part [n].
 * SS_ERR_ARG, with nothing launched or written and the object as it was: n <= 0, a NULL pointer, m not the object's model, a slot
 * outside the object or twice in the call, h_upto[i] < f, h_upto[i] > h_T[i], h_upto[i] > max_frames, out_stride < max h_upto. */
int ss_ctc_stream_advance(ss_model* m, void* stream, ss_ctc_stream* cs, int n, const int32_t* h_slots, const float* d_enc_packed,
                          const int32_t* h_T, const int32_t* h_upto, const int32_t* h_final, void* d_hyps, int32_t* d_tokens,
                          int out_stride, ss_ctc_stream_part* d_part);
/* The plain-C++ twin on an object of ss_debug_ctc_stream_create(on_device = 0): h_logits [sum (upto - f)][ld] are the STACKED NEW
 * rows alone (session i's behind those of the sessions before it), every pointer a HOST pointer; the same step code, records and
 * refusals (and ld < V; there is no h_T). */
int ss_ctc_stream_advance_host(ss_ctc_stream* cs, int n, const int32_t* h_slots, const float* h_logits, int ld, const int32_t* h_upto,
                               const int32_t* h_final, void* h_hyps, int32_t* h_tokens, int out_stride, ss_ctc_stream_part* h_part);
/* ---- Keyword spotting on a text head (csrc/ctc_spot.hip; the step and the emission rule: csrc/ctc_spot.hpp): did these phrases occur
 * in this audio, and when -- many keywords at once, each with a free start and a free end.  Blank = 0; pad and unk are not masked
 * (as in the aligner).  THE RULE:
 * Per-frame cost.  For a head with V columns c[t][v] = logit[t][v] - max_v logit[t][v], one float32 subtraction, so c <= 0; the
 * sum of c along a path is the path's log-likelihood ratio against the arg-max path over the same frames (no denominator).  A frame
 * whose row holds a NaN, or whose maximum is -inf, makes the utterance's status 2: it reports no hits.
 * States.  A keyword is labels y[0..L), 1 <= L <= SS_CTC_SPOT_MAX_LABELS; its states are [y0, 0, y1, 0, ..., y(L-1)], S = 2L - 1, no
 * leading or trailing blank.
 * Recursion, max-plus, the value float64, a start frame carried with every state; before the first frame every value is -inf.
 * State 0 at frame t takes c[t][y0] plus the better of stay (a[t-1][0], its start) and enter (0.0, start = t); stay wins on equality,
 * which as c <= 0 is only while y0 has been the arg-max since its start.  Any other state takes c[t][label(s)] plus the best of
 * stay (s), advance (s - 1) and skip (s - 2, a label state whose label differs from the label before it); ties: stay beats advance
 * beats skip; the start frame is the chosen predecessor's.  Every sum is value + (double)c, in frame order.
 * Candidates.  e_t = a[t][S-1] with start s_t; frame t is a candidate when e_t >= -(double)tau * L, tau >= 0 the keyword's
 * threshold in natural-log units per label.
 * Hits of one keyword never overlap.  Per keyword a pending candidate P and last_end, the end of its last emitted hit.  A candidate
 * with s_t <= last_end is ignored (P stays as it is).  A candidate with s_t <= P.end replaces P when e_t >= P.score (the later wins
 * a tie, so the span covers the last label's run) and is dropped otherwise.  Any other candidate emits P and becomes P.  A frame
 * that is not a candidate emits P.  The utterance's last frame (a stream: its final call) emits P.
 * Order.  An utterance's hits come back sorted by (end, keyword, start).  The count record carries the TRUE number of hits; when it
 * exceeds max_hits the overflow flag is set and WHICH max_hits of them are written is unspecified (they are still sorted). ---- */
typedef struct ss_ctc_hit {
  int32_t keyword;     /* index into the set */
  int32_t start, end;  /* encoder rows of the utterance, both inclusive */
  int32_t n_labels;    /* L */
  double score;        /* e at `end`: the sum of c over the path, <= 0; score / n_labels is what tau bounds */
} ss_ctc_hit;
typedef struct ss_ctc_spot_count {
  int32_t n_hits;      /* the true number of hits (0 with status 2); min(n_hits, max_hits) records were written */
  int32_t status;      /* 0, or 2: a row with a NaN or without a finite maximum (a stream slot: sticky until the slot is reset) */
  int32_t overflow;    /* n_hits > max_hits */
  int32_t frames;      /* frames consumed, this call included */
} ss_ctc_spot_count;
typedef struct ss_ctc_spot_set ss_ctc_spot_set;
typedef struct ss_ctc_spot_stream ss_ctc_spot_stream;
#define SS_CTC_SPOT_MAX_LABELS 32
#define SS_CTC_SPOT_MAX_KEYWORDS 65536
#define SS_CTC_SPOT_MAX_HITS 16384     /* the sort is a rank sort, one workgroup per utterance: m written records cost m * m / 256
                                        * compares per thread -- nothing at the usual 64 .. 256, about 10^6 at the maximum */
#define SS_CTC_SPOT_MAX_UTTERANCES 65535   /* B of a one-shot call, sessions of a stream object: the DP kernel's grid */
/* Builds the set's table on the host; the one upload is made by the first device call that uses the set, so creation needs no
 * device; the table then lives on the device that was current at that call, the object serves THAT device, and a device call
 * with another device current is refused (SS_ERR_ARG): make one set per device.  Keyword k is h_tokens[h_off[k] .. h_off[k + 1]) with the threshold h_tau[k]; h_off holds n_keywords + 1 ascending offsets
 * from 0.  pad / unk: the head's ids, or -1 for none.  The table holds the set's U distinct labels (the blank first), each
 * keyword's states as indices into them, laid onto the lanes of the DP kernel's workgroups in the given order, and the thresholds.
 * Equal keywords are legal (each reports).  SS_ERR_ARG, with nothing allocated: n_keywords outside [1, SS_CTC_SPOT_MAX_KEYWORDS],
 * an empty keyword or one longer than SS_CTC_SPOT_MAX_LABELS, a label that is blank (0), pad, negative or >= V, a negative or
 * non-finite tau, V <= 0, pad / unk outside [-1, V), a missing pointer.  Read-only afterwards: one object serves every context and
 * stream of its device. */
int ss_ctc_spot_set_create(int n_keywords, const int32_t* h_tokens, const int32_t* h_off, const float* h_tau, int V, int pad, int unk,
                           ss_ctc_spot_set** out);
void ss_ctc_spot_set_destroy(ss_ctc_spot_set* set);
/* keywords, distinct labels U (the blank included), states (the sum of 2L - 1), workgroups of the DP kernel per utterance (256
 * lanes each; a keyword never straddles a 64-lane wave) and the bytes the table takes on the device; each pointer may be NULL. */
int ss_ctc_spot_set_info(const ss_ctc_spot_set* set, int32_t* n_keywords, int32_t* n_labels, int64_t* states, int32_t* workgroups,
                         int64_t* device_bytes);
/* B utterances packed as ss_batch_ctc_align takes them (the same head GEMM, pack-invariance setting and scratch booking), stream-
 * ordered.  Device outputs: d_hits [B][max_hits] (records past min(n_hits, max_hits) are left as they were), d_counts [B].  An
 * utterance's records are the same bytes alone and in any pack, in any order (below max_hits).  SS_ERR_ARG, with nothing launched
 * or written: B outside [1, SS_CTC_SPOT_MAX_UTTERANCES], a Tp outside [1, SS_CTC_ALIGN_MAX_FRAMES], max_hits outside [1, SS_CTC_SPOT_MAX_HITS], a set whose V, pad or
 * unk are not the head's, head outside {0, 1}, a NULL pointer.  Working memory, booked on the context's scratch set: sum Tp * U
 * floats of per-frame costs and B * max_hits records; the recursion's state lives in registers. */
int ss_batch_ctc_spot(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp,
                      const ss_ctc_spot_set* set, int max_hits, ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts);
/* The plain-C++ twin of the kernels on host logits [sum T][ld] (the set's V columns read): the same step code, records and refusals
 * (and ld < V), every pointer a HOST pointer.  On overflow it writes the first max_hits records of the order. */
int ss_ctc_spot_host(const float* h_logits, int ld, int B, const int32_t* h_T, const ss_ctc_spot_set* set, int max_hits,
                     ss_ctc_hit* h_hits, ss_ctc_spot_count* h_counts);
/* The same search, resumable: a device object holds, for max_sessions slots of one text head and one set, per slot the frames
 * consumed, the sticky status, per keyword state its value and start frame, and per keyword P and last_end.  THE CONTRACT: the hits
 * of all calls of an utterance, concatenated and sorted by (end, keyword, start), are byte for byte ss_batch_ctc_spot's on all its
 * frames, however the frames were split over the calls.  Memory, booked on m's scratch set in one piece of exact size
 * (SS_ERR_SCRATCH_CAP leaves the set as it was) and released at destroy: max_sessions * (12 NS + 20 K + 4) bytes, rounded up to 8,
 * with NS the set's states and K its keywords.  SS_ERR_ARG at creation: head outside {0, 1}, max_sessions outside [1, SS_CTC_SPOT_MAX_UTTERANCES], a set
 * whose V, pad or unk are not the head's, a NULL pointer. */
int ss_ctc_spot_stream_create(ss_model* m, int head, int max_sessions, const ss_ctc_spot_set* set, ss_ctc_spot_stream** out);
void ss_ctc_spot_stream_destroy(ss_ctc_spot_stream* ks);
/* A new utterance in `slot` (host-only; the state and the sticky status start over at the slot's next advance). */
int ss_ctc_spot_stream_reset(ss_ctc_spot_stream* ks, int slot);
/* One step for n sessions, stream-ordered: ss_ctc_stream_advance's arguments, slot rules and refusals (h_upto[i] at most
 * SS_CTC_ALIGN_MAX_FRAMES; max_hits as above, per session and call).  Only the rows [f, upto) of each session are stacked and go
 * through the head and the gather kernel.  h_final[i] non-zero: the utterance's last call -- P is emitted and the slot is reset by
 * the call itself.  Device outputs: d_hits [n][max_hits] the hits that were emitted in this call, sorted; d_counts [n]. */
int ss_ctc_spot_stream_advance(ss_model* m, void* stream, ss_ctc_spot_stream* ks, int n, const int32_t* h_slots,
                               const float* d_enc_packed, const int32_t* h_T, const int32_t* h_upto, const int32_t* h_final,
                               int max_hits, ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts);
/* The plain-C++ twin on an object of ss_debug_ctc_spot_stream_create(on_device = 0): h_logits [sum (upto - f)][ld] are the STACKED
 * NEW rows alone, every pointer a HOST pointer; the same step code, records and refusals (and ld < V; there is no h_T). */
int ss_ctc_spot_stream_advance_host(ss_ctc_spot_stream* ks, int n, const int32_t* h_slots, const float* h_logits, int ld,
                                    const int32_t* h_upto, const int32_t* h_final, int max_hits, ss_ctc_hit* h_hits,
                                    ss_ctc_spot_count* h_counts);
/* Lockstep beam-1 search from [</s>] (offline: no prefix).  h_max_len[b] = forced-</s> step of
 * utterance b.  h_out_tokens [B][out_stride] receives the generated tokens (incl. the final </s>),
 * h_n_out[b] their number (= rows of valid decoder states); d_feats is [B][feat_rows][dec_dim].
 * B <= 256.  Synchronises. */
int ss_batch_mt_greedy(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp,
                       const int32_t* h_max_len, int min_len, int32_t* h_out_tokens, int out_stride,
                       int32_t* h_n_out, float* d_feats, int feat_rows);
/* Beam search of the offline first-pass text decoder: the reference's SequenceGenerator.generate_decoder with beam_size_mt = beam
 * (fairseq unity/sequence_generator.py:158-525, BeamSearch, finalize_hypos; len_penalty 1), from [</s>] with no prefix.  B
 * utterances x beam hypothesis rows in lockstep; 1 <= beam <= 32 (else SS_ERR_ARG), B * beam <= 256 (else SS_ERR_CAPACITY), checked
 * before anything is launched.  unk_penalty is subtracted from the <unk> log-probability (--unkpen); normalize != 0 divides a
 * finished hypothesis' score by its length (the reference's default; --unnormalized = 0).  Per utterance b and rank i < beam, in the
 * reference's final order (score descending): h_out_tokens [B][beam][out_stride] the tokens incl. the final </s>, h_n_out [B][beam]
 * their number (0 for a rank with no hypothesis), h_scores [B][beam], h_pos_scores [B][beam][out_stride] (may be NULL) the per-token
 * scores.  d_feats [B][feat_rows][dec_dim] receives the decoder states of each utterance's BEST hypothesis: h_n_out[b][0] valid rows
 * (</s> + its tokens without the final </s>), as ss_batch_mt_greedy; rows past them are left untouched.  Buffers are booked on the
 * handle's scratch set (SS_ERR_SCRATCH_CAP past a cap, the set stays usable).  Synchronises every few steps and at the end. */
int ss_batch_mt_beam(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                     const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                     int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows);
/* Ragged continuation of B independent beam-1 searches: per row b exactly the semantics of ss_mt_greedy -- feed [</s>, prefix_b...]
 * (h_prefix: the B prefixes concatenated, h_n_prefix[b] tokens each), then generate; </s> is banned at positions below min_len and
 * forced at position h_max_len[b].  h_out_tokens [B][out_stride] receives the tokens after the prefix incl. the final </s>, h_n_out[b]
 * their number; d_feats [B][feat_rows][dec_dim] the decoder states of every fed position, h_n_feats[b] (may be NULL) = n_prefix_b +
 * n_out_b of them.  Encoder rows packed as in ss_batch_mt_greedy (the session pool's packed output).  The prefixes run as ONE ragged
 * decoder pass, the generated positions in lock-step; pack-invariant arithmetic: a row's tokens and states do not depend on the rest
 * of the call.  Checked before anything is launched: B outside [1, 256], n_prefix_b > max_len_b, h_Tp[b] <= 0 or a prefix id outside
 * the vocabulary -> SS_ERR_ARG; max_len_b + 1 > feat_rows, max_len_b - n_prefix_b + 1 > out_stride or a position past the decoder's
 * table -> SS_ERR_CAPACITY.  Buffers are booked on the handle's scratch set (SS_ERR_SCRATCH_CAP past a cap, the set stays usable).
 * Synchronises every few steps and at the end. */
int ss_batch_mt_continue(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp, const int32_t* h_prefix,
                         const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len, int32_t* h_out_tokens, int out_stride,
                         int32_t* h_n_out, float* d_feats, int feat_rows, int32_t* h_n_feats);
/* Host only: the layout ss_batch_mt_continue makes of such a call, and its refusals (the same codes, same order), with max_tgt_pos /
 * vocab / eos of the model.  h_dims[4] = {S (longest prefix), Tn (most lock-step steps), Lcap (cache rows per row), Np (prefix-pass
 * rows)}; h_tables (may be NULL; tables_cap ints) = the int tables the call uploads: max_len' [B], min_len' [B], row position offset
 * [B], lock-step cross segments [B][4], prefix self segments [B][4], prefix cross segments [B][4], lock-step self segments
 * [max(Tn,1)][B][4], prefix tokens / positions / cache rows / feature rows [Np] each, last prefix row [B]; *h_n_tables their count. */
int ss_batch_mt_continue_plan(int B, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len,
                              int min_len, int out_stride, int feat_rows, int max_tgt_pos, int vocab, int eos, int32_t* h_dims,
                              int32_t* h_tables, int64_t tables_cap, int64_t* h_n_tables);
/* ss_batch_mt_beam behind a forced prefix per utterance (the streaming write path): fairseq's prefix_tokens of the same generator
 * (_prefix_tokens, fairseq/fairseq/sequence_generator.py:596-623).  Utterance b's first h_n_prefix[b] tokens (h_prefix: the B
 * prefixes concatenated; 0 allowed) are forced: after them exactly one hypothesis is alive, its cumulative score the in-order float32
 * sum of the forced tokens' masked log-probabilities (pad -inf, <unk> minus unk_penalty; min_len is not applied at forced steps), and
 * the search goes on from there as ss_batch_mt_beam does from [</s>]; lengths (max_len, min_len, the normalisation) count the prefix.
 * The forced positions are decoded ONCE per utterance, in one ragged pass (that of ss_batch_mt_continue), and the k hypothesis rows
 * read them through the ancestry table.  Per utterance b and rank i: h_out_tokens [B][beam][out_stride] the tokens AFTER the prefix
 * incl. the final </s>, h_n_out [B][beam] their number; h_scores [B][beam] and h_pos_scores [B][beam][out_stride] (may be NULL;
 * h_n_prefix[b] + h_n_out entries) cover the whole hypothesis, prefix included.  d_feats [B][feat_rows][dec_dim]: the decoder
 * states of hypothesis 0 for its h_n_prefix[b] + h_n_out[b][0] fed positions, laid out as ss_batch_mt_continue's.  With no prefix
 * anywhere and beam > 1 the launches are ss_batch_mt_beam's; at beam 1 tokens and states are ss_batch_mt_continue's bit for bit
 * (there the last forced token is a row of the ragged pass, at beam > 1 it is the first lock-step row of all k slots).  Pack-invariant:
 * an utterance's n-best list does not depend on the rest of the call.  Checked before anything is launched, in this order: B <= 0 or
 * beam outside [1, 32] -> SS_ERR_ARG; B * beam > 256 -> SS_ERR_CAPACITY; h_Tp[b] <= 0, n_prefix_b > max_len_b, min_len > max_len_b, a
 * prefix id outside the vocabulary, or </s> / <pad> inside a prefix -> SS_ERR_ARG; max_len_b + 1 > feat_rows, max_len_b + 1 >
 * out_stride or a position past the decoder's table -> SS_ERR_CAPACITY.  Buffers are booked on the handle's scratch set
 * (SS_ERR_SCRATCH_CAP past a cap, the set stays usable).  Synchronises every few steps and at the end. */
int ss_batch_mt_beam_continue(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                              const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                              float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                              float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows);
/* Host only: the layout ss_batch_mt_beam_continue makes of such a call, and its refusals (the same codes, same order), with
 * max_tgt_pos / vocab / eos / pad of the model.  h_dims[8] = {S (longest prefix), Tn (most lock-step steps after the first), Lc
 * (cache rows per slot = S + Tn + 2), Np (prefix-pass rows), R (= B * beam slots), c0 (cache index every slot writes at lock-step
 * index 0), prefix-pass segments, 1 if the last forced token is a prefix-pass row (beam 1)}; h_tables (may be NULL; tables_cap ints)
 * = the int tables the call uploads: lock-step cross segments [R][4], lock-step self segments [Tn + 1][R][4], row position offset
 * [R], first prefix-pass row [B], prefix self / cross segments [segments][4] each, prefix tokens / positions / cache rows / feature
 * rows / forced tokens [Np] each, last prefix-pass row [B]; *h_n_tables their count. */
int ss_batch_mt_beam_continue_plan(int B, int beam, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix,
                                   const int32_t* h_max_len, int min_len, int out_stride, int feat_rows, int max_tgt_pos, int vocab,
                                   int eos, int pad, int32_t* h_dims, int32_t* h_tables, int64_t tables_cap, int64_t* h_n_tables);
/* The controls of the first-pass text search beyond beam, unk_penalty and normalize: the reference's --no-repeat-ngram-size, --lenpen
 * and --temperature (len_penalty, temperature and no_repeat_ngram_size of its generator; unity/sequence_generator.py and
 * fairseq/fairseq/ngram_repeat_block.py).  size = sizeof(ss_mt_search_opts) of the caller (a smaller one is SS_ERR_ARG; fields a
 * later header adds behind these are read only when size covers them).
 *   no_repeat_ngram n (0 = off, else 2 .. 32): at reference step `step` (the hypothesis holds tokens[0 .. step] = </s>, the forced
 *     prefix, the generated tokens) and step + 2 - n >= 0, every i < step + 2 - n whose window tokens[i .. i + n - 2] equals the last
 *     n - 1 tokens bans tokens[i + n - 1]: its log-probability becomes -inf after the other masks (NaN, pad, unk, max_len, min_len)
 *     and before the cumulative score is added.  </s> stands only at position 0 and banned tokens come from positions >= n - 1 >= 1,
 *     so </s> is never banned and a row at max_len always keeps it.  n = 1 is refused: the reference's Python path bans nothing
 *     there and its compiled extension bans every seen token.
 *   len_penalty p (1 = off; finite): with normalize, a finalised hypothesis' score is cum / (float)pow(step + 1, p); p = 1 is the
 *     plain division by step + 1, bit for bit.  Without normalize nothing is divided.
 *   temperature T (1 = off; finite, > 0): the logits are divided by T (a float32 division) before the log-softmax, at every step and
 *     at the forced-prefix rows.
 * NULL, or {size, 0, 1, 1}, is the call without options: the same launches, the same bits. */
typedef struct ss_mt_search_opts {
  int32_t size;
  int32_t no_repeat_ngram;
  float len_penalty;
  float temperature;
} ss_mt_search_opts;
/* ss_batch_mt_beam with search options.  Before every other check: opts->size < sizeof(ss_mt_search_opts), no_repeat_ngram outside
 * {0, 2 .. 32}, a non-finite len_penalty, a non-finite or non-positive temperature -> SS_ERR_ARG.  Then ss_batch_mt_beam's checks. */
int ss_batch_mt_beam_opts(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                          const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                          int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                          const ss_mt_search_opts* opts);
/* ss_batch_mt_beam_continue with search options.  The option checks of ss_batch_mt_beam_opts come first, then
 * ss_batch_mt_beam_continue's in their order, then, with no_repeat_ngram = n: a prefix whose own tokens (</s> in front) hold the same
 * n-gram twice -> SS_ERR_ARG.  Such a prefix would ban one of its forced tokens, and the reference then scores every hypothesis
 * -inf; refusing it means the prefix pass itself needs no ban.  A prefix each of whose tokens was chosen under the same ban (the
 * agents' and session pools' committed prefixes) never trips this check. */
int ss_batch_mt_beam_continue_opts(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                   const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                   float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                                   float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                                   const ss_mt_search_opts* opts);
/* Host only: ss_batch_mt_beam_continue_plan with the refusals ss_batch_mt_beam_continue_opts adds, same codes, same order. */
int ss_batch_mt_beam_continue_plan_opts(int B, int beam, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix,
                                        const int32_t* h_max_len, int min_len, int out_stride, int feat_rows, int max_tgt_pos,
                                        int vocab, int eos, int pad, int32_t* h_dims, int32_t* h_tables, int64_t tables_cap,
                                        int64_t* h_n_tables, const ss_mt_search_opts* opts);
/* Sampling from the first-pass text decoder: the reference generator's --sampling, --sampling-topk, --sampling-topp and --seed
 * (fairseq/fairseq/search.py::Sampling).  size = sizeof(ss_mt_sample_opts) of the caller, versioned as ss_mt_search_opts is.
 *
 * THE RULE.  A call has B utterances with k chains each (1 <= k <= 32, B * k <= 256), a 64-bit seed, one caller-given 64-bit key[b]
 * per utterance, the masks and options of the beam search, topk (0 = off) or topp (0 = off, else in (0, 1]), and optionally a forced
 * prefix per utterance.  Chain j of utterance b is an independent ancestral sample.  At reference step `step` (the prefix counts,
 * as in the beam search) the row's candidate values v[n] are those of the beam search's top-2k kernel, in this order: the float32
 * division of the logits by the temperature; the log-softmax numerics of the log-softmax kernel; the masks in the reference's
 * order (NaN, pad, unk penalty, max_len, min_len, the no-repeat ban).  The cumulative score is NOT added to v[n].  At the first
 * free step all k chains draw from the row of slot 0 (lprobs[:, ::beam_size] of Sampling.step).
 *   Kept set.  topk = K keeps the K largest v[n], ties to the lower id (exact, no arithmetic).  topp = P follows _sample_topp:
 *     order the tokens by v descending, ties to the lower id; with p[n] = exp(v[n]) a token is kept while the running mass BEFORE it
 *     is < P, so the token that crosses P is included.  With neither, every token with v > -inf is kept.  A -inf token is never
 *     kept; a row at max_len keeps </s> alone.
 *   Draw.  u = (x >> 8) * 2^-24 with x = word 0 of Philox4x32-10 at counter (step, j, key_lo, key_hi) and key (seed_lo, seed_hi)
 *     (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85).  The token is the first kept id, in ascending id
 *     order, whose cumulative kept mass exceeds u * Z, Z the kept mass.  The sums are one fixed-order scan per row: no float
 *     atomics, so two runs and two packs give the same bits.
 *   Scores.  The positional score is v[token], the un-renormalised log-probability (scores_buf of Sampling.step); the cumulative
 *     score is the in-order float32 sum of the positional scores (on top of the prefix' sum).  A chain that draws </s> is finalised
 *     and ignored afterwards (cands_to_ignore); its score is cum / (step + 1) ** len_penalty under normalize, formed as the beam
 *     search forms it.  The utterance is done when all k chains are finalised.  Output entries are ordered by final score
 *     descending, ties by chain index; d_feats receives the states of entry 0.
 * The random stream is this library's own; the kept sets, the scores and the distribution are the reference's. */
typedef struct ss_mt_sample_opts {
  int32_t size;
  int32_t topk;        /* 0 = off, else 1 .. tgt_vocab */
  float topp;          /* 0 = off, else in (0, 1] */
  int32_t reserved;
  uint64_t seed;
} ss_mt_sample_opts;
/* ss_batch_mt_beam_opts' argument list with `beam` read as the number of chains k, plus h_keys [B] and the sampling options; opts
 * (search options) may be NULL.  Refusals, before anything is launched and in this order, all SS_ERR_ARG: sample NULL or
 * sample->size < sizeof(ss_mt_sample_opts); topk < 0; topp not finite or outside {0} u (0, 1]; topk and topp both set (the
 * reference silently prefers top-p); h_keys NULL; m NULL; topk > tgt_vocab.  Then the checks of ss_batch_mt_beam_opts in their
 * order.  Every utterance returns exactly k entries. */
int ss_batch_mt_sample(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                       const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride,
                       int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                       const ss_mt_search_opts* opts, const int64_t* h_keys, const ss_mt_sample_opts* sample);
/* The same behind a forced prefix per utterance: ss_batch_mt_beam_continue_opts' argument list, h_keys and the sampling options.
 * The refusals of ss_batch_mt_sample first, then those of ss_batch_mt_beam_continue_opts in their order. */
int ss_batch_mt_sample_continue(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                                float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows, const ss_mt_search_opts* opts,
                                const int64_t* h_keys, const ss_mt_sample_opts* sample);
/* Lexically constrained beam search of the first-pass text decoder: the reference's --constraints with the `ordered`
 * representation (fairseq/fairseq/search.py::LexicallyConstrainedBeamSearch over token_generation_constraints.py
 * ::OrderedConstraintState; Post & Vilar 2018, Hu et al. 2019).  Phrases that must stand in every returned hypothesis, in the order
 * given, with anything between them.
 *
 * THE RULE.  An utterance has phrases p_1 .. p_n of token ids; seq is their concatenation, C = len(seq) <= SS_MT_CONS_MAX_TOKENS,
 * end[i] is set at the last token of each phrase, and U is the number of DISTINCT ids in seq (the reference's
 * num_constraint_tokens = len(state.tokens), a set: U = C unless an id recurs).  Every hypothesis carries state in -1 .. C - 1:
 * bank = state + 1 tokens of seq are out, finished = (state + 1 == C).  advance(state, tok), first case that holds:
 *   1. finished -> state;  2. seq[state + 1] == tok -> state + 1;  3. state == -1 or end[state] -> state;
 *   4. tok == seq[0] -> 0;  5. -1.
 * Case 3 at state -1 is the reference reading endpoints[-1], which Python takes as the LAST element, always set: a hypothesis at
 * the root stays there (cases 4 and 5 would say the same, case 2 having failed).
 * Per step, for each utterance, in the order of LexicallyConstrainedBeamSearch.step / step_sentence:
 *   1. At step > 0, </s> of a row whose state is not finished is -inf: after every other mask (NaN, pad, unk, max_len, min_len,
 *      the no-repeat ban) and before the cumulative score is added.
 *   2. The candidate list: (a) the global top 2k over beam x vocab, in the plain search's order (score, then flattened index);
 *      (b) at step > 0 the best candidate of each row, rows ascending; (c) for each row ascending (row 0 alone at step 0) its next
 *      tokens with their scores from the row: seq[0] if state > 0, seq[state + 1] if not finished -- ascending id, once if equal
 *      (the reference iterates a Python set of them; the outcome cannot depend on that order, see 4 and 5).
 *   3. new_state = advance(state[beam], tok) and bank = new_state + 1 of every candidate.
 *   4. key = (float)((U - bank) * -100) + score: the integer product converted to float32, then one float32 add.  Sort by key
 *      descending, ties by position in the list of 2.
 *   5. Of candidates with the same (beam, tok) the first in that order stays.
 *   6. Order by (rank within the own bank, then higher bank first): round-robin over the banks, furthest-along first.
 *   7. The first 2k are the step's cand_scores / cand_indices / cand_beams; finalisation, the ignore list, the active hypotheses
 *      and `done` are the plain search's, unchanged.
 *   8. Slot j's next state is the new_state of the candidate it continues.
 * Where the reference leaves the outcome to chance -- its sort is unstable, it removes duplicates only between neighbours, its
 * stripe numbers can collide once bank gaps reach the candidate count -- the tie-break of 4 and the identity rule of 5 decide;
 * whenever the reference's own outcome is determined, this is it.  An utterance with no phrase (C = 0) gets the plain search's bits.
 * Temperature, length penalty and the no-repeat ban compose as in the reference: the ban runs before the step, so a banned
 * constraint token is a -inf candidate. */
#define SS_MT_CONS_MAX_TOKENS 64
/* Ints per utterance of the device table: seq [SS_MT_CONS_MAX_TOKENS] | C | U | end bits 0 .. 31 | end bits 32 .. 63 */
#define SS_MT_CONS_TABLE_LD (SS_MT_CONS_MAX_TOKENS + 4)
/* Host only: check the constraints of B utterances and lay out their table.  Utterance b's tokens are h_cons[h_cons_off[b] ..
 * h_cons_off[b + 1]), phrase after phrase; h_cons_end[i] != 0 marks the last token of a phrase.  Refusals, all SS_ERR_ARG: NULL
 * offsets, or NULL tokens / markers with any token; offsets that decrease; more than SS_MT_CONS_MAX_TOKENS tokens for an
 * utterance; a token outside [0, V); pad or </s> in a phrase; an utterance whose last token ends no phrase (an empty or open
 * phrase); with h_max_len, C > h_max_len[b] (the reference would run into its own `assert step < max_len`).  h_table (may be NULL):
 * [B][SS_MT_CONS_TABLE_LD]. */
int ss_mt_cons_table_host(int B, const int32_t* h_cons, const int32_t* h_cons_off, const int32_t* h_cons_end, int V, int pad,
                          int eos, const int32_t* h_max_len, int32_t* h_table);
/* ss_batch_mt_beam_opts' argument list plus the constraints as ss_mt_cons_table_host takes them; opts may be NULL.  The refusals
 * of ss_batch_mt_beam_opts in their order, then those of ss_mt_cons_table_host; nothing is launched or written after one.  The
 * constrained variants of the top-2k and merge kernels run for every utterance of the call, an utterance without phrases
 * included, and return for it the bits ss_batch_mt_beam_opts returns.  The forced-prefix and sampling entry points take no
 * constraints: a constraint bans </s> until every phrase is out, which is not something to do to a partial source. */
int ss_batch_mt_beam_cons(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                          const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                          int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                          const ss_mt_search_opts* opts, const int32_t* h_cons, const int32_t* h_cons_off,
                          const int32_t* h_cons_end);
/* Host only: steps 1 - 8 of the rule for one utterance and one step, in plain C++.  h_lprobs [k][V] are the rows' masked
 * log-probabilities before step 1 and before the cumulative scores h_cum [k] are added (step > 0: v + cum, one float32 add);
 * h_state [k]; the phrases as above (n_cons tokens).  -> the 2k selected candidates in order: score, token, beam, new state.
 * 1 <= k <= 32, V >= 2k + 1; at step 0 only row 0 is read.  The refusals of ss_mt_cons_table_host, and a state outside
 * -1 .. C - 1. */
int ss_mt_cons_select_host(const float* h_lprobs, const float* h_cum, int k, int V, int step, int eos, const int32_t* h_state,
                           const int32_t* h_cons, int n_cons, const int32_t* h_cons_end, float* out_scores, int32_t* out_tokens,
                           int32_t* out_beams, int32_t* out_states);
/* New fbank rows of B streaming sessions in one launch: session b's frames h_first[b] .. h_first[b] + h_n[b] - 1 of its own 16-kHz
 * sample history h_pcm[b] (device; frame i reads samples 160 i .. 160 i + 399) go to h_feat[b] (device, h_n[b] rows of 80).  The
 * same bits as ss_fbank_cmvn's rows.  h_n[b] = 0 skips a session.  1 <= B <= 65535. */
int ss_batch_fbank_frames(ss_model* m, void* stream, int B, const float* const* h_pcm, const int32_t* h_first, const int32_t* h_n,
                          float pcm_scale, float* const* h_feat);
/* ss_batch_fbank_frames for sessions at ANY source rate, each at its own, in one launch and from the source-rate history directly (no
 * 16-kHz history in between): session b's rows h_first[b] .. h_first[b] + h_n[b] - 1 of the fbank of h_pcm[b][0 .. h_n_in[b]) (device,
 * at the source rate) resampled by h_up[b] / h_down[b] (lowest terms) with the low-pass h_taps[b] (device, [2 * h_half_len[b] + 1], gain
 * up: ss_resample's arguments) go to h_feat[b] (device, h_n[b] rows of 80).  Each 16-kHz sample of a row is formed by ss_resample's own
 * sum (the history zero-padded past h_n_in[b]) and the row by ss_fbank_cmvn's code: the same bits as ss_resample over the h_n_in[b]
 * samples followed by ss_fbank_cmvn.  A session with up == down is already at 16 kHz (its taps may be NULL): its rows are
 * ss_batch_fbank_frames' bits.  h_n[b] = 0 skips a session (nothing else of it is read).  1 <= B <= 65535.  SS_ERR_ARG, decided for the
 * whole call before the launch (no row is written): B outside that range, a negative first or count, a ratio ss_fbank_sr_rows refuses
 * (up or down below 1, a negative half_len or n_in, taps that do not fit the workgroup's LDS), a row at or past the rows h_n_in[b]
 * samples resample to, a NULL history / output / tap table of a session with rows. */
int ss_batch_fbank_frames_sr(ss_model* m, void* stream, int B, const float* const* h_pcm, const int32_t* h_n_in, const int32_t* h_up,
                             const int32_t* h_down, const float* const* h_taps, const int32_t* h_half_len, const int32_t* h_first,
                             const int32_t* h_n, float pcm_scale, float* const* h_feat);
/* Host only: the rows ss_batch_fbank_frames_sr can make of n_in source samples, *h_n_rows = 1 + (n16 - 400) / 160 with n16 =
 * ceil(n_in * up / down) (0 below 400), and how many of them are FINAL, *h_n_final: the largest F with
 * ((160 (F - 1) + 399) * down + half_len) / up <= n_in - 1 (integer division) -- the FIR window of the row's last sample lies inside
 * the history, so no later call with more audio changes the row.  Rows from F on still see the zero padding and are recomputed.
 * Either pointer may be NULL.  SS_ERR_ARG for what the entry point refuses about a ratio, from the same code. */
int ss_fbank_sr_rows(int64_t n_in, int up, int down, int half_len, int32_t* h_n_rows, int32_t* h_n_final);
/* Host only, no GPU needed: the non-zero range of every row of a mel matrix h_melw [rows][cols] -- h_lo_hi[2 r] the first non-zero
 * index of row r, h_lo_hi[2 r + 1] one past the last; an all-zero row gives 0, 0 (an empty range).  What a new model computes once
 * from its fe.melw slot ([80][257]) so that the fbank kernel walks bins [lo, hi) of a mel row only: the bins it leaves out are exact
 * zeros, so the row's sum keeps its bits.  SS_ERR_ARG for a NULL pointer or a negative count. */
int ss_fbank_mel_ranges(const float* h_melw, int rows, int cols, int32_t* h_lo_hi);
int ss_batch_t2u_units(ss_model* m, void* stream, int B, const float* d_feats, int feat_rows,
                       const int32_t* h_n, int t2u_causal, int mask_eos, int32_t* d_raw, int32_t* d_tokens,
                       int32_t* d_counts);
/* d_codes / d_dur / d_forced_dur packed [sum K]; d_wav packed, utterance b at h_wav_start[b] with
 * h_n_samples[b] samples.  Synchronises once. */
int ss_batch_vocoder_forward(ss_vocoder* v, void* stream, int B, const int32_t* d_codes, const int32_t* h_K,
                             int dur_prediction, const int32_t* d_forced_dur, float* d_wav,
                             int64_t wav_capacity, int32_t* d_dur, int64_t* h_wav_start,
                             int64_t* h_n_samples);
/* The same with a voice per utterance: h_spkr [B] (host) -- one pack, any mix of speakers (see ss_vocoder_forward_spkr). */
int ss_batch_vocoder_forward_spkr(ss_vocoder* v, void* stream, int B, const int32_t* d_codes, const int32_t* h_K,
                                  int dur_prediction, const int32_t* d_forced_dur, float* d_wav,
                                  int64_t wav_capacity, int32_t* d_dur, int64_t* h_wav_start,
                                  int64_t* h_n_samples, const int32_t* h_spkr /* [B] */);
/* ss_batch_t2u_units with trailing <pad> states: row b's last h_n_tail_pad[b] (0 <= . < h_n[b]) states are masked as keys as
 * ss_t2u_units(..., n_tail_pad) masks them -- T2U encoder self-attention, unit decoder self-attention (ctc_upsample x pad rows) and
 * cross-attention -- and still decoded.  Rows with 0 are bit-identical to ss_batch_t2u_units; pack-invariant like it. */
int ss_batch_t2u_units_pad(ss_model* m, void* stream, int B, const float* d_feats, int feat_rows, const int32_t* h_n,
                           const int32_t* h_n_tail_pad, int t2u_causal, int mask_eos, int32_t* d_raw, int32_t* d_tokens,
                           int32_t* d_counts);
/* MT decoder states only, B rows in one ragged pass (the prefix pass of ss_batch_mt_continue): row b feeds [</s>, tokens_b
 * (h_n_tokens[b], packed in h_tokens), <pad> x h_n_tail_pad[b]] over its h_Tp[b] packed encoder rows; d_feats [B][feat_rows][D]
 * gets the post-LN state of every fed position -- per row what ss_mt_truncate + ss_mt_append(..., n_tail_pad) give.  No search. */
int ss_batch_mt_features(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp, const int32_t* h_tokens,
                         const int32_t* h_n_tokens, const int32_t* h_n_tail_pad, float* d_feats, int feat_rows);
/* ss_batch_mt_features' pass with n_tail_pad = 0 (row b feeds [</s>, tokens_b...]) plus the head-averaged cross-attention of the
 * LAST decoder layer over the fed positions h_first[b] .. h_n_tokens[b] of every row (h_first NULL: 0 for every row; 0 <= h_first[b] <=
 * h_n_tokens[b]): what fairseq returns as a hypothesis' "attention" (agent/sequence_generator.py:383-392; position p is the decoder
 * input that predicts token p).  Row b answers n_b = h_n_tokens[b] + 1 - h_first[b] positions; R = sum n_b.
 *   d_attn (may be NULL): row b's [n_b][h_Tp[b]] probabilities at float offset h_attn_off[b] (an OUTPUT, host, [B], may be NULL, written only
 *     when d_attn is given and only once no refusal can follow: the blocks are packed in row order); attn_capacity = the floats d_attn holds.
 *   d_peak [R] int32: the arg-max source frame of every answered position (lowest index of a tie); d_stat [R][2] = {its probability,
 *     sum_j j * P[j]}; both packed in row order.
 *   d_feats (may be NULL): [B][feat_rows][D], exactly the bits ss_batch_mt_features writes for the same rows.
 * Checks and error codes of ss_batch_mt_features, SS_ERR_CAPACITY also for attn_capacity; nothing is queued before every check and
 * every buffer is made.  Rewrites the scratch set's MT cross-attention K/V (as ss_batch_mt_features does).  Pack-invariant. */
int ss_batch_mt_attention(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp, const int32_t* h_tokens,
                          const int32_t* h_n_tokens, const int32_t* h_first, float* d_feats, int feat_rows, float* d_attn,
                          int64_t* h_attn_off, int64_t attn_capacity, int32_t* d_peak, float* d_stat);
/* ss_batch_mt_features' pass with n_tail_pad = 0 plus the score of the GIVEN text of every row -- fairseq's SequenceScorer
 * (--score-reference) on the first-pass text decoder.  U utterances (h_Tp [U], d_enc_out their packed encoder rows), B >= U rows:
 * row b is a text for utterance h_src[b] (h_src NULL: B == U, row b -> utterance b); several rows may name one utterance -- the
 * cross-attention K/V is computed once over the U utterances, a candidate text costs no encoder copy.  Row b feeds [</s>, tokens_b...]
 * (h_n_tokens[b] tokens WITHOUT </s>, packed in h_tokens): position p predicts tokens_b[p], the last position predicts </s>
 * (fairseq's prev_output_tokens / target pair).  R = sum (h_n_tokens[b] + 1); per position, packed in row order:
 *   d_stat [R][2] float: the natural-log probability of the predicted token under the plain log_softmax of the output projection
 *     (no pad / unk masking, no unk penalty, no temperature), and the arg-max log-probability;
 *   d_idx [R][2] int32: the arg-max id (lowest index of a tie) and the predicted token's rank (0: the model would have chosen it).
 *   d_feats (may be NULL): [B][feat_rows][D], exactly the bits ss_batch_mt_features(..., n_tail_pad 0) writes for the same rows.
 * The states are projected in chunks of at most 2048 rows into one logits buffer of the workspace; [R][V] never exists.  A row's
 * answers are the same bits alone, in any pack and wherever a chunk boundary falls (pack-invariant contexts, the default).
 * Checks and error codes of ss_batch_mt_features, plus SS_ERR_ARG for h_src[b] outside [0, U), U <= 0, U > B, B > 256, and <pad> as
 * a text token (SequenceScorer strips pad).  Every check runs and every buffer is booked before anything is queued: a refusal
 * leaves every output untouched.  Rewrites the scratch set's MT cross-attention K/V and workspace (as ss_batch_mt_features does). */
int ss_batch_mt_score(ss_model* m, void* stream, int U, const float* d_enc_out, const int32_t* h_Tp, int B, const int32_t* h_src,
                      const int32_t* h_tokens, const int32_t* h_n_tokens, float* d_feats, int feat_rows, float* d_stat,
                      int32_t* d_idx);
/* B rows of the S2ST agent's receptive-field vocoder tail: row b has h_K[b] units (packed in d_codes), the last h_n_new[b] new.  With
 * h_ctx[b] > 0 and h_K[b] > n_new + ctx only the last n_new + ctx units are synthesised, unless the durations of context units
 * [2, ctx) cover fewer than h_rf[b] + 2 frames -- then all units are.  Only the new units' samples are written: d_out[h_out_start[b]
 * ..], h_n_out[b] of them (out_capacity floats in all).  h_win_first[b] = first unit synthesised; h_dur (host, sum h_K ints, row b at
 * the prefix sum of h_K) = the durations of the synthesised units.  Synchronises once. */
int ss_batch_vocoder_tail(ss_vocoder* v, void* stream, int B, const int32_t* d_codes, const int32_t* h_K, const int32_t* h_n_new,
                          const int32_t* h_ctx, const int32_t* h_rf, int dur_prediction, float* d_out, int64_t out_capacity,
                          int32_t* h_win_first, int32_t* h_dur, int64_t* h_out_start, int64_t* h_n_out);
/* The same with a voice per row: h_spkr [B] (host).  A row's window and its all-units fallback are synthesised in the row's voice;
 * rows of different voices share the one predictor pass and the one generator pack. */
int ss_batch_vocoder_tail_spkr(ss_vocoder* v, void* stream, int B, const int32_t* d_codes, const int32_t* h_K, const int32_t* h_n_new,
                               const int32_t* h_ctx, const int32_t* h_rf, int dur_prediction, float* d_out, int64_t out_capacity,
                               int32_t* h_win_first, int32_t* h_dur, int64_t* h_out_start, int64_t* h_n_out,
                               const int32_t* h_spkr /* [B] */);

/* ---- Unit spans (csrc/unit_spans.hip): where each text-decoder state is spoken in the output speech.  The unit decoder upsamples
 * every state into ctc_upsample positions, so each raw unit arg-max belongs to one state, the duration predictor gives every unit a
 * whole number of 20-ms frames and the vocoder writes 320 samples per frame: the mapping is exact integers.  For one row of n states,
 * raw[0 .. up n) its arg-max ids (f counts from the row's start):
 *   unit(f)   raw[f] is none of {blank, pad, bos (0), eos} and f == 0 or raw[f] != raw[f - 1] -- exactly what the CTC collapse of
 *             ss_batch_t2u_units plus the callers' dictionary walk keep; its ordinal = the units before it, K = all of them;
 *   it belongs to state f / up (a run that crosses a state boundary: to the earlier state);
 *   d0 <= u0 <= K: dur[j - d0] = the frames of unit ordinal j >= d0 (d0: the first unit the vocoder call synthesised), u0 = the first
 *             NEW unit (the streaming tail emits the units from K - n_new on; offline d0 = u0 = 0).
 * Per state s, over the new units (ordinal >= u0) only: {first_unit = u0 + the new units of states < s, n_units, start_frame = the sum of
 * dur over the new units of states < s, n_frames = the sum over its own}: four int32.  The spans tile the emitted speech: the last
 * start_frame + n_frames, times 320, is the number of samples the vocoder call returned for the row.
 * ss_batch_unit_spans: B rows; d_raw as ss_batch_t2u_units[_pad] leaves it (row b at ctc_upsample x the prefix sum of h_n); the
 * durations either on the device (d_dur, as ss_vocoder_forward / ss_batch_vocoder_forward leave them: packed [sum h_K], d0 = 0 there) or
 * on the host (h_dur, as ss_batch_vocoder_tail returns them) -- exactly one of the two non-NULL; in both, row b lies at the prefix sum of
 * h_K and holds h_K[b] - h_dur_first[b] values.  up / blank / pad / eos are the model's.  One upload (row table and host durations
 * together), one launch (one workgroup per row, any number of states), one download: h_spans [sum h_n][4], h_K_out [B] = the units the
 * kernel counted in each row.  A row whose h_K_out[b] differs from h_K[b] was given the wrong count: its spans are not to be used (no
 * duration at or past h_K[b] is read); the other rows are unaffected.  Synchronises.  SS_ERR_ARG, decided for the whole call with nothing
 * launched or written: B < 1; a null pointer; both or neither duration pointer; an h_n[b] < 1; a negative h_K / h_dur_first;
 * h_dur_first[b] > h_unit0[b]; h_unit0[b] > h_K[b]; a pack of 2^31 positions or units. */
int ss_batch_unit_spans(ss_model* m, void* stream, int B, const int32_t* d_raw, const int32_t* h_n, const int32_t* h_K,
                        const int32_t* h_dur_first, const int32_t* h_unit0, const int32_t* d_dur, const int32_t* h_dur,
                        int32_t* h_spans, int32_t* h_K_out);
/* The plain-C++ twin of the kernel on host arrays, explicit ids: the same definitions and refusals (also: up < 1), no HIP. */
int ss_unit_spans_host(int B, const int32_t* h_raw, const int32_t* h_n, const int32_t* h_K, const int32_t* h_dur_first,
                       const int32_t* h_unit0, const int32_t* h_dur, int up, int blank, int pad, int bos, int eos, int32_t* h_spans,
                       int32_t* h_K_out);

/* ---- profiling hooks for bench.py's roofline leg: bracket every conv-GEMM launch whose tile
 * configuration is in cls_mask with HIP events recorded on the launch stream.  ss_prof_read
 * synchronises on the recorded events and returns the summed kernel time, the summed algorithmic
 * FLOPs (2*M*N*taps*Cin per launch), the launch count and the summed algorithmic bytes (weights,
 * inputs, outputs, residuals once each) of class `cls`. */
int ss_prof_enable(int cls_mask);
/* The same for classes 32 and up: bit i brackets class 32 + i (ss_prof_enable's mask reaches class 31 only). */
int ss_prof_enable_hi(int cls_mask);
int ss_prof_reset(void);
int ss_prof_read(int cls, double* h_ms_total, double* h_flops_total, int64_t* h_launches,
                 double* h_bytes_total);
/* Always-on census since the library was loaded (no events, no synchronisation): launches and algorithmic FLOPs /
 * bytes of tile class `cls` over the WHOLE process -- the denominator for a rocprofv3 kernel-stats or PMC run of the
 * same process (bench.py prints them as "process_census"). */
int ss_prof_totals(int cls, double* h_flops_total, double* h_bytes_total, int64_t* h_launches);
/* Of the launches ss_prof_read covers: the FLOPs the kernels ISSUE as MFMAs.  Equal to the algorithmic count except for the Winograd
 * F(2,3) classes, which issue 4 ceil(k/3) / (2 k) of it -- lets bench.py report a matrix-core busy fraction next to the algorithmic one. */
int ss_prof_read_issued(int cls, double* h_issued_flops_total);
/* Dispatch table: which kernel class took which conv / linear shape.  ss_prof_shape_log(1) starts a fresh in-process collection,
 * ss_prof_shape_dump writes "class N taps Cin operands launches mean_rows gflop_per_launch mbyte_per_launch" lines (operands bit mask:
 * 1 residual, 2 second residual, 4 twin output, 8 input activation, 16 output activation, 32 GLU, 64 ragged segments) into buf and
 * returns the bytes needed (buf may be NULL).  SS_SHAPE_LOG=<path> writes the same table at process exit. */
int ss_prof_shape_log(int on);
int ss_prof_shape_dump(char* buf, int cap);
int ss_prof_num_classes(void);
const char* ss_prof_class_name(int cls);

/* Pack-invariant arithmetic of the ragged-batch twins (default on; SS_PACK_INVARIANT=0 at context creation or on = 0 here switch it
 * off).  The reference decodes ONE utterance per call (agent/speech_to_speech.streamspeech.agent.py:425-478), so an utterance's ids
 * cannot depend on what else is being decoded.  With on = 1 every stage of ss_batch_encoder_forward / ss_batch_ctc_greedy /
 * ss_batch_mt_greedy / ss_batch_t2u_units computes a packed utterance with a summation order that is a function of that utterance
 * alone: every GEMM is one accumulator chain per output element over ascending k (LDS-tiled kernel without split-K, the row-tile
 * kernel, stream-K cut on whole tiles: the same bits), the fused FFN computes every row tile whole in one workgroup, the LayerNorm
 * form and the attention kernel are fixed per layer, the lock-step MT decode uses one split-K form per layer shape -- so the
 * logits of an utterance are bit-identical alone, in any pack and at any position of a pack (tests/test_margin_gpu.py,
 * tests/test_pack_invariance_gpu.py).  on = 0: the fastest kernel for each launch's row count (stream-K k-splits, split-K tiles). */
int ss_model_set_pack_invariant(ss_model* m, int on);
int ss_model_get_pack_invariant(ss_model* m);
/* Test hook: arithmetic mode of the ss_op_* entry points called from the calling thread -- 0 the fastest kernel per shape, 1 the
 * pack-invariant one-chain form, 2 the fixed small-M form of the lock-step decode rows (the model entry points set their own). */
int ss_debug_canon(int mode);

/* Test hook (tests/test_margin_gpu.py): the dense logits [rows, cols] the LAST ss_batch_ctc_greedy / ss_batch_t2u_units call of
 * this context took its arg-max over (they live in the context's scratch until the next call that reuses it).  d_out == NULL:
 * size query only.  Lets a test measure top-1 / top-2 margins of the packed-batch path against the single-utterance path. */
int ss_debug_last_logits(ss_model* m, void* stream, float* d_out, int64_t cap_floats, int* h_rows, int* h_cols);

/* Unit-test entry of the fused Conformer feed-forward kernel (csrc/ffn.hip; what ss_batch_encoder_forward launches twice per
 * layer on packed batches): dY = dX + alpha * (W2 . SiLU(W1 . LayerNorm(dX; ln_g, ln_b) + b1) + b2), then LayerNorm(ln2_g, ln2_b)
 * over the result rows when ln2_g != NULL -- FeedForwardModule.forward + the 0.5-residual wiring and final_layer_norm of
 * ChunkConformerEncoderLayer.forward (researches/chunk_unity/modules/conformer_layer.py:152-164, 254-312).  D must be 256,
 * F % 64 == 0; W1 [F, D], W2 [D, F] row-major; dY may alias dX. */
int ss_op_ffn_fused(void* stream, const float* dX, int ldx, float* dY, int ldy, const float* ln_g, const float* ln_b,
                    const float* dW1, const float* db1, const float* dW2, const float* db2, float alpha,
                    const float* ln2_g, const float* ln2_b, int M, int D, int F);
/* A/B + test hook of the same kernel: grid > 0 fixes its workgroup count (0: heuristic); row_tiles_per_wave 1..4 forces 16- .. 64-row
 * tiles (0: back to the process default: SS_FFN_WM if set, else 48 rows / the pack-invariant form's own choice; -1: keep); enable 0 / 1 switches its use by ss_batch_encoder_forward off / on (-1: keep). */
int ss_debug_ffn(int grid, int row_tiles_per_wave, int enable);
/* A/B + test hook of the row-tile linear kernel (csrc/rtlin.hip: every K = 256 linear of more than 192 rows that goes through
 * ss_op_conv_gemm / the model entry points): grid > 0 fixes its workgroup count (0: heuristic); enable 0 / 1 routes those linears
 * back to the LDS-tiled kernel / to it (-1: keep). */
int ss_debug_rtlin(int grid, int enable);
/* Test hook of the k-blocked row-tile kernel's forms (rt_linear_kb in csrc/rtlin.hip: K = 512 ... 8192 linears of the pack-invariant
 * mode).  uw: 16-column units per wave, 0 = by the launch's unit count, 1 / 2 / 4 force.  order: -1 keep, 0 every workgroup walks a
 * contiguous range of (row tile, column group) units, 1 the launcher's own choice, 2 the XCD-aware order -- also under a forced grid
 * (ss_debug_rtlin(grid, 1)); a launch whose grid G and column groups per tile NCG do not meet that order's conditions (G % 8 == 0,
 * (G / 8) % NCG == 0) then returns SS_ERR_ARG and launches nothing.  Under order 0 or 2 a forced grid is used as given, not clamped
 * to the unit count: the workgroups past the last unit do nothing.  Every form gives the same bits.  Other values: SS_ERR_ARG. */
int ss_debug_rtlin_kb(int uw, int order);
/* {UW, NCG, G, xmap} of the calling process's last rt_linear_kb launch (xmap: 1 = the XCD-aware order ran); zeros before the first. */
int ss_debug_rtlin_kb_last(int32_t out[4]);
/* A/B + test hook of the unit decoder's first layer in ss_batch_t2u_units / ss_batch_t2u_units_pad: its input is 25 copies of each
 * text-decoder state's row, so under pack-invariant arithmetic the LayerNorm and the QKV linear of that layer run on the distinct rows
 * and one copy kernel writes every result row 25 times (on = 1, the default; SS_UNIT_L0_DISTINCT sets it for the process).  on = 0:
 * both run on all upsampled rows, as a context with pack-invariant arithmetic off always does.  The same bits either way.  -1 puts
 * the process default back; other values: SS_ERR_ARG. */
int ss_debug_unit_l0_distinct(int on);
/* A/B + test hook of the fbank kernels (csrc/fbank.hip): dense = 1 walks all 257 bins of every mel row and computes the FFT twiddles
 * with sincospif in the kernel; dense = 0 (the default; SS_FBANK_DENSE sets it for the process) reads the model's tables -- the
 * non-zero bin range of each mel row (ss_fbank_mel_ranges) and the 256 twiddles, filled once per model by the same sincospif
 * expression.  The same bits either way.  -1 puts the process default back; other values: SS_ERR_ARG. */
int ss_debug_fbank_dense(int dense);
/* A/B hook of the 64-channel vocoder-stage kernel (csrc/conv_c64.hip): 0 routes that stage's convs back to the stream-K kernel
 * with pre-activated twin tensors (round 3), 1 to it, -1 keeps the setting; 4 / 5 switch the Winograd F(2,3) form of those convs
 * (csrc/conv_c64w.hip) off / on without touching the first setting; 6 / 7 route the 128-channel stage's ResBlock convs to conv_sk2<128>
 * with twins / to the same Winograd kernel at 128 channels; 8 / 9 the same for the 256-channel stage (the kernel at CH = 256: two slab
 * phases of 128 input channels, two column halves). */
int ss_debug_conv_c64(int enable);
/* A/B hook of the 256-channel form's block shape: rows = 128 (the default: a workgroup produces all 256 output columns of a block of
 * 128 / 126 / 120 rows) or 256 (two workgroups per block of 256 / 252 / 240 rows, one per column half); 0 puts the default back
 * (SS_CONV_C256_ROWS sets it for the process).  Both give the same bits.  Any other value is SS_ERR_ARG. */
int ss_debug_conv_c256_rows(int rows);
/* The same for the 32-channel stage (csrc/conv_c32.hip): 0 = one fused launch per ResBlock (round 3), 1 = one launch per conv;
 * 4 / 5 = the Winograd form of those per-conv launches (csrc/conv_c64w.hip at 32 channels) off / on. */
int ss_debug_conv_c32(int enable);
int ss_debug_conv_c16(int enable);       /* ... and for the 16-channel stage (csrc/conv_c16.hip) */
/* Persistent layer launches of the incremental streaming encoder (csrc/enc_step.hip: two launches + the attention kernel per layer
 * instead of eleven, on a scratch set whose persistent forms are on -- ss_mt_set_persistent -- and for calls with <= 48 rows to compute;
 * SS_NO_ENC_STEP=1 keeps one launch per op): how many such launches this process has made (tests). */
int64_t ss_debug_enc_step_launches(void);
/* Unit-test entry of the LayerNorm-prologue linears (what ln_linear() in model.hip issues for QKV / pointwise conv 1 / the FFNs
 * of one utterance): dC = epi(LayerNorm(dX; ln_g, ln_b, eps 1e-5) . dW^T + dbias), epi as ss_op_conv_gemm (act, alpha, + dR, glu).
 * Served by the small-M kernel (<= 192 rows) or the row-tile kernel (K = 256, more rows); SS_ERR_ARG otherwise. */
int ss_op_ln_linear(void* stream, const float* dX, int ldx, const float* ln_g, const float* ln_b, const float* dW,
                    const float* dbias, const float* dR, int ldr, float* dC, int ldc, int M, int N, int K, int act, float alpha,
                    int glu);
/* ss_op_ln_linear plus what it cannot say.  ln_out (device, [M][K], may be NULL): the normalised rows as a second output -- only the
 * decode GEMV (M <= 4, K % 256 == 0, K <= 2048) writes them, any other shape with ln_out set is SS_ERR_ARG.  canon: the arithmetic
 * mode of this launch (0: the calling thread's, ss_debug_canon; 1 CANON_SEQ; 2 CANON_SMALLM, the fixed small-M form of the lock-step
 * decode rows, up to 1024 rows).  ln_g / ln_b may both be NULL: a plain linear (ln_out is then SS_ERR_ARG, as is one of the two
 * alone).  Returns what launch_conv_gemm returns.  tests/test_gemm_routes_gpu.py. */
int ss_op_ln_linear_ex(void* stream, const float* dX, int ldx, const float* ln_g, const float* ln_b, float* ln_out, const float* dW,
                       const float* dbias, const float* dR, int ldr, float* dC, int ldc, int M, int N, int K, int act, float alpha,
                       int glu, int canon);

/* Tuning / A-B hook (tools/conv_bench.py, tests): bm = 0 heuristic; 1 route every eligible launch to the first-generation
 * stream-K kernel with a grid of ks workgroups (ks = 0 -> 2 per CU; bn = 8: XCD tile groups); 2 no slab kernel; 3 the
 * narrow-stage resblock pairs of the vocoder as two launches; 4 second-generation stream-K with a grid of ks; 5 its split-bf16
 * form; 6 narrow-stage ResBlocks as separate launches; 32 / 64 / 128 a forced tile of the LDS-tiled kernel (bn, ks = KS*10+PD).
 * Any other bm: SS_ERR_ARG. */
int ss_debug_force_tile(int bm, int bn, int ks);
/* Number of bounded-spin time-outs the stream-K kernel has recorded (any value but 0 is a bug). */
int ss_debug_sk_errors(void);
/* Test hook for the key-split form of the single-utterance rel-pos attention (csrc/attention.hip): -1 never split, 0 the
 * launch heuristic (default), n > 0 force n key tiles (of 64 keys) per split. */
int ss_debug_attention_split(int v);
/* Test hook for the few-queries form of the rel-pos attention (attention_relpos_q16_kernel: <= 48 query rows over all keys, the
 * incremental streaming encoder's calls): 0 = off (the 64-query tile kernel takes those launches), 1 = on (default). */
int ss_debug_attention_q16(int v);
/* Test hook: the next time-out check of this handle's scratch set (ss_encoder_stream_status, or the end of a non-deferred
 * ss_encoder_stream_forward) reports a time-out although none happened -- drives the fall-back and the repeat protocol. */
int ss_debug_enc_step_inject_timeout(ss_model* m);
/* Test hook: the booking contract of a scratch set.  *booked = the bytes the set's account holds (what ss_scratch_bytes reports),
 * *held = the sum of the sizes of all its device buffers; the contract is *booked == *held.  SS_ERR_ARG if any buffer of the set
 * is booked under another account or none (both outputs are written anyway). */
int ss_debug_scratch_audit(ss_scratch* sc, size_t* booked, size_t* held);
/* Test hook: the next launch of the persistent MT decode step behaves as if a bounded wait had timed out (it publishes -1),
 * without touching the counter above.  tests/test_mt_persistent_gpu.py drives the fall-back with it. */
int ss_debug_mt_inject_timeout(ss_model* m);

/* ---- op-level entry points (unit tests of single kernels; same launchers the stages use) ---- */
int ss_op_conv_gemm(void* stream, const float* dA, int lda, const float* dW, const float* dbias,
                    const float* dR, int ldr, const float* dR2, int ldr2, float* dC, int ldc,
                    int M, int N, int Cin, int taps, int dil, int stride, int pad, int in_len,
                    int chunk, int in_act, float in_slope, int act, float alpha, float div, int glu);
/* Every form of the conv launcher (csrc/gemm.hpp): the fields mirror the GemmArgs fields a caller can set, one to one (all pointers
 * DEVICE pointers, NULL where optional); the call fills a GemmArgs and returns what launch_conv_gemm returns.  On top of
 * ss_op_conv_gemm: the ragged pack (segs: nseg x {out_start, out_len, in_start, in_len}, max_seg_out = the longest out_len; M and
 * in_len are then the packed totals), the pre-activated twin dC2 = leaky_relu(dC, c2_slope), the slope of a leaky-ReLU epilogue
 * (act_slope), and same_rows as the caller states it (1: stride 1, output row m reads rows m - pad + j * dil of the same packed
 * buffer, segments contiguous with out_start == in_start -- what the persistent slab kernels require).
 * tests/test_slab_ops_gpu.py runs every slab conv kernel through it against tests/slab_ref.py. */
typedef struct ss_op_conv_args {
  const float* A; const float* W; const float* bias; const float* R; const float* R2; float* C; float* C2;
  int32_t lda, ldc, ldr, ldr2, ldc2;
  int32_t M, N, Cin, taps, dil, stride, pad, in_len, chunk;
  int32_t in_act; float in_slope;
  int32_t act; float act_slope, alpha, div, c2_slope;
  int32_t glu;
  const int32_t* segs; int32_t nseg, max_seg_out;
  int32_t same_rows;
} ss_op_conv_args;
int ss_op_conv_gemm_ex(void* stream, const ss_op_conv_args* a);
/* ss_op_conv_gemm_ex plus the GemmArgs fields only the streaming encoder sets.  m_begin: the launch computes output rows [m_begin, M) of
 * a single utterance, pointers / in_len / chunk rule those of row 0 (ss_encoder_stream_forward; the LDS-tile kernel with N > 32, no
 * segments; cleared by the pack-invariant routes, which write every row).  seg_mb (device, nseg x {first row, chunk}) / seg_A (device,
 * nseg input pointers; in_start is relative to them): the ragged subsampler of the session pool -- segment z writes rows
 * [out_start + seg_mb[2 z], out_start + out_len) and nothing below, max_seg_out = the longest out_len - first row; legal only with
 * canon = 1 (CANON_SEQ) and nseg > 0.  canon: the arithmetic mode of this launch (0: the calling thread's, ss_debug_canon).  Returns
 * what launch_conv_gemm returns, SS_ERR_ARG included.  tests/test_stream_ops_gpu.py. */
int ss_op_conv_gemm_rows(void* stream, const ss_op_conv_args* a, int m_begin, const int32_t* seg_mb, const float* const* seg_A, int canon);
/* The fused ResBlock half of the narrow vocoder stages (csrc/conv_slab.hip, launch_conv_pair with the caller's arguments unchanged):
 * dC = conv2(lrelu(conv1_dil(lrelu(dA)) + db1)) + db2 + dA [+ dR2] [/ div], dC2 = leaky_relu(dC, c2_slope) when set; C = 16 / 32,
 * odd taps, M >= 2048 packed rows; d_segs as above ({start, len, ., .}).  SS_ERR_ARG for what the kernel does not take. */
int ss_op_conv_pair(void* stream, const float* dA, int lda, const float* dW1, const float* db1, const float* dW2, const float* db2,
                    float* dC, int ldc, const float* dR2, int ldr2, float div, float* dC2, int ldc2, float c2_slope, int C, int taps,
                    int dil, int M, int in_len, float slope, const int32_t* d_segs, int nseg);
/* The fused ResBlock of the narrow stages (csrc/resblock.hip, launch_resblock_fused with the caller's arguments unchanged):
 * x = dX; for i in 0..2: x = conv2_i(lrelu(conv1_i,dil[i](lrelu(x)) + B1[i])) + B2[i] + x; dY = [dR2 +] x [/ div].  dW1 / dB1 / dW2 /
 * dB2: HOST arrays of three device pointers ([C][taps * C] tap-major matrices, [C] biases), dil: HOST array of three dilations.
 * C = 16 / 32, taps = 3 / 7 / 11, (taps - 1) / 2 * (dil[0] + dil[1] + dil[2] + 3) <= 64, at most 256 segments; SS_ERR_ARG otherwise. */
int ss_op_resblock_fused(void* stream, const float* dX, int ldx, const float* const* dW1, const float* const* dB1,
                         const float* const* dW2, const float* const* dB2, const int32_t* dil, float* dY, int ldy, const float* dR2,
                         int ldr2, float div, int C, int taps, int M, float slope, const int32_t* d_segs, int nseg);
/* Test hook of the persistent slab kernels (conv_slab / conv_pair / resblock_fused / conv_c16 / c32 / c64 and the Winograd forms):
 * grid > 0 caps their workgroup count (the 256-channel Winograd form in 256-row blocks keeps its minimum of 16), 0 lifts the cap; min_rows >= 0
 * replaces the five row thresholds of the dispatch (conv_c16 / c32 / c64, the 128- and 256-channel Winograd forms), min_rows < 0
 * restores them.  (0, -1) is the default state; a negative grid is SS_ERR_ARG.  Tests restore it in `finally`. */
int ss_debug_slab(int grid, long long min_rows);
/* The FP16 conv of the wide vocoder stages (csrc/conv_f16.hip) on C x C weights dW [C][taps*C] (tap-major; packed to FP16 per
 * call): dC [M][C] = epi(sum act_in(dA) * dW) with "same" padding dil*(taps-1)/2, act_in = in_act (0 / 3 = leaky-ReLU in_slope),
 * epi = + dbias, act (0 / 3 leaky-ReLU 0.1), + dR, + dR2, / div (div > 0), dC2 = leaky_relu(dC, 0.1) when set.  C = 64 / 128 / 256.
 * d_segs (device, nseg x {out_start, out_len, in_start = out_start, in_len = out_len}) makes it a ragged launch over M packed rows. */
int ss_op_conv_f16(void* stream, const float* dA, const float* dW, const float* dbias, const float* dR, const float* dR2,
                   float* dC, float* dC2, int M, int C, int taps, int dil, int in_act, float in_slope, int act, float div,
                   const int32_t* d_segs, int nseg);
int ss_op_layernorm(void* stream, const float* dx, int ldx, float* dy, int ldy, const float* dg,
                    const float* db, int M, int D, float eps);
int ss_op_attention(void* stream, const float* dQ, int ldq, const float* dK, int ldk, const float* dV,
                    int ldv, float* dO, int ldo, int Tq, int Tk, int H, float scale, int causal,
                    int chunk, const float* dP, int ldp, const float* du, const float* dv);
/* Every form of the attention launcher (csrc/attention.hpp): the fields mirror AttnArgs one to one (all pointers DEVICE pointers),
 * the call fills an AttnArgs and returns what launch_attention returns, SS_ERR_ARG included.  use_split != 0 binds the process-wide
 * key-split scratch ss_op_attention binds when dP is set; 0 leaves it unbound (the launcher then never splits keys across
 * workgroups).  tests/test_attention_gpu.py runs every kernel of attention.hip through it. */
typedef struct ss_op_attn_args {
  const float* Q; const float* K; const float* V; float* O;
  int32_t ldq, ldk, ldv, ldo;
  int32_t Tq, Tk, H;
  float scale;
  int32_t causal, chunk, q0, k_mask_tail;
  const float* P; int32_t ldp;
  const float* bias_u; const float* bias_v;
  const int32_t* segs; int32_t nseg, max_q, p_tmax;
  const int32_t* seg_tail;
  int32_t no_decode_kernel;
  const int32_t* anc; int32_t anc_ld, anc_slots;
  int32_t use_split;
} ss_op_attn_args;
int ss_op_attention_ex(void* stream, const ss_op_attn_args* a);
/* The head-averaged attention probabilities kernel (csrc/attn_probs.hpp, AttnProbsArgs field for field; all DEVICE pointers):
 * segs as above, of segment s the query rows q_first[s] .. q_len - 1 are answered; answered row i is output row o = row_off[s] + i -
 * q_first[s]: P[p_off[s] + (i - q_first[s]) * k_len + j] = mean over the H heads of softmax_j(scale * q_i . k_j) (P may be NULL),
 * peak[o] = its arg-max (lowest j of a tie), stat[2 o] = P[i][peak], stat[2 o + 1] = sum_j j * P[i][j].  max_rows = the most answered
 * rows of a segment.  Returns what launch_attention_probs returns.  tests/test_mt_attention_gpu.py against tests/mt_attention_ref.py. */
typedef struct ss_op_attn_probs_args {
  const float* Q; const float* K;
  int32_t ldq, ldk, H;
  float scale;
  const int32_t* segs; int32_t nseg;
  const int32_t* q_first; const int32_t* row_off; const int64_t* p_off;
  float* P; int32_t* peak; float* stat;
  int32_t max_rows;
} ss_op_attn_probs_args;
int ss_op_attention_probs(void* stream, const ss_op_attn_probs_args* a);
/* The tail-query attention of the concurrent streaming step (PoolAttnArgs, csrc/attention.hpp), field for field; returns what
 * launch_attention_pool returns. */
typedef struct ss_op_pool_attn_args {
  const float* Qs; float* cache; float* O;
  int32_t ld, ldo, slot_rows;
  const float* P; int32_t ldp, p_tmax;
  const float* bias_u; const float* bias_v;
  const int32_t* sess; const int32_t* qt_pre;
  int32_t nsess, qtiles, H;
  float scale;
} ss_op_pool_attn_args;
int ss_op_attention_pool(void* stream, const ss_op_pool_attn_args* a);
/* Test hook: 1 routes every attention launch the MFMA kernels would take to the VALU kernel (attention_kernel), 0 = default. */
int ss_debug_attention_no_mfma(int v);
int ss_op_dwconv_bn_silu(void* stream, const float* dx, int ldx, float* dy, int ldy, const float* dwt,
                         int K, const float* mean, const float* var, const float* gamma,
                         const float* beta, float eps, int T, int C, int chunk);
/* ... with the launcher's other forms: the ragged pack (segs: device, nseg x {row_start, len}; T = the longest len, every utterance
 * convolved alone) and a row range (rows [t_begin, T) are written, rows below are read as input only). */
int ss_op_dwconv_bn_silu_ex(void* stream, const float* dx, int ldx, float* dy, int ldy, const float* dwt, int K, const float* mean,
                            const float* var, const float* gamma, const float* beta, float eps, int T, int C, int chunk,
                            const int32_t* segs, int nseg, int t_begin);
/* The session pool's own kernels (csrc/stream_pool.hip), each launcher with the arguments the pool step passes; all DEVICE pointers.
 * pool_dwconv: depthwise conv + BatchNorm + SiLU of the tail rows of nsess sessions, sess = nsess x {q_start, n, r0, T, slot, -, chunk,
 * -}: input row t of a session is row t of its slot (cache + slot * slot_rows * C) below r0, stacked row q_start + t - r0 of gs from r0
 * on; y rows q_start .. q_start + n are written, and stacked rows are copied to slot rows [r0, r0 + n).  max_n = the largest n.
 * K odd, <= 31.
 * pool_gather_rows (W = 256 floats per row) / pool_gather_ids (one int32 per row): tab = nsess x {-, len, k0, nf, slot, s_start}, pre =
 * nsess + 1 ascending row offsets of the packed output; row j of a session comes from its slot's row j below k0 and from stacked row
 * s_start + j - k0 otherwise; rows k0 <= j < nf are also written to the slot.
 * pool_stack_rows: out row r of segment z (rows pre[z] .. pre[z + 1]) = enc row src[z] + r - pre[z]; W % 4 == 0, W <= 1024.
 * SS_ERR_ARG for what a kernel cannot take (nsess <= 0 included). */
int ss_op_pool_dwconv(void* stream, const float* gs, float* cache, int slot_rows, float* y, const float* wt, int K, const float* bn_mean,
                      const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int C, const int32_t* sess,
                      int nsess, int max_n);
int ss_op_pool_gather_rows(void* stream, float* out, const float* stk, float* cache, int slot_rows, int W, const int32_t* tab,
                           const int32_t* pre, int nsess, int total);
int ss_op_pool_gather_ids(void* stream, int32_t* out, const int32_t* stk, int32_t* cache, int slot_rows, const int32_t* tab,
                          const int32_t* pre, int nsess, int total);
int ss_op_pool_stack_rows(void* stream, float* out, const float* enc, int W, const int32_t* src, const int32_t* pre, int nsess,
                          int total);

/* ---- the decode glue kernels (csrc/elementwise.hip), each launcher with the caller's arguments unchanged; every pointer is a DEVICE
 * pointer, NULL where the launcher's argument is optional (segs with nseg = 0: the single-utterance form).  Semantics: the comments
 * of csrc/elementwise.hpp; tests/test_glue_ops_gpu.py runs them against tests/glue_ref.py. ---- */
int ss_op_masked_argmax(void* stream, const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2, int force,
                        int32_t* ids, const int32_t* row_max_len, int step, int force_id, const int32_t* row_min_len, int ban_id);
int ss_op_ctc_collapse(void* stream, const int32_t* raw, int T, int blank, int pad, int32_t* tokens, int32_t* index, int32_t* count,
                       const int32_t* segs, int nseg);                /* segs {start, len}: count[s] */
/* The scored twins of the two above (csrc/ctc_scores.hip; agent/ctc_decoder.py:52-62): ids as ss_op_masked_argmax without force / row
 * lengths, lprob[row] = max over unmasked columns of log_softmax(row); tokens / index / count as ss_op_ctc_collapse, last[j] the last
 * frame of token j's run, tok_lprob[j] the float32 sum of lprob over it.  tests/test_ctc_scores_gpu.py against tests/ctc_ref.py. */
int ss_op_masked_argmax_lprob(void* stream, const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2, int32_t* ids,
                              float* lprob);
int ss_op_ctc_collapse_spans(void* stream, const int32_t* raw, const float* lprob, int T, int blank, int pad, int32_t* tokens,
                             int32_t* index, int32_t* last, float* tok_lprob, int32_t* count, const int32_t* segs, int nseg);
/* The token score kernel of ss_batch_mt_score (csrc/mt_score.hip) on the caller's logits [rows][ld] (device; V columns read): for
 * row r with tk = d_target[r] in [0, V): d_stat[2 r] = log_softmax(row)[tk], d_stat[2 r + 1] = the arg-max log-probability --
 * both the bits ss_log_softmax writes at those columns -- d_idx[2 r] = the arg-max id (lowest index of a tie), d_idx[2 r + 1] =
 * #{n: x[n] > x[tk]} + #{n < tk: x[n] == x[tk]}.  tk outside [0, V): the row writes nothing.  A row with a NaN or +inf column, or
 * all -inf: NaN, NaN, -1, -1.  V <= 8192 is held in registers (one read of the row); wider rows, or every row after
 * ss_debug_mt_score_form(1), take the two-read strided form with the same bits.  SS_ERR_ARG before anything is queued for a null
 * pointer, rows <= 0, V <= 0, ld < V, or rows > 16777215 (rows is the grid's x extent: 256 threads a row must stay below 2^32).
 * tests/test_mt_score_gpu.py against tests/mt_score_ref.py. */
int ss_op_mt_token_scores(void* stream, const float* d_logits, int ld, int rows, int V, const int32_t* d_target, float* d_stat,
                          int32_t* d_idx);
int ss_debug_mt_score_form(int force_strided);
/* The two kernels of ss_batch_ctc_align on the caller's logits [sum T][ld] (device; V columns read), arguments and outputs as
 * ss_ctc_align_host with device output pointers.  tests/test_ctc_align_gpu.py against tests/ctc_align_ref.py. */
int ss_op_ctc_align(void* stream, const float* d_logits, int ld, int V, int pad, int B, const int32_t* h_T, const int32_t* h_targets,
                    const int32_t* h_n_targets, ss_ctc_align_result* d_results, int32_t* d_path, int32_t* d_first, int32_t* d_last,
                    float* d_tok_lprob, float* d_frame_lprob);
/* The kernel of ss_batch_unit_spans on the caller's device arrays with explicit ids: arguments, definitions and refusals as
 * ss_unit_spans_host, d_raw / d_dur / d_spans (16-byte aligned) / d_K_out on the device, the row table uploaded on the stream.
 * Stream-ordered.  tests/test_unit_spans_gpu.py against tests/spans_ref.py. */
int ss_op_unit_spans(void* stream, int B, const int32_t* d_raw, const int32_t* h_n, const int32_t* h_K, const int32_t* h_dur_first,
                     const int32_t* h_unit0, const int32_t* d_dur, int up, int blank, int pad, int bos, int eos, int32_t* d_spans,
                     int32_t* d_K_out);
/* The two kernels of ss_batch_ctc_beam on the caller's logits [sum T][ld] (device; V columns read), arguments and outputs as
 * ss_ctc_beam_host with device output pointers.  tests/test_ctc_beam_gpu.py against tests/ctc_beam_ref.py. */
int ss_op_ctc_beam(void* stream, const float* d_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam,
                   int cand, int nbest, ss_ctc_beam_hyp* d_hyps, int32_t* d_tokens, int out_stride, float* d_den,
                   int32_t* d_cand_id);
/* ss_op_ctc_beam with a model: the kernels of ss_batch_ctc_beam_lm on the caller's logits.  tests/test_ctc_beam_lm_gpu.py. */
int ss_op_ctc_beam_lm(void* stream, const float* d_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam,
                      int cand, int nbest, ss_ctc_beam_lm_hyp* d_hyps, int32_t* d_tokens, int out_stride, float* d_den,
                      int32_t* d_cand_id, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts);
/* An ss_ctc_stream without a model, for V columns with the ids pad / unk (< 0: none): on_device = 0 in host memory, for
 * ss_ctc_stream_advance_host; else in device memory that no scratch set books, for ss_op_ctc_stream_advance.  Refusals as
 * ss_ctc_stream_create (V <= 0 in place of the head).  tests/test_ctc_stream_cpu.py, tests/test_ctc_stream_gpu.py. */
int ss_debug_ctc_stream_create(int V, int pad, int unk, int on_device, int max_sessions, int max_frames, int beam, int cand, int nbest,
                               const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, ss_ctc_stream** out);
/* The kernels of ss_ctc_stream_advance on the caller's device logits: arguments as ss_ctc_stream_advance_host with d_logits and
 * the outputs on the device. */
int ss_op_ctc_stream_advance(void* stream, ss_ctc_stream* cs, int n, const int32_t* h_slots, const float* d_logits, int ld,
                             const int32_t* h_upto, const int32_t* h_final, void* d_hyps, int32_t* d_tokens, int out_stride,
                             ss_ctc_stream_part* d_part);
/* ss_op_ctc_beam_lm with a hotword set (lm and opts may both be NULL): the kernels of ss_batch_ctc_beam_bias on the caller's logits.
 * tests/test_ctc_beam_bias_gpu.py. */
int ss_op_ctc_beam_bias(void* stream, const float* d_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam,
                        int cand, int nbest, ss_ctc_beam_bias_hyp* d_hyps, int32_t* d_tokens, int out_stride, float* d_den,
                        int32_t* d_cand_id, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias,
                        const ss_ctc_bias_opts* bias_opts);
/* ss_debug_ctc_stream_create for the bias form: the object of ss_ctc_stream_create_bias without a model context.
 * tests/test_ctc_stream_bias_cpu.py, tests/test_ctc_stream_bias_gpu.py. */
int ss_debug_ctc_stream_create_bias(int V, int pad, int unk, int on_device, int max_sessions, int max_frames, int beam, int cand,
                                    int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias,
                                    const ss_ctc_bias_opts* bias_opts, ss_ctc_stream** out);
/* ss_ctc_bias_score_host on the device, one wave per sequence: d_tokens packed (device), h_n on the host, d_delta / d_state (may be
 * NULL) / d_sum device arrays of the twin's sizes.  tests/test_ctc_bias_gpu.py. */
int ss_op_ctc_bias_score(void* stream, const ss_ctc_bias* bias, int B, const int32_t* d_tokens, const int32_t* h_n, int finish,
                         double* d_delta, int32_t* d_state, double* d_sum);
/* The three kernels of ss_batch_ctc_spot on the caller's device logits [sum T][ld]: arguments as ss_ctc_spot_host with d_logits and
 * the outputs on the device; scratch made here, a buffer per stream of the calling thread.  tests/test_ctc_spot_gpu.py. */
int ss_op_ctc_spot(void* stream, const float* d_logits, int ld, int B, const int32_t* h_T, const ss_ctc_spot_set* set, int max_hits,
                   ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts);
/* The host twin's recursion laid open on ONE utterance of host logits [T][ld]: h_e / h_start [T][K] receive every keyword's e_t and
 * s_t (the value and start frame of its last state after frame t).  SS_ERR_ARG also for an utterance of status 2.
 * tests/test_ctc_spot_cpu.py. */
int ss_debug_ctc_spot_trace_host(const float* h_logits, int ld, int T, const ss_ctc_spot_set* set, double* h_e, int32_t* h_start);
/* A measuring knob: which of the spotter's three kernels every later call launches (bit 0 the gather, bit 1 the DP, bit 2 the sort;
 * 7, the default, all of them).  ONE word for the whole process, read once per call: with anything else no caller's records
 * are valid, in any context or thread, until it is set back to 7 -- for a measuring process that does nothing else.
 * tools/ctc_spot_bench.py. */
int ss_debug_ctc_spot_phases(int mask);
/* The object of ss_ctc_spot_stream_create without a model context: on_device = 0 for ss_ctc_spot_stream_advance_host (no device is
 * touched), non-zero for ss_op_ctc_spot_stream_advance (the state in a buffer of its own, booked on no set). */
int ss_debug_ctc_spot_stream_create(const ss_ctc_spot_set* set, int on_device, int max_sessions, ss_ctc_spot_stream** out);
/* The kernels of ss_ctc_spot_stream_advance on the caller's device logits: arguments as ss_ctc_spot_stream_advance_host with
 * d_logits and the outputs on the device. */
int ss_op_ctc_spot_stream_advance(void* stream, ss_ctc_spot_stream* ks, int n, const int32_t* h_slots, const float* d_logits, int ld,
                                  const int32_t* h_upto, const int32_t* h_final, int max_hits, ss_ctc_hit* d_hits,
                                  ss_ctc_spot_count* d_counts);
/* ss_ngram_score_host on the device, one wave per sequence: d_tokens packed (device), h_n on the host, d_lp / d_state (may be
 * NULL) device arrays laid out as the host call's.  The op-level handle on the lookup the fused search runs.  Stream-ordered. */
int ss_op_ngram_score(void* stream, const ss_ngram_lm* lm, int B, const int32_t* d_tokens, const int32_t* h_n, int with_eos,
                      double* d_lp, int32_t* d_state);
/* The beam cap of ss_ctc_beam_host alone (the kernels keep SS_CTC_BEAM_MAX_BEAM): tests/test_ctc_beam_cpu.py raises it so that every
 * labelling of a tiny case fits the beam.  -> the cap before the call; max_beam < 1 only reads it. */
int ss_debug_ctc_beam_host_max(int max_beam);
int ss_op_dur_predict(void* stream, const float* logdur, const int32_t* forced, int K, int32_t* dur, int32_t* cum,
                      const int32_t* segs, int nseg);                 /* segs {start, len}: cum of segment s at start + s */
int ss_op_repeat_rows(void* stream, const float* emb, const int32_t* cum, int K, int D, float* out, int F, const int32_t* segs,
                      int nseg);                                      /* segs {unit_start, n_units, frame_start, n_frames}; F = max */
int ss_op_embed_tokens(void* stream, const int32_t* tok, const float* emb, const float* pos_table, float scale, int pos0, float* out,
                       int n, int D, int pos_stride, int pad_id, int vocab);
int ss_op_embed_tokens_rows(void* stream, const int32_t* tok, const float* emb, const float* pos_table, int pos_rows, float scale,
                            int pos0, const int32_t* row_pos, float* out, int n, int D, int pad_id, int vocab);
int ss_op_upsample_add_pos(void* stream, const float* src, int n, int up, const float* pos_row, float pad_value, float* out, int D);
int ss_op_gather_rows(void* stream, const int32_t* idx, const float* table, int D, float* out, int n, int rows);
int ss_op_scatter_rows(void* stream, const int32_t* dst_row, const float* src, int lds, float* dst, int ldd, int D, int n,
                       int dst_rows);
int ss_op_conv_post_tanh(void* stream, const float* x, int T, int C, const float* w, const float* bias, float slope, float* wav,
                         const int32_t* segs, int nseg);              /* segs {sample_start, n_samples}; T = max */
int ss_op_conv_post_tanh_crop(void* stream, const float* x, int C, const float* w, const float* bias, float slope, float* wav,
                              const int32_t* segs, int nseg, int max_keep);   /* segs {sample_start, n_samples, first, out_start} */
/* The speaker add of a multi-speaker conv_pre (see ss_vocoder_forward_spkr): y[row] = act(x[row] + table[speaker][4 lo + hi - 3]) for
 * every row of every segment, segs {start, len, ., .} [nseg] with speakers spkr [nseg] (device) and max_seg_out the longest segment;
 * nseg = 0: one segment of M rows, speaker spkr0.  act != 0: leaky-ReLU(slope).  y may be x; rows outside the segments stay. */
int ss_op_spkr_pre_add(void* stream, const float* x, float* y, int ld, int C0, const float* table, const int32_t* spkr, int spkr0,
                       const int32_t* segs, int nseg, int max_seg_out, int M, int act, float slope);

/* ---- the kernels of the beam search (csrc/beam.hip), one launch each.  R = B * k hypothesis rows; the candidate lists have a row
 * stride of SS_OP_BEAM_CAND entries whatever k is. ---- */
#define SS_OP_BEAM_CAND 64
/* beam_topk_kernel: logits [R][V], cum [R], max_len / npre / done [B] -> the 2k best (score, token) of every taking-part row in
 * cand_s / cand_t [R][SS_OP_BEAM_CAND].  1 <= k <= 32, V >= 2k + 1, V <= 16384 (SS_ERR_ARG otherwise). */
int ss_op_beam_topk(void* stream, const float* logits, int R, int V, int k, int t_step, int min_len, const int32_t* max_len,
                    const int32_t* npre, const int32_t* done, const float* cum, int pad, int unk, int eos, float unk_pen,
                    float* cand_s, int32_t* cand_t);
/* The search state beam_merge_kernel works on (BeamState of csrc/beam.hip field for field; all DEVICE pointers):
 * tok / cum [t_step + 2][R] step-major, anc [2][R][Lc] (anc[t & 1] read at lock-step index t), cand_s / cand_t [R][SS_OP_BEAM_CAND],
 * ignore [R], done / max_len / npre / fin_cnt [B], fin_score / fin_len [B][k], fin_tok / fin_pos / fin_anc [B][k][Lc]. */
typedef struct ss_op_beam_state {
  int32_t* tok; float* cum; int32_t* anc; float* cand_s; int32_t* cand_t; int32_t* ignore; int32_t* done; int32_t* max_len;
  int32_t* npre;
  int32_t* fin_cnt; float* fin_score; int32_t* fin_len; int32_t* fin_tok; float* fin_pos; int32_t* fin_anc;
} ss_op_beam_state;
/* beam_merge_kernel for one step (lock-step index t_step, first free cache index c0; c0 + t_step + 2 <= Lc) */
int ss_op_beam_merge(void* stream, const ss_op_beam_state* st, int B, int k, int Lc, int V, int t_step, int c0, int eos,
                     int normalize);
/* beam_prefix_score_kernel: lp[i] = masked log-softmax of logits row i at ftok[i] (rows with ftok < 0 are left as they are) */
int ss_op_beam_prefix_score(void* stream, const float* logits, int rows, int V, const int32_t* ftok, int pad, int unk, float unk_pen,
                            float* lp);
/* beam_prefix_chain_kernel: per utterance b the float32 chain over lp[row0[b] .. + npre[b]) -> pos (same rows), cum0[b * k] */
int ss_op_beam_prefix_chain(void* stream, const float* lp, const int32_t* row0, const int32_t* npre, int B, int k, float* cum0,
                            float* pos);
/* The option variants of the three kernels above (ss_mt_search_opts), one launch each.
 * beam_topk_kernel<options>: the logits are divided by temperature; with no_repeat_ngram = n >= 2 the row's history is staged in LDS
 * -- tokens[p] = ptok[row0[b] + p] for p < npre[b] (the utterance's prefix-pass tokens, </s> first), tokens[npre[b] + u] =
 * tok[u][anc[r][c0 + u]] for u <= t_step (tok [t_step + 1][R] step-major, anc [R][Lc] the table read at this step) -- and the banned
 * entries are -inf before the top-2k selection.  ptok / row0 may be NULL when every npre is 0; c0 + t_step < Lc.  row_scores (may be
 * NULL): [R][V], every taking-part row's candidate scores as the selection sees them (masks, ban, + cum).  With temperature 1,
 * n = 0 and row_scores NULL this launches the kernel ss_op_beam_topk launches. */
int ss_op_beam_topk_opts(void* stream, const float* logits, int R, int V, int k, int t_step, int min_len, const int32_t* max_len,
                         const int32_t* npre, const int32_t* done, const float* cum, int pad, int unk, int eos, float unk_pen,
                         float* cand_s, int32_t* cand_t, float temperature, int no_repeat_ngram, const int32_t* tok,
                         const int32_t* anc, int Lc, int c0, const int32_t* ptok, const int32_t* row0, float* row_scores);
/* beam_merge_kernel<len_penalty>: a finalised score is cum / (float)pow(step + 1, len_penalty) when normalize; len_penalty 1
 * launches the kernel ss_op_beam_merge launches. */
int ss_op_beam_merge_opts(void* stream, const ss_op_beam_state* st, int B, int k, int Lc, int V, int t_step, int c0, int eos,
                          int normalize, float len_penalty);
/* beam_prefix_score_kernel<temperature>: the logits are divided by temperature; 1 launches the kernel ss_op_beam_prefix_score
 * launches. */
int ss_op_beam_prefix_score_opts(void* stream, const float* logits, int rows, int V, const int32_t* ftok, int pad, int unk,
                                 float unk_pen, float* lp, float temperature);
/* beam_cons_select_kernel: the selection stage of the constrained search (the rule: ss_batch_mt_beam_cons, steps 2 - 8) alone, one
 * workgroup per utterance.  All DEVICE pointers: cand_s / cand_t [R][SS_OP_BEAM_CAND] the rows' sorted 2k lists as the top-2k
 * kernel leaves them (after step 1 and + cum), next_s / next_t [R][2] each row's next tokens (ascending, -1 = none) with their
 * scores from the row, state [R], cons_table [B][SS_MT_CONS_TABLE_LD] (ss_mt_cons_table_host).  -> per utterance the 2k selected
 * candidates in order, row stride SS_OP_BEAM_CAND: score, token, beam, new state.  A state outside -1 .. C - 1 is read as the
 * nearer end. */
int ss_op_beam_cons_select(void* stream, const float* cand_s, const int32_t* cand_t, const float* next_s, const int32_t* next_t,
                           const int32_t* state, const int32_t* cons_table, int B, int k, int t_step, float* out_s, int32_t* out_t,
                           int32_t* out_beam, int32_t* out_state);
/* sample_step_kernel for one step (the rule: ss_mt_sample_opts).  Every row is an utterance of its own with one chain: logits
 * [R][V], max_len / npre [R], the chain index row_j [R] and the key keys [R] of each row (all DEVICE pointers), the mask and ban
 * arguments of ss_op_beam_topk_opts (tok [t_step + 1][R], anc [R][Lc]).  -> per row the drawn token, its positional score v[token],
 * the uniform u and the size of the kept set.  1 <= V <= 16384; the refusals of ss_batch_mt_sample's options, then the
 * temperature's and the ban's as in ss_op_beam_topk_opts. */
int ss_op_sample_step(void* stream, const float* logits, int R, int V, int t_step, int min_len, const int32_t* max_len,
                      const int32_t* npre, int pad, int unk, int eos, float unk_pen, float temperature, int no_repeat_ngram,
                      const int32_t* tok, const int32_t* anc, int Lc, int c0, const int32_t* ptok, const int32_t* row0,
                      const int32_t* row_j, const int64_t* keys, const ss_mt_sample_opts* sample, int32_t* out_tok, float* out_score,
                      float* out_u, int32_t* out_kept);
/* The uniforms of the rule, n at once (all DEVICE pointers): seed / key [n] 64-bit, step / j [n] -> u [n] and the four Philox words
 * [n][4] of counter (step, j, key_lo, key_hi) under key (seed_lo, seed_hi). */
int ss_op_sample_uniform(void* stream, int n, const uint64_t* seed, const int64_t* key, const int32_t* step, const int32_t* j,
                         float* u, uint32_t* words);

#ifdef __cplusplus
}
#endif
#endif /* STREAMSPEECH_HIP_H */
