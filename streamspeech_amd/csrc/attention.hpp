// Multi-head attention kernels (head_dim = 64) for the S2ST path.
//  * rel-pos (Transformer-XL style) chunk-masked self-attention of the Conformer encoder:
//    reference researches/uni_unity/modules/espnet_multihead_attention.py:154-209,
//    score[i,j] = ((q_i+u).k_j + (q_i+v).p[j-i+T-1]) / sqrt(64), key j hidden iff j >= (i/c+1)*c
//    (chunk_unity/models/s2t_conformer.py:195-213).
//  * fairseq MHA (MT decoder, T2U encoder, unit decoder): reference
//    researches/ctc_unity/modules/multihead_attention.py:544-760, q pre-scaled by d_h^-0.5,
//    optional causal triu(-inf, 1) mask, softmax in fp32.
#pragma once
#include "common.hpp"
#include "dispatch.hpp"

namespace ss {

struct AttnArgs {
  const float* Q = nullptr; const float* K = nullptr; const float* V = nullptr; float* O = nullptr;
  int ldq = 0, ldk = 0, ldv = 0, ldo = 0;  // row strides in floats; head h occupies cols [64h, 64h+64)
  int Tq = 0, Tk = 0, H = 0;
  float scale = 1.0f;        // scores *= scale
  int causal = 0;            // key j visible iff j <= i + (Tk - Tq)
  int chunk = 0;             // > 0: key j visible iff j < (i/chunk + 1)*chunk
  int q0 = 0;                // single-utterance rel-pos/chunk form only: query row i is absolute position q0 + i
                             // (keys are 0..Tk-1); used by the incremental streaming encoder (tail queries over all keys)
  int k_mask_tail = 0;       // the last k_mask_tail keys are padding (fairseq key_padding_mask on trailing <pad>)
  // rel-pos extras (null => plain attention); requires q0 + Tq == Tk
  const float* P = nullptr; int ldp = 0;   // projected positional table [2*Tk-1, H*64]
  const float* bias_u = nullptr; const float* bias_v = nullptr;  // [H*64]
  // Ragged batch (nseg > 0): independent utterances packed along the row axis.  segs[4*s] =
  // {q_start, q_len, k_start, k_len}: queries/outputs are rows q_start.. of Q/O, keys rows k_start..
  // of K/V; Tq/Tk above are ignored except max_q (grid sizing).  For the rel-pos form P must point
  // at row 0 of the FULL table (relative offset p_tmax-1) and the kernel slices it per segment.
  const int* segs = nullptr; int nseg = 0; int max_q = 0; int p_tmax = 0;
  // Ragged plain attention only: seg_tail[s] trailing key rows of segment s are padding (k_mask_tail per segment, the same masking
  // semantics; the scalar k_mask_tail is then ignored).  nullptr = the scalar for every segment.  A count of 0 takes exactly the
  // arithmetic of an unmasked segment.
  const int* seg_tail = nullptr;
  // Key-split scratch of the calling context (rel-pos form, single utterance only; nullptr = never split): few query tiles
  // over many keys -- one utterance, or the tail rows of the incremental streaming encoder -- would otherwise run as
  // (query tiles x heads) workgroups that each walk ALL key tiles one after the other.  See attention_relpos_mfma_kernel.
  float* part = nullptr;       // [part_slots][ATTN_PART_FLOATS] parked partial (o, m, l) of a (query tile, head, key split)
  unsigned* cnt = nullptr;     // [cnt_slots] arrivals per (query tile, head); zero between launches
  int part_slots = 0, cnt_slots = 0;
  int ksplit = 0, ktiles_per_split = 0;   // filled in by launch_attention
  // Kernel choice for plain (no rel-pos) attention.  0: by query count (the decode kernel up to 8 queries); 1: always the MFMA tile
  // kernel -- ragged batches whose max_q depends on the pack (T2U encoder rows) must not change kernels with it (pack-invariant bits);
  // the lock-step MT decode (max_q = 1 by construction) keeps 0.
  int no_decode_kernel = 0;
  // Ancestry indirection of the beam search (beam.hip; ragged decode form only, nullptr = plain addressing): key / value j of segment z
  // is row anc[z * anc_ld + k0 + j] * anc_ld + k0 + j of K / V, k0 = the segment's k_start -- slot anc[..] wrote its row of cache
  // index k0 + j there and never overwrites it (k0 > 0: a row whose position 0 is shifted into the cache, beam.hip).  Slot ids are non-negative (beam.hip writes no other); an id of anc_slots or more reads
  // the last slot (an unsigned min, which would send a negative id there as well).  The key-tile and summation order are those of
  // the plain form, so an identity table gives its bits.
  const int* anc = nullptr; int anc_ld = 0; int anc_slots = 0;
};
constexpr int ATTN_PART_FLOATS = 5 * 256 * 4;   // 5 b128 per thread: o[4], {m, l, -, -}
constexpr int ATTN_PART_SLOTS = 512, ATTN_CNT_SLOTS = 512;
inline size_t attention_split_bytes() { return (size_t)ATTN_PART_SLOTS * ATTN_PART_FLOATS * sizeof(float) + ATTN_CNT_SLOTS * sizeof(unsigned); }
// points a.part / a.cnt into a scratch block of attention_split_bytes() bytes whose counter part is zero
inline void attention_bind_split(AttnArgs& a, void* scratch) {
  a.part = static_cast<float*>(scratch);
  a.cnt = reinterpret_cast<unsigned*>(a.part + (size_t)ATTN_PART_SLOTS * ATTN_PART_FLOATS);
  a.part_slots = ATTN_PART_SLOTS; a.cnt_slots = ATTN_CNT_SLOTS;
}
void attention_debug_q16(int v);       // test hook: 0 = never the few-queries rel-pos form (attention_relpos_q16_kernel), 1 = default
void attention_debug_split(int v);     // test hook: -1 never split, 0 heuristic, n > 0 key tiles per split = n

int launch_attention(const AttnArgs& a, hipStream_t stream);

// Ragged tail-query rel-pos attention of the concurrent streaming step (stream_pool.hip): ONE launch covers the tail rows of every
// session of the step.  Session z's record sess[8 z] = {q_start, n, r0, T2, slot, chunk, -, -}: its n query rows are rows q_start ..
// of the stacked q|k|v rows Qs (absolute positions r0 .. T2 - 1), its keys are 0 .. T2 - 1 -- rows below r0 from the slot's cache
// (cache + slot * slot_rows * ld), the others from Qs -- its rel-pos table is P sliced at p_tmax - T2, chunk > 0 masks key j iff
// j >= (i / chunk + 1) * chunk.  qt_pre [nsess + 1]: prefix sums of the sessions' 16-query tiles.  Each workgroup also writes its
// query rows' head slice of q|k|v to the slot cache (rows r0 .. of the slot: nobody in the launch reads them from there).
struct PoolAttnArgs {
  const float* Qs = nullptr; float* cache = nullptr; float* O = nullptr;
  int ld = 0, ldo = 0, slot_rows = 0;      // ld: q|k|v row (3 H 64), shared by Qs and the cache
  const float* P = nullptr; int ldp = 0, p_tmax = 0;
  const float* bias_u = nullptr; const float* bias_v = nullptr;
  const int* sess = nullptr; const int* qt_pre = nullptr;
  int nsess = 0, qtiles = 0, H = 0;
  float scale = 1.f;
};
int launch_attention_pool(const PoolAttnArgs& a, hipStream_t stream);
void attention_debug_no_mfma(int v);   // test hook: 1 routes plain attention to the VALU kernel

}  // namespace ss
