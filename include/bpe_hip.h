/*
 * bpe_hip.h -- C-ABI of libbpe_hip.so, the MI355X (gfx950) BPE train/encode engine.
 *
 * This is the drop-in boundary for minbpe's hot path.  The reference
 * (karpathy/minbpe) has no FFI of its own: its boundary is the Python surface
 * minbpe/__init__.py:1-4.  Each entry point below names the reference code it
 * replaces; minbpe_amd/ (Python, ctypes) mirrors the reference classes on top.
 *
 * Conventions
 *   - every call returns BPE_OK (0) or a negative status; no C++ exception
 *     crosses the ABI; bpe_last_error() gives a human-readable message.
 *   - the caller owns every host buffer for the duration of the call; the
 *     library owns all device memory, tied to the ctx, freed by bpe_destroy.
 *   - a ctx is bound to one GPU and is not thread-safe.  One ctx per GPU.
 *   - token ids are int32 (minbpe: Python ints; new id = 256 + i, basic.py:37).
 *   - chunk_offsets: n_chunks START offsets into the byte/id stream, ascending,
 *     chunk_offsets[0] == 0; NULL (n_chunks ignored) = one chunk.  Pairs never
 *     span chunks (regex.py:44,60).
 */
#ifndef BPE_HIP_H
#define BPE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BPE_OK 0
#define BPE_E_HIP (-1)         /* a HIP runtime call failed (see bpe_last_error) */
#define BPE_E_ARG (-2)         /* bad argument */
#define BPE_E_EMPTY_STATS (-3) /* stats dict empty: minbpe raises ValueError from max() (basic.py:35, regex.py:56) */
#define BPE_E_STATE (-4)       /* call out of order (e.g. train before load) */
#define BPE_E_CAP (-5)         /* caller's output buffer too small */
#define BPE_E_LIMIT (-6)       /* size beyond what this build supports */
#define BPE_E_INTERNAL (-7)    /* device-side consistency check failed */

typedef struct bpe_ctx bpe_ctx;

/* ---- lifetime -------------------------------------------------------------- */
int bpe_create(int device_id, bpe_ctx **out);
void bpe_destroy(bpe_ctx *ctx);
const char *bpe_last_error(bpe_ctx *ctx); /* ctx may be NULL: last create error */
/* Run all subsequent work of this ctx on an existing hipStream_t (e.g. torch's
 * current stream, so collectives issued by the host order with our kernels). */
int bpe_set_stream(bpe_ctx *ctx, void *hip_stream);
/* Knobs: "mode" = 0 recount (get_stats every iteration, the literal reference
 * loop) | 1 delta (pair table kept current by the merge pass).  "profile" =
 * 1 records hipEvents around every hot kernel.  Unknown names -> BPE_E_ARG.
 * Variants of the training loop, all producing identical merges (kept for
 * cross-checks and measurement; the defaults are the fast ones):
 *   "slots"  0 contiguous stream | 1 4096-id slots | 2 one-wave slots, in place (default)
 *   "sparse" 0 every pass visits every slot | 1 auto (default) | 2 always through the index
 *   "lean"   0 every iteration takes the general five-launch path | 1 three-launch lean iterations once a
 *            pair's count is <= "lean_count" (2^20; default) | 2 from the first merge on (tests)
 *   "lean_sum" (1: a lean selection works from the previous table update's per-wave records),
 *   "lean_chain" (1: tied pairs are merged off the list one selection made), "aa_sparse" (1: an a == b
 *   pass visits the slots the index names and keeps the index current), "enc_cache" (1), "enc_chain" (1),
 *   "sparse_ratio" (1), "tie_index" (1), "rep_min" (4), "rep_max" (8: log2 of delta replicas),
 *   "lds_delta" (1), "depth" (8: iterations the host runs ahead), "prof_stride" (64), "merge", "k1",
 *   "chain_kcap" (1..31, default 31: most pairs a sparse chain step merges in one sweep; sharded steps: "dp_kcap",
 *   1..15, default 8), "pool_hint" (0..128, 0 = chain_kcap: the pool is rebuilt when fewer untouched entries are left),
 *   "chain_aa" (1: a sparse chain step on 256-id slots merges a pair with a == b at the head of its order itself, as a
 *   batch of one; 0: it hands that merge back to the general path),
 *   "chain_share_first" (1: the batch of a single-GPU job's three-launch chain step may hold a first token twice --
 *   (a, b1), (a, b2), whose sites never overlap --, its merge pass finds a site by its pair; 0: first tokens stay
 *   distinct, as they always do in sharded steps, one-launch steps and forced replays; the results are the same),
 *   "chain_hash_kmin" (0 = 2: the smallest batch whose merge pass looks a site up in the pair table; 32: never --
 *   every position is compared with every pair, the exact fall-back of a batch without a collision-free multiplier),
 *   "lb_tune", "scan_sup" (1024: the three-pass merge scans the tile summaries of streams of more tiles
 *   than this in three small launches instead of one workgroup);
 *   bpe_decode_batch_resident's copy pass: "dec_copy" (1 staged through an LDS window, 16-byte stores | 0 one token
 *   per lane, byte stores), "dec_window" (8192: bytes of that window), "dec_tile" (1024: tokens per workgroup tile);
 *   bpe_rows_resident's pack kernel: "rows_tile" (4096: output elements per workgroup tile, 64..65536, a multiple of
 *   4), "rows_stage" (1024: document starts a tile stages in LDS, 0..4096; a tile that holds more searches global
 *   memory instead, and 0 makes every tile do so -- the cross-check form);
 *   bpe_token_spans_resident's emit kernel: "spans_stage" (1024, 0..4096: the same for its tiles of 1024 tokens);
 *   bpe_project_resident's placement kernel: "proj_tile" (256: tokens per workgroup tile, 64..16384, a multiple of
 *   64), "proj_window" (2048: ids of its LDS window, 64..8192, a multiple of 4);
 *   bpe_count_resident's counting kernel: "count_lds_bins" (32768: the first bins, counted in a workgroup's LDS,
 *   256..32768, a multiple of 256), "count_flush" (2^31: ids a workgroup counts between flushes of that table,
 *   64..2^31), "count_combine" (0: one add per id | 1 equal ids among the 16 bytes a lane loads are one add; measured
 *   no faster);
 *   bpe_select_docs_resident's placement kernel: "sel_tile" (4096: output elements per workgroup tile, 64..65536, a
 *   multiple of 4), "sel_stage" (1024: output starts a tile stages in LDS, 0..4096; a tile that holds more searches
 *   global memory instead, and 0 makes every tile do so -- the cross-check form);
 *   bpe_dup_docs_resident: "dup_tile" (4096: stream positions per workgroup tile of its hash pass, 64..65536, a multiple
 *   of 4), "dup_wave_len" (64, 4..1024: a key of more ids than this is probed and compared by a whole wave, a shorter
 *   one by its lane), "dup_hash_bits" (64, 0..64: only so many bits of a key's hash choose its first table slot and
 *   spare comparisons; 0 makes every probe a full comparison -- the results are the same at every value);
 *   bpe_minhash_resident's signature pass: "mh_tile" (2048: stream positions per workgroup tile, a power of two from
 *   64 to 65536; a tile goes through LDS 2048 positions at a time, a smaller tile whole -- the results are the same at
 *   every value);
 *   bpe_ngram_index_resident / bpe_ngram_overlap_resident's window pass: "ng_tile" (4096: stream positions per workgroup
 *   tile, a power of two from 64 to 65536; a tile goes through LDS 2048 positions at a time, a smaller tile whole),
 *   "ng_hash_bits" (64, 0..64: only so many bits of a window's hash choose its first table slot and its tag; 0 makes
 *   every window start at slot 0 and every probe a full comparison; an index keeps the value it was built with -- the
 *   results are the same at every value);
 *   bpe_repeat_stats_resident's passes: "rp_tile" (4096: stream positions per workgroup tile, a power of two from 64
 *   to 65536; a tile goes through LDS 2048 positions at a time, a smaller tile whole), "rp_hash_bits" (64, 0..64: only
 *   so many bits of a window's hash choose its first table slot and its tag; 0 puts every window of a document onto one
 *   probe chain and makes every probe a full comparison -- the results are the same at every value);
 *   bpe_dup_spans_resident's passes: "ds_tile" (4096: stream positions per workgroup tile, a power of two from 64 to
 *   65536; a tile goes through LDS 2048 positions at a time, a smaller tile whole), "ds_hash_bits" (64, 0..64: only so
 *   many bits of a window's hash choose its first table slot and its tag; 0 puts every window of the stream onto one
 *   probe chain with tag 0 and makes every probe a full comparison -- the results are the same at every value);
 *   bpe_segment_docs_resident's and bpe_segment_marks_resident's passes: "seg_tile" (4096: positions per workgroup
 *   tile, a multiple of 64 from 64 to 65536), "seg_stage" (1024, 0..4096: ranges a tile of the marks pass stages in LDS;
 *   0 makes every lane search global memory -- the results are the same at every value). */
int bpe_set_option(bpe_ctx *ctx, const char *name, int64_t value);

/* ---- input ----------------------------------------------------------------- */
/* text.encode("utf-8") -> list(bytes)  (basic.py:25-26; per chunk regex.py:44).
 * Uploads the bytes; they stay resident so bpe_train can be re-run. */
int bpe_load_bytes(bpe_ctx *ctx, const uint8_t *bytes, uint64_t n,
                   const uint64_t *chunk_offsets, uint64_t n_chunks);
/* The same with a weight per chunk: every pair inside chunk c counts
 * 2^weight_exp[c] times (weight_exp[c] <= 31).  A chunk that occurs w times in the text
 * (regex.py:41-44 keeps all w copies) can be loaded once per set bit of w -- see
 * bpe_dedup_chunks, which builds exactly that list in first-appearance order, so that
 * counts AND the first-occurrence tie-break are those of the full list.  Stream lengths
 * reported by bpe_train then refer to the de-duplicated stream. */
int bpe_load_bytes_weighted(bpe_ctx *ctx, const uint8_t *bytes, uint64_t n,
                            const uint64_t *chunk_offsets, uint64_t n_chunks,
                            const uint8_t *weight_exp);
/* Arbitrary id lists, for the module-level get_stats()/merge() drop-ins
 * (base.py:13-41 called on user lists). */
int bpe_load_ids(bpe_ctx *ctx, const int32_t *ids, uint64_t n,
                 const uint64_t *chunk_offsets, uint64_t n_chunks);

/* ---- single-step hot functions (parity tests, module-level drop-ins) ------- */
/* get_stats(ids) over all chunks into one table (base.py:13-22, regex.py:51-54).
 * Also records each pair's first position (dict insertion order, F3). */
int bpe_get_stats(bpe_ctx *ctx, uint64_t *n_pairs_out);
/* Read back the table of the last bpe_get_stats, unordered; sort by first_pos
 * to obtain the reference's dict order. */
int bpe_read_stats(bpe_ctx *ctx, int32_t *a, int32_t *b, uint64_t *cnt,
                   uint64_t *first_pos, uint64_t cap, uint64_t *n_out);
/* max(stats, key=stats.get) with first-occurrence tie-break (basic.py:35) on
 * the current ids: returns the pair and its count, BPE_E_EMPTY_STATS if none. */
int bpe_argmax(bpe_ctx *ctx, int32_t *a, int32_t *b, uint64_t *count);
/* merge(ids, pair, idx) on every chunk (base.py:25-41, regex.py:60). */
int bpe_merge(bpe_ctx *ctx, int32_t a, int32_t b, int32_t idx, uint64_t *new_len);
int bpe_len(bpe_ctx *ctx, uint64_t *n);
/* Current ids, start flags stripped. */
int bpe_read_ids(bpe_ctx *ctx, int32_t *out, uint64_t cap);
/* Current chunk start offsets (positions in the current id stream). */
int bpe_read_chunk_starts(bpe_ctx *ctx, uint64_t *out, uint64_t cap, uint64_t *n_out);

/* ---- the training loop ----------------------------------------------------- */
/* BasicTokenizer.train / RegexTokenizer.train loop (basic.py:31-45,
 * regex.py:49-66) on the loaded bytes, entirely on device.
 *   pairs_out[2*i], pairs_out[2*i+1] : pair merged at iteration i (idx 256+i)
 *   counts_out[i]                    : stats[pair] (the verbose print, F10)
 *   len_out[i]                       : total ids after merge i
 *   iter_ms_out                      : optional (NULL ok) per-iteration device ms
 *   n_done                           : merges completed
 * Returns BPE_E_EMPTY_STATS when the pair table empties before num_merges
 * (n_done tells where); the Python layer raises ValueError like the reference. */
int bpe_train(bpe_ctx *ctx, int32_t num_merges, int32_t *pairs_out,
              uint64_t *counts_out, double *iter_ms_out, uint64_t *len_out,
              int32_t *n_done);

/* ---- data-parallel training over sharded chunks ------------------- */
/* One ctx per rank; each rank bpe_load_bytes() its contiguous range of chunks.
 * Every rank keeps a replica of the GLOBAL pair table; per iteration the host
 * all-reduces two tiny device buffers (RCCL through torch.distributed, see
 * minbpe_amd/dist.py) -- ids and the table never move:
 *
 *   bpe_dp_begin(num_merges, rank, nranks)   widen + local byte-pair counts
 *   [all-reduce SUM   table   (int32 x 2 x 65536: every count as two 16-bit limbs, low halves then high halves,
 *                              so that the sum over up to 1024 ranks cannot wrap)]
 *   bpe_dp_table_ready()                     the GLOBAL counts from the summed limbs; BPE_E_LIMIT on EVERY rank if a
 *                                            pair occurs 2^32 times or more in the whole job (counts are 32-bit)
 *   for i in range(num_merges):
 *       bpe_dp_select(i)                     arg-max on the replica; local tie-break candidate
 *       [all-reduce MIN   tiekey  (int64 x 3)]   lowest (rank, position) wins the tie (F3/F5);
 *                                               word 2 = -(device status): any rank's failure stops all
 *                                               (a status raised inside merge i travels with exchange i + 1:
 *                                               the peers stop one merge after the failing rank)
 *       bpe_dp_merge(i)                      merge locally, produce the 4 delta vectors
 *       [all-reduce SUM   delta   (int32 x delta_count)]
 *       bpe_dp_apply(i)                      fold them into the replica
 *   bpe_dp_poll(i, ...) any time after bpe_dp_merge(i): the iteration's record
 *   bpe_dp_end()
 * All calls only enqueue work on the ctx's stream (bpe_set_stream) except
 * bpe_dp_poll, which waits for the device to report iteration i.
 * EVERY rank must issue this same schedule for every i in [0, num_merges), also after one of
 * its own polls reported a failure: the remaining iterations are no-ops on the device, and a
 * rank that stopped issuing collectives would leave its peers blocked in theirs. */
int bpe_dp_begin(bpe_ctx *ctx, int32_t num_merges, int32_t rank, int32_t nranks);
int bpe_dp_buffers(bpe_ctx *ctx, void **table, uint64_t *table_count, void **delta,
                   uint64_t *delta_count, void **tiekey);
int bpe_dp_table_ready(bpe_ctx *ctx);
int bpe_dp_select(bpe_ctx *ctx, int32_t iter);
int bpe_dp_merge(bpe_ctx *ctx, int32_t iter);
int bpe_dp_apply(bpe_ctx *ctx, int32_t iter);
int bpe_dp_poll(bpe_ctx *ctx, int32_t iter, int32_t *a, int32_t *b, uint64_t *count,
                uint64_t *local_len, int32_t *status);
int bpe_dp_end(bpe_ctx *ctx);
/* The same loop driven from inside the library with RCCL called directly (librccl is
 * dlopen'ed): rank 0 makes a 128-byte id (bpe_comm_unique_id), the application
 * broadcasts it by whatever means it has, every rank calls bpe_comm_init, then
 * bpe_dp_train.  Identical results on every rank; len_out holds GLOBAL lengths. */
/* 1 if librccl could be loaded in this process (ranks should agree on this, e.g. with a MIN
 * all-reduce over their bootstrap transport, BEFORE any of them enters bpe_comm_init: a rank
 * without the library would leave the others blocked in ncclCommInitRank). */
int bpe_comm_available(void);
int bpe_comm_unique_id(uint8_t *out128);
int bpe_comm_init(bpe_ctx *ctx, int32_t rank, int32_t nranks, const uint8_t *id128);
int bpe_comm_destroy(bpe_ctx *ctx);
int bpe_dp_train(bpe_ctx *ctx, int32_t num_merges, int32_t *pairs_out, uint64_t *counts_out,
                 uint64_t *len_out, int32_t *n_done);
/* bpe_dp_train runs the single-GPU engine's CHAIN STEPS across the ranks: a step merges the next 1..K pairs
 * the reference would merge (the tied pairs at the maximum in order of first occurrence, as long as they share no
 * token), and costs two all-reduces whatever K is:
 *   MIN  int64 x 98              a tie's first occurrences, rank << 40 | local position per tied pair (word 0 = -status,
 *                                word 1 = -1 from a rank that cannot order its share: the general path decides instead)
 *   SUM  int32 x (2 K_cap S + 64)   the batch's delta vectors (S = ids in use, rounded to 64) + per-pair adj words +
 *                                one status word: a failure inside rank r's merge pass is known to every rank BEFORE
 *                                the table update of that same step -- all ranks stop at the same merge
 * (the merges before the tied regime, and every a == b merge, take the per-merge schedule above).
 * bpe_dp_train_cb is the same loop with the collectives handed to the caller: fn(user, device_buffer, count, dtype,
 * op, hip_stream) must all-reduce `count` elements IN PLACE across the ranks, ordered after the work already enqueued on
 * hip_stream and before whatever is enqueued next (enqueue it on that stream, or synchronise), and return 0 -- how
 * torch.distributed (or a test's host-side reduction) drives the loop without librccl in the library.  Every rank
 * calls fn the same number of times with the same counts, also after a rank-local failure. */
#define BPE_DT_INT32 0
#define BPE_DT_INT64 1
#define BPE_OP_SUM 0
#define BPE_OP_MIN 1
typedef int (*bpe_allreduce_fn)(void *user, void *device_buffer, uint64_t count, int32_t dtype, int32_t op,
                                void *hip_stream);
int bpe_dp_train_cb(bpe_ctx *ctx, int32_t num_merges, int32_t rank, int32_t nranks, bpe_allreduce_fn fn, void *user,
                    int32_t *pairs_out, uint64_t *counts_out, uint64_t *len_out, int32_t *n_done);

/* ---- encode ----------------------------------------------------------------- */
/* _encode_chunk for a batch of chunks (regex.py:92-121; basic.py:57-74 when
 * n_chunks == 1).  merges: 2*M int32, in PRIORITY order (the reference's
 * `min(stats, key=merges.get)` picks the lowest merges[pair] value; pass the
 * pairs sorted by that value); the pair at position r merges to id merge_ids[r]
 * (NULL: 256 + r).  ids_out needs n entries; out_offsets n_chunks+1 entries
 * (token offset of each chunk in ids_out).  Invalidates the ids loaded by
 * bpe_load_bytes/bpe_load_ids (buffers are shared). */
int bpe_encode_batch(bpe_ctx *ctx, const int32_t *merges, const int32_t *merge_ids, int32_t M,
                     const uint8_t *bytes, uint64_t n, const uint64_t *chunk_offsets,
                     uint64_t n_chunks, int32_t *ids_out, uint64_t *out_offsets,
                     uint64_t *n_out);
/* The same with every large buffer already ON THE DEVICE (bytes, chunk_offsets, ids_out with room for n ids, out_offsets
 * with n_chunks + 1 entries are device pointers; merges / merge_ids stay host arrays): the kernels read the caller's
 * offsets and write the caller's outputs in place; only the rank table and a few counters cross PCIe.  For callers
 * that keep their batches in HBM (a data loader on the GPU, torch tensors: tensor.data_ptr()).  Offsets are validated
 * on the device (ascending, <= n).  Synchronises the ctx's stream before returning. */
int bpe_encode_batch_resident(bpe_ctx *ctx, const int32_t *merges, const int32_t *merge_ids, int32_t M,
                              const uint8_t *d_bytes, uint64_t n, const uint64_t *d_chunk_offsets,
                              uint64_t n_chunks, int32_t *d_ids_out, uint64_t *d_out_offsets,
                              uint64_t *n_out);
/* Whether bpe_encode_batch's encoder WITHOUT the chunk cache (option enc_cache = 0) keeps tokens and ranks
 * in 16-bit columns for this merge table (host logic, no GPU): every rank below 65535 and every token id
 * -- merge_ids[r], or 256 + r when merge_ids is NULL -- below 65536.  The default (cached) encoder is
 * 32-bit throughout. */
int bpe_encode_uses_16bit(const int32_t *merge_ids, int32_t M);

/* ---- decode -------------------------------------------------------- */
/* `b"".join(vocab[idx] for idx in ids)` (basic.py:51-55, regex.py:78-90, gpt4.py:87-92)
 * for a batch of token ids.  The vocab is a table resident in HBM: entry i holds the
 * bytes vocab_bytes[vocab_offsets[i] .. vocab_offsets[i+1]), i in [0, V).  Sparse ids
 * (special tokens) are the caller's to map onto table indices.
 *   bpe_decode_set_vocab   upload the table (kept until replaced)
 *   bpe_decode_batch       ids -> bytes, left resident; *n_bytes = their number.  An id
 *                          outside [0, V) fails with BPE_E_ARG and *bad_index = the first
 *                          such position (the reference raises KeyError / ValueError there)
 *   bpe_decode_read        copy the bytes out; with doc_token_offsets (k token positions,
 *                          each <= n) also the byte offset of each of those positions. */
int bpe_decode_set_vocab(bpe_ctx *ctx, const uint8_t *vocab_bytes, const uint64_t *vocab_offsets, int32_t V);
int bpe_decode_batch(bpe_ctx *ctx, const int32_t *ids, uint64_t n, uint64_t *n_bytes, uint64_t *bad_index);
int bpe_decode_read(bpe_ctx *ctx, uint8_t *out, uint64_t cap, const uint64_t *doc_token_offsets,
                    uint64_t k, uint64_t *doc_byte_offsets_out);

/* Ids outside [0, V_dense) that decode nevertheless: sparse_ids[j] (strictly ascending, each < 0 or >= V_dense)
 * is table entry V_dense + j of the vocab given to bpe_decode_set_vocab, whose V must equal V_dense + n_sparse.
 * Used by bpe_decode_batch_resident only; bpe_decode_set_vocab clears it (V_dense = V, no sparse ids). */
int bpe_decode_set_sparse(bpe_ctx *ctx, const int32_t *sparse_ids, int32_t n_sparse, int32_t V_dense);

/* bpe_decode_batch + bpe_decode_read with every large buffer ON THE DEVICE and owned by the caller:
 *   d_ids                 n token ids, id_width = 4 (int32) or 8 (int64) bytes each, read in place, never written
 *   d_doc_token_offsets   k token positions (each <= n; NULL with k = 0), validated on the device
 *   d_out, out_cap        receives the bytes; NULL / 0 = only count
 *   d_doc_byte_offsets    k entries: byte offset of each of those positions
 *   *n_bytes              total bytes of the batch (set whenever the ids are valid, also on BPE_E_CAP)
 *   *bad_index            first position whose id does not decode (~0 if none)
 * An id that is neither in [0, V_dense) nor in the sparse list -- negative ids and 64-bit ids outside the int32
 * range included -- fails with BPE_E_ARG and *bad_index; out_cap < total fails with BPE_E_CAP and writes nothing
 * to d_out; a document position > n fails with BPE_E_ARG.  Never writes d_out[out_cap] or beyond, whatever the
 * alignment of d_out.  Synchronises the ctx's stream before returning; keeps no pointer of the caller's.
 * The ctx's decode scratch is shared with bpe_decode_batch: a result of that call not yet read is dropped. */
int bpe_decode_batch_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                              const uint64_t *d_doc_token_offsets, uint64_t k,
                              uint8_t *d_out, uint64_t out_cap, uint64_t *d_doc_byte_offsets,
                              uint64_t *n_bytes, uint64_t *bad_index);

/* ---- resident training rows ---------------------------------------- */
/* A flat id stream with document offsets -- what bpe_encode_batch_resident leaves in HBM -- to fixed-length rows, every
 * large buffer ON THE DEVICE and owned by the caller:
 *   d_ids            n token ids (int32), read in place, never written
 *   d_doc_offsets    n_docs + 1 token positions (never NULL: one entry when n_docs = 0), validated on the device:
 *                    ascending, none beyond n.  Document d is ids[off[d] : off[d + 1]); ids before off[0] or after
 *                    off[n_docs] belong to no document and are never read into a row
 *   the stream       seq_d = ids of document d, followed by sep_id with BPE_ROWS_HAS_SEP (an empty document is then a
 *                    lone separator); stream = seq_0 | seq_1 | ..., T = its length
 *   BPE_ROWS_PACK    row r, column j = stream[r * stride + j] while that position is < T, else pad_id; 1 <= stride <=
 *                    row_len (stride = row_len: disjoint rows; row_len - 1: input and target overlap by one token).
 *                    R = 0 if T = 0, else 1 + ceil(max(T - row_len, 0) / stride): only the last row can be partial.
 *                    d_doc_index / d_pos (either may be NULL): int32 arrays of the rows' shape -- the document an
 *                    element belongs to (a separator to the document it closes; pad: -1) and its index inside seq_d
 *                    (pad: 0)
 *   BPE_ROWS_PER_DOC R = n_docs; row d = seq_d cut to row_len -- the head, or the tail with BPE_ROWS_TRUNC_LEFT --
 *                    then padded with pad_id on the right, or the left with BPE_ROWS_PAD_LEFT.  d_lengths (may be
 *                    NULL): n_docs int32, min(len(seq_d), row_len).  stride is ignored
 *   d_rows           rows_cap rows of row_len elements of row_width = 4 (int32) or 8 (int64) bytes, sep_id and pad_id
 *                    sign-extended; NULL = only count
 *   *n_rows          R (set whenever the offsets are valid, also on BPE_E_CAP)
 *   *bad_doc         first entry of d_doc_offsets that descends or lies beyond n (~0 if none)
 * BPE_E_ARG before any device work: row_len = 0, stride = 0 or > row_len in pack mode, row_width not 4 or 8, an unknown
 * mode or flag (the per-document flags in pack mode included), d_doc_index / d_pos in per-document mode, d_lengths in
 * pack mode.  BPE_E_LIMIT: n >= 2^32, or d_doc_index / d_pos with n + n_docs >= 2^31.  Bad offsets fail with BPE_E_ARG
 * and *bad_doc; rows_cap < R fails with BPE_E_CAP; both write nothing.  Never writes outside the first R * row_len
 * elements of d_rows (and of the companions), whatever their alignment.  Runs on the ctx's stream and synchronises it
 * before returning; keeps no pointer of the caller's. */
#define BPE_ROWS_PACK 0
#define BPE_ROWS_PER_DOC 1
#define BPE_ROWS_HAS_SEP 1u
#define BPE_ROWS_TRUNC_LEFT 2u
#define BPE_ROWS_PAD_LEFT 4u
int bpe_rows_resident(bpe_ctx *ctx, const int32_t *d_ids, uint64_t n,
                      const uint64_t *d_doc_offsets, uint64_t n_docs,
                      int32_t mode, uint32_t flags, uint64_t row_len, uint64_t stride,
                      int32_t sep_id, int32_t pad_id,
                      void *d_rows, int32_t row_width, uint64_t rows_cap,
                      int32_t *d_doc_index, int32_t *d_pos, int32_t *d_lengths,
                      uint64_t *n_rows, uint64_t *bad_doc);

/* ---- resident token spans ------------------------------------------- */
/* The offset mapping of a batch of token ids that live in HBM: for every token, where it lies in the text its document
 * decodes to, in bytes and in characters.  Every large buffer is ON THE DEVICE and owned by the caller.
 *   e(t)             the bytes of table entry t: the vocab as uploaded (bpe_decode_set_vocab / bpe_decode_set_sparse),
 *                    ids resolved as bpe_decode_batch_resident resolves them
 *   lead             a byte b with (b & 0xC0) != 0x80: ASCII, UTF-8 start bytes and bytes that are no UTF-8 at all;
 *                    only 10xxxxxx is not
 *   len_i, leads_i   len(e(t_i)) and the number of lead bytes in e(t_i), for token i of the batch
 *   cont_i           1 if len_i > 0 and the first byte of e(t_i) is not a lead, else 0
 *   B_i, C_i         the sums of len_j and of leads_j over the tokens j < i of the same document
 *   byte span        (B_i, B_i + len_i)
 *   char span        (max(C_i - cont_i, 0), C_i + leads_i)
 * Documents: d_doc_offsets = NULL (n_docs = 0): the whole batch is one document.  Otherwise n_docs + 1 token positions,
 * validated on the device as in bpe_rows_resident (ascending, none beyond n; empty documents are fine), document d being
 * tokens [off[d], off[d + 1]); a token before off[0] or at or after off[n_docs] belongs to no document, its spans are
 * (-1, -1).
 * If the bytes a document decodes to are valid UTF-8 of a string s, then s.encode()[b0:b1] == e(t_i), and for a
 * non-empty token s[c0:c1] is the shortest run of code points whose encoding covers those bytes (two byte tokens that
 * split one two-byte character both get (k, k + 1)); an empty token gets c0 == c1.  On invalid UTF-8 the numbers are
 * still the ones defined above; the clamp at 0 only matters there.
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_byte_spans, d_char_spans   int64 [n][2] each, 8-byte aligned (16-byte stores are used where the address allows);
 *                    either may be NULL, both NULL = validate and count only.  Nothing outside the first 2 n elements of
 *                    either array is written
 *   *n_bytes, *n_chars   the batch's totals: sum of len_i, sum of leads_i (documents or not)
 *   *bad_index       first position whose id does not decode (~0 if none)
 *   *bad_doc         first entry of d_doc_offsets that descends or lies beyond n (~0 if none)
 * BPE_E_STATE without a vocab table.  BPE_E_ARG: id_width not 4 or 8, d_doc_offsets = NULL with n_docs > 0, a span array
 * that is not 8-byte aligned, an id that does not decode (*bad_index), bad offsets (*bad_doc); on either of the last
 * two nothing is written to the span arrays.  BPE_E_LIMIT: a table entry of 2^31 lead bytes or more, n >= 2^43,
 * n_docs >= 2^32.  n = 0 is BPE_OK with totals 0.  The UTF-8 meta of the table (leads and cont of every entry) is made on
 * the device by the first call after a bpe_decode_set_vocab.  Runs on the ctx's stream and synchronises it before
 * returning; keeps no pointer of the caller's; only counters cross PCIe.  The ctx's decode scratch is shared with
 * bpe_decode_batch: a result of that call not yet read is dropped. */
int bpe_token_spans_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                             const uint64_t *d_doc_offsets, uint64_t n_docs,
                             int64_t *d_byte_spans, int64_t *d_char_spans,
                             uint64_t *n_bytes, uint64_t *n_chars,
                             uint64_t *bad_index, uint64_t *bad_doc);

/* ---- projection onto a smaller vocabulary ---------------------------- */
/* A tokenizer of 256 + M entries contains every smaller one: its first vocab_size - 256 merges are the tokenizer of
 * vocab_size entries, and what that one makes of a text is what this one makes of it with every id >= vocab_size
 * expanded into its two children, recursively (both apply ranks in increasing order).  Ids that live in HBM are
 * projected there; every large buffer is ON THE DEVICE and owned by the caller.
 *   bpe_project_set_merges   the merge list, kept until replaced: merges = a0, b0, a1, b1, ..., merge r makes id 256 + r
 *                    and must have the shape training makes: 0 <= a, b < 256 + r, no pair twice.  pass_ids (special
 *                    tokens): n_pass ids, strictly ascending, each < 0 or >= 256 + M; they are legal in the input and
 *                    pass through unchanged.  BPE_E_ARG for a list of another shape
 *   E(t)             [t] if 0 <= t < vocab_size or t is a pass id; E(a) + E(b) if vocab_size <= t < 256 + M and (a, b)
 *                    is the pair of t
 *   bpe_project_resident     out = E(t_0) + E(t_1) + ... for the n ids of d_ids
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   vocab_size       256 <= vocab_size <= 256 + M, else BPE_E_ARG
 *   d_doc_token_offsets   k token positions (each <= n; NULL with k = 0), validated on the device
 *   d_out, out_cap   receives the ids, of the input's width; NULL / 0 = only count.  Must not overlap d_ids: the
 *                    caller's contract
 *   d_doc_out_offsets     k entries: the output position of each of those positions (position n: the total); written
 *                    by a count-only call too
 *   *n_out           ids of the output (set whenever the ids are valid, also on BPE_E_CAP)
 *   *bad_index       first position whose id does not project (~0 if none)
 * Any id E() does not define -- negative ids and 64-bit ids outside the int32 range included, unless a pass id -- fails
 * with BPE_E_ARG and *bad_index, and nothing is written; out_cap < *n_out fails with BPE_E_CAP and writes nothing to
 * d_out; a document position > n fails with BPE_E_ARG and writes nothing to d_out.  Never writes d_out[out_cap] or
 * beyond, whatever the alignment of d_out (to id_width it must be aligned, as d_ids; 16-byte stores are used where the
 * address allows).  BPE_E_STATE before bpe_project_set_merges.
 * The expansions of one vocab_size -- length and ids of every id in [vocab_size, 256 + M) -- are a table made on the
 * host from the merge list and uploaded by the first call at that size; the next calls at the same size build and
 * upload nothing (one size is kept).  BPE_E_LIMIT, decided on the host from the merge list before any device work:
 * the table would hold more than 2^28 ids (which also keeps every single expansion below 2^31), or n times the
 * longest expansion reaches 2^62.
 * Runs on the ctx's stream and synchronises it before returning; keeps no pointer of the caller's; only counters cross
 * PCIe per call.  The decode vocab table is not touched.  The lengths and their scan are the ctx's decode scratch, shared
 * with bpe_decode_batch: a result of that call not yet read is dropped. */
int bpe_project_set_merges(bpe_ctx *ctx, const int32_t *merges, int32_t M,
                           const int32_t *pass_ids, int32_t n_pass);
int bpe_project_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n, int32_t vocab_size,
                         const uint64_t *d_doc_token_offsets, uint64_t k,
                         void *d_out, uint64_t out_cap, uint64_t *d_doc_out_offsets,
                         uint64_t *n_out, uint64_t *bad_index);

/* ---- token counts: id histogram and the compression curve ------------- */
/* How often each id occurs in ids that live in HBM, and from that histogram alone -- no second look at the ids -- the
 * histogram and the token count at every smaller vocabulary.
 *   bins             B = 256 + M + P of them, M and the P pass ids being those of bpe_project_set_merges: bin t for
 *                    0 <= t < 256 + M, bin 256 + M + j for the j-th pass id in ascending order
 *   bpe_count_resident   d_counts[i] = occurrences of bin i's id among the n ids of d_ids (DEVICE buffers, the caller's)
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes at any address aligned to id_width, read in place; a 64-bit id
 *                    is compared at its full width
 *   d_counts, n_bins B uint64; n_bins must equal B -- the caller's statement of the layout --, else BPE_E_ARG
 *   accumulate       0: d_counts[i] = the count; otherwise d_counts[i] += the count (a corpus larger than HBM, batch by
 *                    batch)
 *   *bad_index       first position whose id has no bin (~0 if none): BPE_E_ARG, and nothing is written to d_counts, in
 *                    either mode
 * Nothing outside d_counts[0, B) is ever written.  n = 0 is BPE_OK: zeros, or the array as it is when accumulating.
 * BPE_E_STATE before bpe_project_set_merges; BPE_E_ARG: id_width not 4 or 8, d_ids = NULL with n > 0, d_counts = NULL, a
 * misaligned pointer.  The call counts into a scratch of the ctx's own -- the first "count_lds_bins" bins (32768;
 * 256..32768, a multiple of 256) in LDS tables private to a workgroup, flushed at the end and every "count_flush" ids of
 * a workgroup (2^31; 64..2^31), the rest by 64-bit adds to memory; "count_combine" (0): 1 = equal ids among the 16 bytes
 * a lane loads are one add instead of one add per id -- and commits it to d_counts once the host has read
 * back that no id was bad.  Runs on the ctx's stream and synchronises it before returning; keeps no pointer of the
 * caller's; one counter crosses PCIe.  The decode scratch, a bpe_decode_batch result not yet read, the decode table and
 * the projection table are not touched.
 *   bpe_count_fold   host only, no ctx.  counts: a histogram in the layout above (n_bins >= 256 + M words; those from
 *                    256 + M on are pass bins).  Undoing merge t -> (a, b) adds counts[t] tokens and moves counts[t]
 *                    into a's and b's bins; t walks from 255 + M down
 *   folded           n_bins words or NULL: the histogram at vocab_size -- bins [vocab_size, 256 + M) zero, pass bins
 *                    unchanged
 *   curve            M + 1 words or NULL: curve[k] = tokens at 256 + k entries; curve[M] = the sum of all bins,
 *                    curve[k] = curve[k + 1] + (the histogram at 256 + k + 1 entries)[256 + k]
 * BPE_E_ARG: a merge list of another shape than bpe_project_set_merges takes, vocab_size outside [256, 256 + M],
 * n_bins < 256 + M, counts = NULL.  Every add is checked: a sum of 2^64 or more is BPE_E_LIMIT, and the outputs are then
 * undefined. */
int bpe_count_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                       uint64_t *d_counts, uint64_t n_bins, int32_t accumulate, uint64_t *bad_index);
int bpe_count_fold(const int32_t *merges, int32_t M, const uint64_t *counts, uint64_t n_bins,
                   int32_t vocab_size, uint64_t *folded, uint64_t *curve);

/* ---- document selection: gather, filter and shuffle ids in HBM -------- */
/* Which documents of an id stream that lives in HBM go on, and in what order: a shuffle, a filter or a sample in front
 * of rows, decode, spans, projection and counts.  Every large buffer is ON THE DEVICE and owned by the caller.
 *   off              the n_docs + 1 entries of d_doc_offsets; len(d) = off[d + 1] - off[d]
 *   selection j      d = index[j];  l_j = len(d) if max_len == 0, otherwise min(len(d), max_len);
 *                    s_j = off[d], or off[d + 1] - l_j with BPE_SELECT_TAIL
 *   out              ids[s_0 : s_0 + l_0] | ids[s_1 : s_1 + l_1] | ...
 *   out_offsets[j]   l_0 + ... + l_{j-1}; out_offsets[m] is the total
 * index may repeat documents, name them in any order and leave any out; m = 0 gives an empty output with
 * out_offsets = [0].
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_doc_offsets    validated on the device exactly as in bpe_rows_resident: ascending, none beyond n.  The first bad
 *                    entry goes to *bad_doc (~0 if none) and the call fails with BPE_E_ARG.  Ids before off[0] or at or
 *                    after off[n_docs] belong to no document and can never reach the output
 *   d_index, m       m int64 document numbers, each in [0, n_docs), compared at its full 64 bits (a negative one does not
 *                    wrap).  The lowest offending j goes to *bad_sel (~0 if none) and the call fails with BPE_E_ARG.
 *                    Offsets are checked first.  On either failure nothing is written to d_out or d_out_offsets
 *   max_len, flags   max_len = 0: whole documents; otherwise at most max_len ids of each, its head, or its tail with
 *                    BPE_SELECT_TAIL
 *   d_out, out_cap   receives the ids, of the input's width; NULL / 0 = only count.  Must not overlap d_ids: the
 *                    caller's contract.  out_cap < total fails with BPE_E_CAP and leaves d_out untouched
 *   d_out_offsets    m + 1 words, never NULL; written by a count-only call and on BPE_E_CAP too
 *   *n_out           the total, set as soon as it is known, also on BPE_E_CAP
 * Never writes d_out[out_cap] or beyond, nor anything outside d_out_offsets[0, m], whatever the alignment of d_out (to
 * id_width it must be aligned, as d_ids; 16-byte stores are used where the address allows).
 * BPE_E_ARG before any device work: id_width not 4 or 8, an unknown flag, BPE_SELECT_TAIL with max_len == 0, d_index =
 * NULL with m > 0, d_ids = NULL with n > 0, d_doc_offsets or d_out_offsets NULL, a misaligned pointer.  BPE_E_LIMIT:
 * n >= 2^32 (as for rows; it also makes every l_j and s_j fit 32 bits), m >= 2^32, n_docs >= 2^48; the total itself is
 * 64-bit -- repetition can take it past 2^32.
 * The placement is laid out by the output: "sel_tile" elements per workgroup, the output starts inside a tile staged in
 * LDS ("sel_stage" of them; bpe_set_option).  Runs on the ctx's stream and synchronises it before returning; keeps no
 * pointer of the caller's; only counters cross PCIe.  The lengths, their scan and the sources s_j are the ctx's decode
 * scratch, shared with bpe_decode_batch: a result of that call not yet read is dropped.  The decode vocab table, the
 * projection table and the count scratch are not touched. */
#define BPE_SELECT_TAIL 1u
int bpe_select_docs_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                             const uint64_t *d_doc_offsets, uint64_t n_docs,
                             const int64_t *d_index, uint64_t m,
                             uint64_t max_len, uint32_t flags,
                             void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                             uint64_t *n_out, uint64_t *bad_doc, uint64_t *bad_sel);

/* ---- document de-duplication: exact first copies, found in HBM -------- */
/* Which documents of an id stream that lives in HBM are copies of an earlier one: the mask "keep one copy of each" that
 * bpe_select_docs_resident takes, made without the ids leaving the device.  Every large buffer is ON THE DEVICE and
 * owned by the caller.
 *   key(d)           the slice bpe_select_docs_resident emits for document d with the same max_len and flags:
 *                    ids[s_d : s_d + l_d], l_d = len(d) or min(len(d), max_len), s_d = off[d] or off[d + 1] - l_d
 *   key(d) == key(e) the same length and the same ids at their full width: two int64 ids that differ only above bit 32
 *                    differ; empty keys are equal to each other
 *   first[d]         the lowest e with key(e) == key(d): first[d] <= d, first[first[d]] == first[d], and
 *                    first[d] == d marks the copy to keep
 *   counts[d]        the number of documents with d's key where first[d] == d, and 0 elsewhere
 *   *n_distinct      the number of d with first[d] == d
 * The result is exact and does not depend on scheduling: a hash of the key chooses where a table of document numbers
 * is probed and spares comparisons, and every equality reported has been established by comparing the ids themselves.
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_doc_offsets    validated on the device exactly as in bpe_rows_resident: ascending, none beyond n.  The first bad
 *                    entry goes to *bad_doc (~0 if none), the call fails with BPE_E_ARG and nothing is written to
 *                    d_first or d_counts
 *   max_len, flags   as in bpe_select_docs_resident: 0 = whole documents, BPE_SELECT_TAIL = the last max_len ids
 *   d_first          n_docs int64 words (NULL only with n_docs == 0)
 *   d_counts         n_docs words, or NULL: not wanted
 * n_docs == 0 is BPE_OK with *n_distinct = 0 and nothing written.
 * BPE_E_ARG before any device work: id_width not 4 or 8, an unknown flag, BPE_SELECT_TAIL with max_len == 0, d_ids =
 * NULL with n > 0, d_doc_offsets NULL, d_first NULL with n_docs > 0, a misaligned pointer (d_ids to id_width, the others
 * to 8 bytes).  BPE_E_LIMIT, before anything is launched or allocated: n >= 2^32, n_docs >= 2^32 - 1 (document numbers
 * are 32-bit words with ~0 for "none").
 * Three passes (bpe_set_option: "dup_tile", "dup_wave_len", "dup_hash_bits"): the keys' hashes in one read of the
 * stream, laid out by the ids and not by the documents; the insertion into an open-addressing table of the power of
 * two >= 2 n_docs slots, with the full comparisons; first and counts.  Runs on the ctx's stream and synchronises it
 * before returning; keeps no pointer of the caller's; only counters cross PCIe.  Its scratch (8 + 12 bytes per
 * document and the table) is a group of its own, grow-only: no other call's pending result is touched -- unlike
 * selection it leaves the decode scratch alone. */
int bpe_dup_docs_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                          const uint64_t *d_doc_offsets, uint64_t n_docs,
                          uint64_t max_len, uint32_t flags,
                          int64_t *d_first, uint64_t *d_counts,
                          uint64_t *n_distinct, uint64_t *bad_doc);

/* ---- near-duplicate documents: MinHash signatures, made in HBM -------- */
/* The MinHash signature of every document of an id stream that lives in HBM: n_perm int32 words per document, such
 * that the share of positions at which two rows agree estimates the Jaccard similarity of the two documents' sets of
 * ngram-id windows.  Banding the rows (bpe_dup_docs_resident on d_sig as an int32 stream) finds candidates,
 * bpe_minhash_agree_resident verifies them, and the result is a `first` column that bpe_select_docs_resident takes: all
 * without the ids leaving the device.  Every large buffer is ON THE DEVICE and owned by the caller.  All arithmetic is
 * unsigned; "& M32" is mod 2^32.
 *   fmix32(h)        h ^= h >> 16; h = h * 0x85EBCA6B & M32; h ^= h >> 13; h = h * 0xC2B2AE35 & M32; h ^= h >> 16
 *   tok(x)           x sign-extended to 64 bits (an int32 id and the int64 id of the same value hash alike; two int64
 *                    ids that differ only above bit 32 do not): lo = x & M32, hi = x >> 32;
 *                    tok = fmix32(lo ^ (hi * 0x9E3779B1 & M32))
 *   key(d)           the slice bpe_select_docs_resident emits for document d with the same max_len and flags, length l
 *   shingles(d)      window w = ngram.  l == 0: none.  ww = min(w, l); m = l - ww + 1 shingles; for i in [0, m):
 *                    s = 0; for k in [0, ww): s = (s * 0x01000193 + tok(key[i + k])) & M32;
 *                    S_i = fmix32(s ^ ((seed ^ ww) & M32)).  A key shorter than the window is ONE shingle, all of it;
 *                    a shingle never crosses a document's end, nor the end of the key where max_len cuts it
 *   A_p, B_p         z = seed; for p in [0, n_perm): A_p = next() | 1, B_p = next(); next() is splitmix64:
 *                    z = z + 0x9E3779B97F4A7C15; r = z; r = (r ^ r >> 30) * 0xBF58476D1CE4E5B9;
 *                    r = (r ^ r >> 27) * 0x94D049BB133111EB; return r ^ r >> 31 (all mod 2^64).  Made on the host and
 *                    uploaded, at most 16 KiB
 *   sig[d][p]        min_i ((A_p * S_i + B_p) mod 2^64) >> 33: a value in [0, 2^31), an int32 that is never negative;
 *                    no shingle (an empty key): 0x7FFFFFFF for every p
 * The result does not depend on scheduling: a minimum is the same in whatever order its terms are folded.
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_doc_offsets    validated on the device exactly as in bpe_rows_resident: ascending, none beyond n.  The first bad
 *                    entry goes to *bad_doc (~0 if none), the call fails with BPE_E_ARG and nothing is written to d_sig.
 *                    Ids before off[0] or at or after off[n_docs], and ids beyond max_len, enter no shingle
 *   max_len, flags   as in bpe_select_docs_resident: 0 = whole documents, BPE_SELECT_TAIL = the last max_len ids
 *   ngram            1..64
 *   n_perm           1..1024; it need not be a multiple of 64
 *   d_sig, sig_cap   int32 [n_docs][n_perm], row-major; sig_cap = the words there is room for (NULL only with
 *                    n_docs == 0).  sig_cap < n_docs * n_perm fails with BPE_E_CAP and nothing is written
 * n_docs == 0 is BPE_OK with nothing written.
 * BPE_E_ARG before any device work: id_width not 4 or 8, an unknown flag, BPE_SELECT_TAIL with max_len == 0, ngram
 * outside [1, 64], n_perm outside [1, 1024], d_ids = NULL with n > 0, d_doc_offsets NULL, d_sig NULL with n_docs > 0, a
 * misaligned pointer (d_ids to id_width, d_doc_offsets to 8 bytes, d_sig to 4).  BPE_E_LIMIT, before anything is
 * launched or allocated: n >= 2^32, n_docs >= 2^32 - 1, n_docs * n_perm >= 2^40.
 * Never writes a word outside d_sig[0, n_docs * n_perm).
 * Two passes (bpe_set_option: "mh_tile"): the rows of empty keys, and of keys whose shingles lie in more than one strip
 * of the next pass, are set to 0x7FFFFFFF; then one read of the stream, laid out by the ids and not by the documents --
 * per tile the shingle that starts at every position goes to LDS, and every wave walks a strip of them with a
 * permutation per lane: a key inside one strip is one plain store per word, the others fold by atomicMin.  Runs on the
 * ctx's stream and synchronises it before returning; keeps no pointer of the caller's; only the parameters and counters
 * cross PCIe.  Its scratch (16 n_perm bytes) is a group of its own, grow-only: the decode scratch and every other
 * call's pending result are left alone. */
int bpe_minhash_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                         const uint64_t *d_doc_offsets, uint64_t n_docs,
                         uint64_t max_len, uint32_t flags,
                         uint32_t ngram, uint32_t n_perm, uint64_t seed,
                         int32_t *d_sig, uint64_t sig_cap,
                         uint64_t *bad_doc);
/* At how many positions two signatures agree: agree[j] = #{p : sig[a_j][p] == sig[b_j][p]}, for m pairs of rows of a
 * signature matrix in HBM; agree[j] / n_perm estimates the Jaccard similarity of documents a_j and b_j.
 *   d_sig            int32 [n_docs][n_perm], row-major, read in place, never written
 *   d_a, d_b, m      m int64 document numbers each, in [0, n_docs), compared at their full 64 bits (a negative one does
 *                    not wrap); a_j == b_j and repeated pairs are fine.  The lowest j at which a_j or b_j is outside
 *                    goes to *bad_pair (~0 if none), the call fails with BPE_E_ARG and nothing is written to d_agree
 *   d_agree          m int32 words
 * m == 0 is BPE_OK with nothing written.
 * BPE_E_ARG before any device work: n_perm outside [1, 1024]; with m > 0, d_a, d_b or d_agree NULL, or d_sig NULL with
 * n_docs > 0; a misaligned pointer (d_sig and d_agree to 4 bytes, d_a and d_b to 8).  BPE_E_LIMIT: n_docs >= 2^32 - 1,
 * n_docs * n_perm >= 2^40.
 * Never writes a word outside d_agree[0, m).  16 lanes per pair, 16-byte loads where n_perm % 4 == 0 and d_sig is
 * 16-byte aligned.  Runs on the ctx's stream and synchronises it before returning; keeps no pointer of the caller's;
 * only a counter crosses PCIe; no scratch besides that counter. */
int bpe_minhash_agree_resident(bpe_ctx *ctx, const int32_t *d_sig, uint64_t n_docs, uint32_t n_perm,
                               const int64_t *d_a, const int64_t *d_b, uint64_t m,
                               int32_t *d_agree,
                               uint64_t *bad_pair);

/* ---- n-gram overlap: documents that share a window with a held-out set -------- */
/* Decontamination: which documents of an id stream in HBM contain a window of w = ngram consecutive ids that also
 * occurs in a reference stream (benchmarks, eval splits, a block list).  bpe_ngram_index_resident makes the ctx's index
 * of the reference windows, bpe_ngram_overlap_resident looks every window of a corpus up in it.  Every large buffer is ON
 * THE DEVICE and owned by the caller.  The definition (tests/ngram_model.py is its executable form):
 *   reference        R [n_ref] with roff [n_ref_docs + 1].  For every reference document r and every i with
 *   windows          roff[r] <= i and i + w <= roff[r + 1], the tuple R[i : i + w) is a reference window.  A reference
 *                    document shorter than w contributes nothing; ids outside [roff[0], roff[n_ref_docs]) contribute nothing
 *   equality         two windows are equal when they hold the same ids at their full width, by value: an int32 id and
 *                    the int64 id of the same value are equal, two int64 ids that differ only above bit 32 are not;
 *                    negative ids are values like any other
 *   low(W)           for every distinct reference window W, the lowest stream position i at which it starts
 *   key(d)           the slice bpe_select_docs_resident emits for document d of ids [n], off [n_docs + 1] with the same
 *                    max_len and flags: start s_d, length l_d
 *   hits             a window of the key starts at every key position k with k + w <= l_d; it is a hit if it equals
 *                    some reference window.  A key shorter than w has no window (it is not shortened)
 *   hits[d]          the number of hit positions (0 when the key has no window or the index is empty)
 *   first[d]         (s_d - off[d]) + k for the lowest hit k, -1 when there is none: a position inside the uncut document
 *   ref_pos[d]       low(W) for the window W at that first hit, -1 when there is none: an absolute position in R
 *   starts[p]        uint8, 1 where a hit window starts at stream position p and 0 at every other of the n positions
 * Exact, and the result does not depend on scheduling: a hash only chooses where to look, every equality is established
 * by comparing ids, counts are sums and first / ref_pos are minima.
 *
 * bpe_ngram_index_resident builds the ctx's ONE n-gram index, replacing any earlier one.  The ctx keeps its own copy of
 * the reference ids, sign-extended to 64 bits, so that a corpus of either width is compared by value: the caller may free
 * its buffers when the call returns.
 *   d_ref_ids, id_width  n_ref ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_ref_offsets    validated on the device exactly as in bpe_rows_resident: ascending, none beyond n_ref.  The first
 *                    bad entry goes to *bad_doc (~0 if none) and the call fails with BPE_E_ARG
 *   ngram            1..64
 *   *index_id        a non-zero number, new for every successful build on this ctx (required)
 *   *n_windows       the reference windows, repeats counted;  *n_distinct: the distinct ones (either may be NULL)
 * An index without a window (n_ref_docs == 0, every reference document shorter than ngram) is valid.  A call that
 * fails, for whatever reason, leaves the ctx WITHOUT an index.
 * BPE_E_ARG before any device work: id_width not 4 or 8, ngram outside [1, 64], d_ref_ids = NULL with n_ref > 0,
 * d_ref_offsets or index_id NULL, a misaligned pointer (d_ref_ids to id_width, d_ref_offsets to 8 bytes).  BPE_E_LIMIT,
 * before anything is launched or allocated: n_ref >= 2^32, n_ref_docs >= 2^32 - 1.
 * Passes (bpe_set_option: "ng_tile", "ng_hash_bits"): the copy; then the window pass over it -- laid out by the stream,
 * the ids of a tile and their halo in LDS, a lane per position -- which puts every window into an open-addressing table
 * of more than twice as many slots, a power of two: a slot is claimed by atomicCAS with tag << 32 | position and holds
 * that for good, repeats fold their position into the slot's lowest by atomicMin.  The index (8 n_ref bytes and 12 per
 * slot) is a scratch group of its own, grow-only: no other entry point touches it, it survives every other call on the
 * ctx and is freed with it.  Only the counters {first bad entry, roff[0], roff[n_ref_docs]}, {windows, distinct} cross PCIe.
 *
 * bpe_ngram_overlap_resident:
 *   index_id         must be the ctx's current index, otherwise BPE_E_STATE: 0, a replaced index, and any id after a
 *                    failed rebuild
 *   d_ids, id_width  n ids of 4 or 8 bytes -- either width against an index of either --, read in place, never written
 *   d_doc_offsets    validated as above; the first bad entry goes to *bad_doc, BPE_E_ARG, nothing is written
 *   max_len, flags   as in bpe_select_docs_resident: 0 = whole documents, BPE_SELECT_TAIL = the last max_len ids
 *   d_hits           int64 [n_docs] (NULL only with n_docs == 0);  d_first, d_ref_pos: int64 [n_docs], each may be NULL
 *   d_starts         uint8 [n], may be NULL; all n bytes are written
 *   *n_hit_docs      the documents with hits > 0
 * n_docs == 0 is BPE_OK with nothing written but d_starts.
 * BPE_E_ARG before any device work: id_width not 4 or 8, an unknown flag, BPE_SELECT_TAIL with max_len == 0, d_ids =
 * NULL with n > 0, d_doc_offsets NULL, d_hits NULL with n_docs > 0, a misaligned pointer (d_ids to id_width, the others
 * but d_starts to 8 bytes).  BPE_E_LIMIT: n >= 2^32, n_docs >= 2^32 - 1.  Nothing is written to any output before the
 * last check has passed.
 * The same window pass over the corpus, the table read-only: per position the window's hash, then the probe -- an empty
 * slot means no hit, a slot whose tag agrees is compared id by id, the window's own ids from LDS against the index's
 * 64-bit copy.  Per document the hits fold by atomicAdd and (first, ref_pos) together by one 64-bit atomicMin on
 * first << 32 | low; a last small pass unpacks into the caller's columns.  Runs on the ctx's stream and synchronises it
 * before returning; keeps no pointer of the caller's; only the counters {first bad entry, off[0], off[n_docs]},
 * {n_hit_docs} cross PCIe.  Its rows (12 bytes per document) are a scratch group of their own, grow-only. */
int bpe_ngram_index_resident(bpe_ctx *ctx, const void *d_ref_ids, int32_t id_width, uint64_t n_ref,
                             const uint64_t *d_ref_offsets, uint64_t n_ref_docs, uint32_t ngram,
                             uint64_t *index_id, uint64_t *n_windows, uint64_t *n_distinct, uint64_t *bad_doc);
int bpe_ngram_overlap_resident(bpe_ctx *ctx, uint64_t index_id, const void *d_ids, int32_t id_width, uint64_t n,
                               const uint64_t *d_doc_offsets, uint64_t n_docs, uint64_t max_len, uint32_t flags,
                               int64_t *d_hits, int64_t *d_first, int64_t *d_ref_pos, uint8_t *d_starts,
                               uint64_t *n_hit_docs, uint64_t *bad_doc);

/* ---- repetition statistics: repeated n-grams inside each document -------- */
/* The repetition filters of the Gopher / MassiveText rules on an id stream in HBM: how often the windows of w = ngram
 * consecutive ids of a document occur again inside the SAME document.  Every large buffer is ON THE DEVICE and owned by
 * the caller.  The definition (tests/repetition_model.py is its executable form):
 *   key(d)           the slice bpe_select_docs_resident emits for document d of ids [n], off [n_docs + 1] with the same
 *                    max_len and flags: start s_d, length l_d
 *   windows          a window starts at every key position k with k + w <= l_d.  A key shorter than w has no window (it
 *                    is not shortened)
 *   equality         two windows of the same document are equal when they hold the same ids at their full width: two
 *                    int64 ids that differ only above bit 32 are different; negative ids are values like any other.
 *                    Windows of different documents are never compared
 *   repeat           position k is a repeat if an equal window starts at a lower key position of the same document
 *   length[d]        l_d
 *   windows[d]       max(0, l_d - w + 1)
 *   distinct[d]      the number of distinct windows (= windows - repeats)
 *   covered[d]       the number of key positions i that lie inside a window at a repeat: some repeat k with
 *                    k <= i < k + w -- the token form of Gopher's "fraction inside duplicated n-grams"
 *   top_count[d]     the largest multiplicity of any window of the document, 0 without a window
 *   top_pos[d]       (s_d - off[d]) + the lowest start of the window with that multiplicity, among several such windows
 *                    the one whose first start is lowest; -1 without a window: a position inside the uncut document
 *   marks[p]         uint8 [n].  Bit 0: a repeat window starts at stream position p; bit 1: p is covered; 0 at every
 *                    other of the n positions
 * Exact, and the result does not depend on scheduling: a hash only chooses where to look, every equality is established
 * by comparing ids, counts are sums, lowest starts are minima and the top window is one maximum over
 * count << 32 | (2^32 - 1 - lowest start).
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_doc_offsets    validated on the device exactly as in bpe_rows_resident: ascending, none beyond n.  The first bad
 *                    entry goes to *bad_doc (~0 if none), the call fails with BPE_E_ARG and nothing is written
 *   ngram            1..64
 *   max_len, flags   as in bpe_select_docs_resident: 0 = whole documents, BPE_SELECT_TAIL = the last max_len ids
 *   d_length .. d_top_pos  int64 [n_docs] each, each may be NULL;  d_marks: uint8 [n], may be NULL, all n bytes are
 *                    written.  With n_docs > 0 at least one of the seven must be given
 *   *n_repeat_docs   the documents with distinct < windows
 * n_docs == 0 is BPE_OK with nothing written but d_marks (zeroed).
 * BPE_E_ARG before any device work: id_width not 4 or 8, ngram outside [1, 64], an unknown flag, BPE_SELECT_TAIL with
 * max_len == 0, d_ids = NULL with n > 0, d_doc_offsets NULL, no output with n_docs > 0, a misaligned pointer (d_ids to
 * id_width, the others but d_marks to 8 bytes).  BPE_E_LIMIT, before anything is launched or allocated: n >= 2^32,
 * n_docs >= 2^32 - 1.  Nothing is written to any output before the last check has passed.
 * Passes (bpe_set_option: "rp_tile", "rp_hash_bits"), all laid out by the stream, a tile per workgroup, a lane per
 * position: INSERT -- the ids of a tile and their halo of w - 1 in LDS; every window goes into an open-addressing table
 * of two slots per position of [off[0], off[n_docs]), in which every key owns the slots of its own positions -- twice as
 * many as it has windows, so that windows of different documents never meet and the probes of a tile stay as local as
 * its ids --: a slot is claimed by atomicCAS with tag << 32 | position, a window with the same ids joins it (its own ids
 * from LDS against the stream at the slot's position), and folds its position into the slot's lowest by atomicMin and 1
 * into its count; READ -- the same walk after the insert pass has completed: a position
 * that is not its slot's lowest is a repeat, the one that is speaks for its class by one 64-bit atomicMax; COVER -- the
 * repeat marks of a tile and of the w - 1 positions before it as bits in LDS; FINISH -- the rows into the caller's
 * columns.  Nothing is read outside [off[0], off[n_docs]).  Runs on the ctx's stream and synchronises it before
 * returning; keeps no pointer of the caller's; only the counters {first bad entry, off[0], off[n_docs]},
 * {n_repeat_docs} cross PCIe.
 * Limits: the table is 16 bytes per slot, two slots per id -- 32 bytes per id --, the rows 16 bytes per document, and a call without d_marks keeps n bytes of marks of its own: a scratch group of its own,
 * grow-only, freed with the ctx.  The call leaves the ctx's n-gram index and every other entry point's results alone. */
int bpe_repeat_stats_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                              const uint64_t *d_doc_offsets, uint64_t n_docs, uint32_t ngram,
                              uint64_t max_len, uint32_t flags,
                              int64_t *d_length, int64_t *d_windows, int64_t *d_distinct, int64_t *d_covered,
                              int64_t *d_top_count, int64_t *d_top_pos, uint8_t *d_marks,
                              uint64_t *n_repeat_docs, uint64_t *bad_doc);

/* ---- span de-duplication: windows an earlier document already holds -------- */
/* The exact-substring de-duplication of Lee et al. ("Deduplicating training data makes language models better") and the
 * span removal of RefinedWeb on an id stream in HBM: which windows of w = ngram consecutive ids of a document were already
 * seen in an EARLIER document of the same stream -- the licence text, the menu, the signature that otherwise different
 * documents share.  Every large buffer is ON THE DEVICE and owned by the caller.  The definition
 * (tests/dupspans_model.py is its executable form):
 *   key(d)           the slice bpe_select_docs_resident emits for document d of ids [n], off [n_docs + 1] with the same
 *                    max_len and BPE_SELECT_TAIL: start s_d (an absolute stream position), length l_d
 *   windows          a window starts at every absolute position p with s_d <= p and p + w <= s_d + l_d.  A key shorter
 *                    than w has none
 *   equality         two windows are equal when they hold the same ids at their full width: two int64 ids that differ
 *                    only above bit 32 differ; negative ids are values like any other.  Windows of ALL documents are
 *                    compared with one another
 *   low(W)           the lowest absolute position at which a window equal to W starts, over all keys
 *   seen             the window at p in document d is seen if low(W) < s_d: an equal window starts inside an earlier
 *                    document's key (the default scope).  With BPE_SPANS_ANYWHERE it is seen if low(W) < p: every
 *                    occurrence but the stream's first, in-document repeats included -- Lee et al.'s rule
 *   length[d]        l_d
 *   windows[d]       max(0, l_d - w + 1)
 *   seen[d]          the number of seen positions
 *   covered[d]       the key positions i with k <= i < k + w for some seen k
 *   first[d]         (s_d - off[d]) + the lowest seen position relative to s_d, -1 without one: a position inside the
 *                    uncut document, like bpe_ngram_overlap_resident's first
 *   src_pos[d]       low(W) of the window at that first seen position, -1 without one: an absolute stream position;
 *                    upper_bound(off, src_pos) - 1 names the source document
 *   marks[p]         uint8 [n].  Bit 0: a seen window starts at stream position p; bit 1: p is covered; 0 at every other
 *                    of the n positions
 * Exact, and the result does not depend on scheduling: a hash only chooses where to look, every equality is established
 * by comparing ids, counts are sums, low, first and src_pos are minima -- first << 32 | low goes through one 64-bit
 * atomicMin, and equal windows share one low.
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_doc_offsets    validated on the device exactly as in bpe_rows_resident: ascending, none beyond n.  The first bad
 *                    entry goes to *bad_doc (~0 if none), the call fails with BPE_E_ARG and nothing is written
 *   ngram            1..64
 *   max_len, flags   as in bpe_select_docs_resident: 0 = whole documents, BPE_SELECT_TAIL = the last max_len ids;
 *                    BPE_SPANS_ANYWHERE = the scope above
 *   d_length .. d_src_pos  int64 [n_docs] each, each may be NULL;  d_marks: uint8 [n], may be NULL, all n bytes are
 *                    written.  With n_docs > 0 at least one of the seven must be given
 *   *n_docs_seen     the documents with seen > 0;  *n_windows: all windows;  *n_distinct: the distinct ones (each may be
 *                    NULL).  With BPE_SPANS_ANYWHERE the seen windows sum to n_windows - n_distinct
 * n_docs == 0 is BPE_OK with nothing written but d_marks (zeroed).
 * BPE_E_ARG before any device work: id_width not 4 or 8, ngram outside [1, 64], an unknown flag, BPE_SELECT_TAIL with
 * max_len == 0, d_ids = NULL with n > 0, d_doc_offsets NULL, no output with n_docs > 0, a misaligned pointer (d_ids to
 * id_width, the others but d_marks to 8 bytes).  BPE_E_LIMIT, before anything is launched or allocated: n >= 2^32,
 * n_docs >= 2^32 - 1.  Nothing is written to any output before the last check has passed.
 * Passes (bpe_set_option: "ds_tile", "ds_hash_bits"), all laid out by the stream, a tile per workgroup, a lane per
 * position: BUILD -- the ids of a tile and their halo of w - 1 in LDS; every window goes into ONE open-addressing table
 * of 2 positions + 1 slots over [off[0], off[n_docs]): a slot is claimed by atomicCAS with tag << 32 | position, a window
 * with the same ids joins it (its own ids from LDS against the stream at the slot's position: no copy of the stream is
 * made), and folds its position into the slot's lowest by atomicMin; QUERY -- the same walk after the build has
 * completed: every window finds the slot of its class, reads its lowest and applies the scope rule; COVER -- the cover
 * pass of bpe_repeat_stats_resident, unchanged, over this call's marks; FINISH -- the rows into the caller's columns.
 * Every probe loop carries its bound; a window the query does not find is counted and the call returns BPE_E_INTERNAL.
 * A stream none of whose positions can hold a window skips the passes.  Nothing is read outside [off[0], off[n_docs]).
 * Runs on the ctx's stream and synchronises it before returning; keeps no pointer of the caller's; only the counters
 * {first bad entry, off[0], off[n_docs]}, {n_windows, n_distinct, windows not found, n_docs_seen} cross PCIe.
 * Limits: the table is 16 bytes per slot, two slots per id -- 32 bytes per id --, the rows 16 bytes per document, and a
 * call without d_marks keeps n bytes of marks of its own: a scratch group of its own, grow-only, freed with the ctx.
 * The seen set lives for one call: a corpus larger than one stream needs an index with a lifetime like
 * bpe_ngram_index_resident's.  The call leaves the ctx's n-gram index, the repetition scratch and every other entry
 * point's results alone. */
#define BPE_SPANS_ANYWHERE 2u
int bpe_dup_spans_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                           const uint64_t *d_doc_offsets, uint64_t n_docs, uint32_t ngram,
                           uint64_t max_len, uint32_t flags,
                           int64_t *d_length, int64_t *d_windows, int64_t *d_seen, int64_t *d_covered,
                           int64_t *d_first, int64_t *d_src_pos, uint8_t *d_marks,
                           uint64_t *n_docs_seen, uint64_t *n_windows, uint64_t *n_distinct, uint64_t *bad_doc);

/* Cut marked ids out of a stream on the device: what the marks of bpe_dup_spans_resident and
 * bpe_repeat_stats_resident and the starts of bpe_ngram_overlap_resident are for (tests/dupspans_model.py: keep).
 *   kept             position p of [off[0], off[n_docs]) is kept iff (mask[p] & bits) != 0; with BPE_KEEP_DROP iff
 *                    (mask[p] & bits) == 0.  Ids outside that range are dropped
 *   out              the kept ids in order, in the width of d_ids
 *   out_offsets[d]   the number of kept positions in [off[0], off[d]), d = 0 .. n_docs: a document that loses everything
 *                    stays as an empty document, and document numbers do not change
 *   d_mask           uint8 [n], read inside [off[0], off[n_docs]) only;  bits: 1..255
 *   d_out, out_cap   d_out = NULL or out_cap = 0: a count-only call (*n_out and d_out_offsets are written all the same).
 *                    out_cap < total fails with BPE_E_CAP, *n_out set, d_out untouched
 *   d_out_offsets    n_docs + 1 words, never NULL
 * BPE_E_ARG before any device work: id_width not 4 or 8, bits outside [1, 255], an unknown flag, a NULL pointer but
 * d_out (d_ids and d_mask with n > 0), a misaligned pointer, d_out [out_cap] overlapping d_ids [n].  BPE_E_LIMIT: n >= 2^32.
 * Offsets are validated as in bpe_rows_resident (*bad_doc, BPE_E_ARG, nothing written).  A length pass (0 or 1 per
 * position), a scan and a placement pass by the skeleton bpe_project_resident and bpe_select_docs_resident share: it
 * uses the decode scratch (12 bytes per id) and drops a pending bpe_decode_batch result, as bpe_select_docs_resident
 * does.  Runs on the ctx's stream and synchronises it; only counters cross PCIe. */
#define BPE_KEEP_DROP 1u
int bpe_keep_ids_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                          const uint64_t *d_doc_offsets, uint64_t n_docs,
                          const uint8_t *d_mask, uint32_t bits, uint32_t flags,
                          void *d_out, uint64_t out_cap, uint64_t *d_out_offsets,
                          uint64_t *n_out, uint64_t *bad_doc);

/* The segments of every document -- its lines, with the class table of Tokenizer.segment_classes -- as an id stream of
 * its own, made on the device, so that every per-document call above becomes a per-segment call: the segment stream
 * and its seg_offsets are an (ids, doc_offsets) pair (tests/segments_model.py: segment_docs).
 *   class(t)         d_class[t] & 3 if 0 <= t < n_class, the id taken at its full width; 0 otherwise -- a negative id,
 *                    an id beyond the table, an int64 id whose low 32 bits happen to index it.  n_class == 0 or
 *                    d_class == NULL: every class is 0.  BPE_SEG_BREAK: a segment boundary lies BEHIND this id;
 *                    BPE_SEG_SKIP: the id belongs to no segment
 *   positions        only those of [off[0], off[n_docs]) take part
 *   the walk         inside a document, position by position, with one bit of state, FRESH or OPEN, FRESH at the
 *                    document's start.  A position without SKIP is content.  A content position seen in state FRESH
 *                    starts a segment.  Content sets the state to OPEN; BREAK sets it to FRESH behind the position;
 *                    SKIP alone leaves it as it is
 *   segment          the content from one start up to the next boundary or the document's end: none is empty, a
 *                    document may have none, none spans two documents
 *   out              the content ids of all segments in order, in the width of d_ids.  With BPE_SEG_TAG_DOC every
 *                    segment is preceded by one id that holds its document's number: equal segments of different
 *                    documents then differ, and a per-document call compares the segments of one document only
 *   seg_offsets[s]   where segment s begins in out (with BPE_SEG_TAG_DOC: its tag); seg_offsets[n_seg] = n_out
 *   seg_doc[s]       the segment's document;  doc_seg_offsets[d]: the segments in documents below d, d = 0 .. n_docs
 *   src_start[s], src_end[s]  a range of positions in d_ids: it begins at off[d] for the first segment of document d and
 *                    at the segment's first content position otherwise; it ends at the first content position of the
 *                    next segment of the same document, at off[d + 1] without one.  The ranges of a document's segments
 *                    tile the document: skipped ids and separators trail the segment in front of them, leading ones go
 *                    with the first segment
 * Exact, and the result does not depend on scheduling: every output is a function of the inputs through scans.
 *   d_ids, id_width  n ids of 4 (int32) or 8 (int64) bytes, read in place, never written
 *   d_doc_offsets    validated on the device exactly as in bpe_rows_resident: ascending, none beyond n.  The first bad
 *                    entry goes to *bad_doc (~0 if none), the call fails with BPE_E_ARG and nothing is written
 *   d_class, n_class uint8 [n_class], only the two low bits of an entry are read
 *   d_out, out_cap   d_out = NULL or out_cap = 0: a count-only call -- *n_out, *n_seg and d_doc_seg_offsets are written
 *                    all the same, nothing else
 *   d_seg_offsets, seg_cap  seg_cap + 1 words (NULL only in a count-only call);  d_seg_doc, d_src_start, d_src_end:
 *                    int64 [seg_cap] each, each may be NULL;  d_doc_seg_offsets: n_docs + 1 words, may be NULL
 *   *n_out, *n_seg   the totals (each may be NULL), set from the moment they are known
 * out_cap < n_out or seg_cap < n_seg fails with BPE_E_CAP, both totals set: nothing is written to d_out or to any
 * per-segment array, and never is anything written at or beyond a capacity.  n == 0, n_docs == 0 or empty documents
 * only: BPE_OK with totals 0 (d_doc_seg_offsets zeroed, seg_offsets[0] = 0 unless count-only).
 * BPE_E_ARG before any device work: id_width not 4 or 8, an unknown flag, d_ids = NULL with n > 0, d_doc_offsets NULL,
 * d_seg_offsets NULL with an output, a misaligned pointer (d_ids and d_out to id_width, the others but d_class to 8
 * bytes), d_out [out_cap] overlapping d_ids [n].  BPE_E_LIMIT, before anything is launched or allocated: n >= 2^32,
 * n_docs >= 2^32 - 1, BPE_SEG_TAG_DOC with id_width == 4 and n_docs > 2^31 (a tag would not fit), n_class > 2^26.
 * Passes (bpe_set_option: "seg_tile"): a segment start is no neighbour predicate -- SKIP ids in any number may lie
 * between a boundary and the next content -- but a scan over the monoid {identity, ->FRESH, ->OPEN}, "the last event
 * that is not the identity", a document start being ->FRESH in front of its position.  Document starts are a flag byte
 * per position, written by a pass over the documents (empty documents and several at one position are harmless).
 * CLASSIFY -- a tile per workgroup: the class of every id next to that flag, and the tile's summary byte; CARRY -- a
 * launch of its own, one workgroup: the exclusive scan of the summaries, across any number of all-identity tiles;
 * MARK -- per wave two ballots and a count of leading zeros below the lane, across the waves of a tile LDS, across
 * tiles the carried byte: a start flag and an output length per position; two scans (k_scan_*); PLACE -- out,
 * seg_offsets, seg_doc, src_start and the ends that a next segment sets (the one search of the call: per segment, for
 * its document); ENDS -- the ends that a document's end sets.  No workgroup waits for another inside a launch, and
 * every loop carries its bound.  Nothing is read outside [off[0], off[n_docs]).
 * Runs on the ctx's stream and synchronises it before returning; keeps no pointer of the caller's; only the counters
 * {first bad entry, off[0], off[n_docs]}, {n_out, n_seg} cross PCIe.
 * Scratch: the output lengths, their scan and the start flags use the decode scratch (16 bytes per id), so the call drops
 * a pending bpe_decode_batch result, as bpe_keep_ids_resident and bpe_select_docs_resident do; the flag bytes, the scan
 * of the starts and the tile summaries (9 bytes per id) are a group of its own, grow-only, freed with the ctx.  Every
 * other entry point's scratch and results are left alone. */
#define BPE_SEG_BREAK 1u
#define BPE_SEG_SKIP 2u
#define BPE_SEG_TAG_DOC 1u
int bpe_segment_docs_resident(bpe_ctx *ctx, const void *d_ids, int32_t id_width, uint64_t n,
                              const uint64_t *d_doc_offsets, uint64_t n_docs,
                              const uint8_t *d_class, uint64_t n_class, uint32_t flags,
                              void *d_out, uint64_t out_cap, uint64_t *d_seg_offsets, uint64_t seg_cap,
                              int64_t *d_seg_doc, int64_t *d_src_start, int64_t *d_src_end,
                              uint64_t *d_doc_seg_offsets,
                              uint64_t *n_out, uint64_t *n_seg, uint64_t *bad_doc);

/* Per-segment verdicts back as the marks bpe_keep_ids_resident takes (tests/segments_model.py: segment_marks).
 *   marks[p]         d_seg_val[s] where src_start[s] <= p < src_end[s], 0 at every other of the n positions: all n
 *                    bytes are written
 *   d_src_start, d_src_end  int64 [n_seg] each, as bpe_segment_docs_resident leaves them.  They must ascend without
 *                    overlap inside [0, n]: entry s is bad if start[s] < 0, end[s] < start[s], end[s] > n, or
 *                    start[s] < end[s - 1].  The first bad entry goes to *bad_seg (~0 if none), the call fails with
 *                    BPE_E_ARG and nothing is written.  Empty ranges and gaps between ranges are fine
 *   d_seg_val        uint8 [n_seg];  d_marks: uint8 [n]
 * n_seg == 0 writes n zeros.  BPE_E_ARG before any device work: a NULL pointer that is needed (the three inputs with
 * n_seg > 0, d_marks with n > 0), d_src_start or d_src_end not 8-byte aligned.  BPE_E_LIMIT: n >= 2^32, n_seg >= 2^32.
 * Passes (bpe_set_option: "seg_tile", "seg_stage"): a check of the ranges; then, laid out by the positions, a tile per
 * workgroup: one binary search for the tile's first range, the next "seg_stage" ranges staged in LDS, a lane searches
 * there once and walks on; a tile in which more ranges begin than are staged searches global memory -- the pattern of
 * bpe_select_docs_resident's placement.  Every loop carries its bound.  No scratch but a counter word.  Runs on the
 * ctx's stream and synchronises it; only the counter {first bad range} crosses PCIe. */
int bpe_segment_marks_resident(bpe_ctx *ctx, const int64_t *d_src_start, const int64_t *d_src_end, uint64_t n_seg,
                               const uint8_t *d_seg_val, uint64_t n, uint8_t *d_marks, uint64_t *bad_seg);

/* ---- measurement ------------------------------------------------------------ */
#define BPE_PROF_WIDEN 0
#define BPE_PROF_PAIR_COUNT 1
#define BPE_PROF_ARGMAX 2   /* rowmax + argmax + tie-break + finalize */
#define BPE_PROF_MERGE 3    /* merge pass(es) */
#define BPE_PROF_TABLE 4    /* delta apply / table clear */
#define BPE_PROF_ENCODE 5
#define BPE_PROF_DECODE 6
#define BPE_PROF_NKINDS 7
/* Accumulated since the last bpe_prof_reset: device ms (hipEvents on the ctx's
 * stream), launches, algorithmic bytes (4 B per id read or written,
 * tables and flags not counted). */
int bpe_prof_reset(bpe_ctx *ctx);
int bpe_prof_read(bpe_ctx *ctx, double *ms, uint64_t *launches, uint64_t *alg_bytes);
/* How the last bpe_train ran its merge passes: out[0] = dense passes (every slot of the stream
 * is visited), out[1] = sparse passes (only the slots the inverted slot index cannot rule out),
 * out[2] = builds of that index, out[3] = slots of the stream at the end. */
int bpe_train_stats(bpe_ctx *ctx, uint64_t *out4);
/* The same, extended: out[4] = merges done by lean iterations or chain steps (three launches per merge or per
 * batch of merges, the pair table updated at the merge sites themselves; options "lean", "chain"), out[5] =
 * merges they handed back to the general path (pairs with a == b, ties they could not settle), out[6] = merges
 * that needed no selection of their own (their pair came off the list of tied pairs an earlier selection made:
 * the reference merges those in order of first occurrence while their counts stand), out[7] = chain steps,
 * out[8] = chain steps that selected (gathered the pool of pairs anew; the others took their pairs off it), out[9] = ids
 * per slot the stream ended in (1024; 256 once it was re-packed for sparse passes, option "small_slots"), out[10] =
 * chain steps that were ONE launch (selection, merge pass and table update as phases of one resident grid: option
 * "fuse_step"), out[11] = merges of a pair with a == b that chain steps did themselves (option "chain_aa") instead of
 * handing them back, out[12] = chain steps whose batch held a first token twice (option "chain_share_first").
 * Writes min(n, 13) values. */
int bpe_train_stats_ex(bpe_ctx *ctx, uint64_t *out, int n);

/* ---- text.encode("utf-8") by all host threads (host, no GPU needed) ------------------ */
/* The first statement of every train() / encode() of the reference (basic.py:25, regex.py:44): an array of code
 * points of `kind` = 1, 2 or 4 bytes each (what a CPython str holds) as UTF-8, counted and written by segments in
 * parallel.  out may be NULL to only count (*n_bytes); BPE_E_CAP if cap is too small; BPE_E_ARG on a lone surrogate
 * or a value above 0x10FFFF (str.encode raises there: the caller leaves such a text to it).  threads <= 0: all cores. */
int bpe_utf8_encode(int kind, const void *code_points, uint64_t n_chars, uint8_t *out, uint64_t cap,
                    uint64_t *n_bytes, int threads);

/* ---- native pre-split (host, no GPU needed) ----------------------------- */
/* regex.findall(pattern, text) for the two GPT split patterns (regex.py:18-19, 41, 114),
 * as chunk START byte offsets into the UTF-8 text.  which: 2 = GPT-2 pattern, 4 = GPT-4
 * pattern (any other pattern stays with the `regex` module).  Both patterns match every
 * character, so the chunks partition the text.  starts_out may be NULL to only count;
 * returns BPE_E_CAP (with *n_chunks set) if cap is too small.  threads <= 0: all cores. */
int bpe_split(int which, const uint8_t *utf8, uint64_t n, uint64_t *starts_out, uint64_t cap,
              uint64_t *n_chunks, int threads);

/* The same for a batch of documents laid out back to back (document d starts at doc_offsets[d];
 * the last one ends at n): every document is split on its own, as a loop of encode() calls over
 * the documents would (regex.py:111-121).  doc_first_chunk (n_docs + 1 entries, may be NULL)
 * receives the index of each document's first chunk in starts_out. */
int bpe_split_docs(int which, const uint8_t *utf8, uint64_t n, const uint64_t *doc_offsets,
                   uint64_t n_docs, uint64_t *starts_out, uint64_t cap, uint64_t *n_chunks,
                   uint64_t *doc_first_chunk, int threads);

/* ---- chunk de-duplication (host, no GPU needed) ---------------------------- */
/* In: the chunk list of regex.py:41-44 as bytes + chunk START offsets (chunk c ends where
 * chunk c+1 starts, the last one at n).  Out: the distinct chunks in order of first
 * appearance, each emitted once per set bit k of its multiplicity with weight_exp = k (so
 * the emitted weights 2^k sum to the multiplicity).  The output never exceeds the input:
 * out_bytes needs n bytes, out_offsets and out_weight_exp need n_chunks entries.
 * threads <= 0: all cores. */
int bpe_dedup_chunks(const uint8_t *bytes, uint64_t n, const uint64_t *chunk_offsets, uint64_t n_chunks,
                     uint8_t *out_bytes, uint64_t *out_offsets, uint8_t *out_weight_exp,
                     uint64_t *n_out_bytes, uint64_t *n_out_chunks, uint64_t *n_distinct, int threads);

/* ---- host utilities (no GPU needed) ------------------------------------------ */
/* Deterministic synthetic UTF-8 text (SURVEY 8d synth_text): explicit
 * splitmix64, integer tables only.  Writes exactly n bytes, valid UTF-8. */
int bpe_synth_text(uint8_t *out, uint64_t n, uint64_t seed);
/* Library version / build info string. */
const char *bpe_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BPE_HIP_H */
