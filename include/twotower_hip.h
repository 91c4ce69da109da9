/*
 * twotower_hip.h — C ABI of the MI355X (gfx950) two-tower retrieval training hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no
 * torch / HIP C++ types.  All pointers are DEVICE pointers unless a comment says HOST.
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).  Every entry
 * point enqueues on `stream` and returns without synchronising; it never allocates.
 * Return value: TT_OK (0) or a TT_ERR_* code; tt_last_error() gives the message of the
 * calling thread's last failure.  No C++ exception crosses this boundary.
 *
 * What each group replaces in the reference (citations into /root/reference):
 *   - The reference declares the training path but ships no code for it:
 *       src/models/__init__.py:1, src/training/__init__.py:1 (docstring stubs);
 *       entry point `train-model = "src.training.train:main"`   pyproject.toml:67;
 *       hyper-parameter schema                                  configs/data_config.yaml:54-71.
 *     The arithmetic would have come from tensorflow / tensorflow-recommenders
 *     (pyproject.toml:22,24).  The ops below are what those packages' CPU kernels
 *     (tf.gather, Dense matmul, tfrs.tasks.Retrieval, Keras SGD/Adagrad) would run.
 *   - Inputs are the int64 ids produced by
 *       scripts/data_processing/prepare_training_data.py:113-123,209-210 (user_idx,item_idx)
 *       src/data/preprocessor.py:478-491 (user_id_encoded, item_id_encoded, category_encoded).
 *   - Serving - the exact, IVF and int8 top-K indices, and the MMR diversified re-ranking of the pool they return
 *     (tt_mmr_rerank_f32, the last group below) - is what tfrs.layers.factorized_top_k would have served; the
 *     reference's README promises it and its src/serving/ is empty.
 */
#ifndef TWOTOWER_HIP_H
#define TWOTOWER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TT_ABI_VERSION 10

enum {
  TT_OK = 0,
  TT_ERR_INVALID_ARG = 1,   /* null pointer, bad size/alignment, unsupported dim            */
  TT_ERR_LAUNCH = 2,        /* hipLaunch / hip runtime error                                */
  TT_ERR_UNSUPPORTED = 3,   /* valid request this build does not implement                  */
  TT_ERR_WORKSPACE = 4      /* caller-provided workspace too small                          */
};

enum { TT_OPT_SGD = 0, TT_OPT_ADAGRAD = 1 };
enum { TT_IDS_UNIFORM = 0, TT_IDS_POWERLAW = 1 };

typedef void* tt_stream_t;

int tt_abi_version(void);
const char* tt_last_error(void);
/* sizeof of the structs below as this library was built (0 tt_train_step, 1 tt_dense_fwd_args, 2 tt_dense_bwd_args,
 * 3 tt_sparse_table_ids, 4 tt_dense_seg, 5 tt_id_buckets, 6 tt_dense_lookup, 7 tt_l2norm_fwd_args, 8 tt_l2norm_bwd_args,
 * 10 tt_adam_table, 11 tt_adam_seg, 12 tt_adam_hyper, 14 tt_dense_features_fwd_args, 15 tt_dense_features_bwd_args,
 * 17 tt_cross_fwd_args, 18 tt_cross_bwd_args, 21 tt_layer_norm_fwd_args, 22 tt_layer_norm_bwd_args, 23 tt_clip_buffer,
 * 24 tt_rowwise_table; else -
 * 9, 13, 16, 19 and 20 included, which stay unassigned - -1): a binding checks its mirrors with it. */
int64_t tt_abi_struct_bytes(int32_t which);

/* ---------------------------------------------------------------------------------------
 * Built-in kernel timing (SURVEY.md §5 "Tracing / profiling": the reference has none).
 * tt_profile_enable("score_bwd,gather", 4096) makes every launch of the kernels carrying one
 * of those tags record a hipEvent pair on ITS OWN stream (capacity = launches kept per tag);
 * tags: fill, gather, sparse_plan, sparse_apply, dense_fwd, dense_bwd (dx+dw in one launch), dense_bwd_dx, dense_bwd_dw,
 * dense_update, optimizer (sparse + dense in one launch), score_fwd, score_bwd, score_fused, score_rank, score_aux, route, scatter_rows, encode_ids,
 * topk_select, topk_merge (and the scope topk around a whole tt_retrieval_topk_f32 call), ivf_bucket, ivf_select (and
 * the scope ivf around a whole tt_ivf_search_f32 call), quantize_i8, topk_i8_scan, topk_i8_rerank, topk_i8_scale (and the
 * scope topk_i8 around a whole tt_retrieval_topk_i8_f32 call), ivf_i8_select (and the scope ivf_i8 around a whole
 * tt_ivf_search_i8_f32 call, whose other launches carry the tags of the code they share: topk_select, topk_merge, ivf_bucket,
 * topk_i8_rerank, topk_i8_scale), l2norm_fwd, l2norm_bwd, adam_sparse, adam_finish (the two launches of tt_adam_step_f32), bag_fwd, bag_bwd, sample (tt_sample_candidates_i64),
 * features_fwd, features_bwd (tt_dense_features_*_f32), rating_fwd, rating_bwd (tt_rating_head_*_f32), cross_fwd, cross_bwd
 * (tt_cross_*_f32), layer_norm_fwd, layer_norm_bwd (tt_layer_norm_*_f32), rowwise_sparse, rowwise_finish (the two launches of
 * tt_rowwise_adagrad_step_f32), freq_update, freq_estimate (the two launches of tt_frequency_estimate_i64), mmr
 * (tt_mmr_rerank_f32).
 * An empty string (or NULL) disables it.
 * tt_profile_read synchronises on the recorded events, writes up to `cap` durations in
 * milliseconds (launch order) to the HOST array `ms`, stores the number of durations written in
 * *count (HOST) and clears the tag.  Disabled = one predictable branch per launch.           */
int tt_profile_enable(const char* tags_csv, int32_t capacity_per_tag);
int tt_profile_read(const char* tag, float* ms, int32_t cap, int32_t* count);
/* Bracket only every stride-th launch of a tag (default 1 = every launch).  A hipEventRecord is a barrier packet
 * that costs the stream 4-7 us: a whole-step throughput measurement that also wants live kernel durations
 * samples them (bench.py: every 4th step).                                                                  */
int tt_profile_set_stride(int32_t stride);

/* ---------------------------------------------------------------------------------------
 * Synthetic inputs (SURVEY.md §8d "Synthetic inputs"; no reference counterpart).
 * Counter-based splitmix64; bit-identical to oracle/synth.py.
 *   value(i) = fl32(fl32(u(start+i) * scale) + lo),  u in [0,1) with 24 bits.          */
int tt_fill_uniform_f32(float* dst, int64_t n, uint64_t seed, uint64_t tensor_id,
                        int64_t start, float lo, float scale, tt_stream_t stream);
/* Rows row_start, row_start+row_stride, ... of a [*, dim] tensor whose flat element (r, d) uses counter
 * r*dim + d: the shard of a row-sharded table (owner = row % world) without materialising the whole. */
int tt_fill_uniform_rows_f32(float* dst, int64_t n_rows, int32_t dim, int64_t row_start, int64_t row_stride,
                             uint64_t seed, uint64_t tensor_id, float lo, float scale, tt_stream_t stream);
/* ids in [0,num_rows): variant TT_IDS_UNIFORM or TT_IDS_POWERLAW (floor(N*u^4)).        */
int tt_fill_ids_i64(int64_t* dst, int64_t n, uint64_t seed, uint64_t tensor_id,
                    int64_t start, int64_t num_rows, int32_t variant, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a6/a7 — id encoding (scripts/data_processing/prepare_training_data.py:113-123,209-210 sorted(unique)+enumerate+map;
 * src/data/preprocessor.py:478-491 LabelEncoder().fit_transform): codes[i] = rank of string i among the sorted
 * DISTINCT strings, int64.  `rows` is an [n, width] uint8 matrix of UTF-8 bytes, zero-padded on the right, width a
 * multiple of 8, no NUL inside a string (Python str order = code-point order = UTF-8 byte order; a shorter string
 * that is a prefix sorts first, like the zero padding).  *n_unique (device int32, may be NULL) receives the vocabulary size. */
int64_t tt_encode_ids_workspace_bytes(int64_t n);
int tt_encode_ids_u8(const uint8_t* rows, int64_t n, int32_t width, void* workspace, int64_t workspace_bytes,
                     int64_t* codes, int32_t* n_unique, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a1 — embedding lookup (Keras Embedding / tf.gather; configs/data_config.yaml:55).
 *   out[b, :] = table[ids[b], :]          table [num_rows, dim] f32 row-major, dim % 4 == 0
 * Ids outside [0,num_rows) produce a zero row and set *oob_flag (device int32, may be
 * NULL) to 1 — the caller turns that into the error TF's CPU gather raises.  The id -1 is a
 * PADDING slot (fixed-capacity all-to-all buffers of the row-sharded path): zero row, no flag.
 * The `2` form gathers the user and the item table in ONE launch.                        */
int tt_embedding_gather_f32(const float* table, int64_t num_rows, int32_t dim,
                            const int64_t* ids, int64_t n_ids, float* out,
                            int32_t* oob_flag, tt_stream_t stream);
int tt_embedding_gather2_f32(const float* table_a, int64_t rows_a, const int64_t* ids_a, float* out_a,
                             const float* table_b, int64_t rows_b, const int64_t* ids_b, float* out_b,
                             int32_t dim, int64_t n_ids, int32_t* oob_flag, tt_stream_t stream);
/* A further feature summed into a tower input (BASELINE configs[4]: the hashed category feature added to the
 * item tower's input): out[p,:] += table[ids[p],:] (one f32 add per element; id -1 / out of range adds
 * nothing, out of range sets the flag).  Its gradient rows are the tower-input gradient rows themselves.  */
int tt_embedding_gather_add_f32(const float* table, int64_t num_rows, int32_t dim,
                                const int64_t* ids, int64_t n_ids, float* out,
                                int32_t* oob_flag, tt_stream_t stream);
/* Hash feature ids: out[i] = FNV-1a-64(bytes of row i up to its first NUL) mod n_buckets, rows as for
 * tt_encode_ids_u8 (zero-padded [n, width] u8).  The reference names no hash (SURVEY.md Appendix A "not
 * specified anywhere"); this one is restated in oracle/hashing.py.                                          */
int tt_hash_bucket_u8(const uint8_t* rows_u8, int64_t n, int32_t width, int64_t n_buckets,
                      int64_t* out, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Embedding bag (added to v10: new symbols only, the version is unchanged) - a bag of hashed token rows pooled into one
 * vector: TFRS TextVectorization -> Embedding -> GlobalAveragePooling1D, here the pooled item-title feature summed into the
 * item tower's input (csrc/bag.hip).
 * Layout: tokens [n_token_rows, L] int32 row-major, one row per item; the slot value -1 is PADDING and may stand anywhere
 * in a row.  table [table_rows, dim] f32, dim % 4 == 0, 4 <= dim <= 1024.
 * Forward.  Bag b pools token row bag_rows[b] (bag_rows [n_bags] int64; NULL = identity, then n_bags must equal
 * n_token_rows).  bag_rows[b] == -1 is an empty bag; any other value outside [0, n_token_rows) is an empty bag and sets
 * *oob_flag (device int32, may be NULL).  A slot is VALID when its token lies in [0, table_rows); padding slots are skipped,
 * any other token out of range is skipped and sets the flag; cnt = the number of valid slots.
 * Arithmetic (f32, one rounding per operation, no contraction): s = the first valid row, every further valid row added in
 * ascending slot order;
 *   pooling 0 (sum):    inv = 1            pooled = s
 *   pooling 1 (mean):   inv = 1 / cnt      pooled = s * inv          (correctly rounded division)
 *   pooling 2 (sqrtn):  inv = 1 / sqrt(cnt)  pooled = s * inv        (correctly rounded square root, then division)
 *   accumulate 1: out[b] = out[b] + pooled;  accumulate 0: out[b] = pooled.
 * An empty bag (cnt == 0) has inv = 0; with accumulate 1 its out row is not written, with accumulate 0 it is written as +0.
 * Optional outputs (either may be NULL): batch_ids [n_bags * L] int64 = the token of every slot, -1 for a skipped slot
 * (the ids tt_sparse_plan sorts); inv [n_bags] f32.
 * One launch; bit-reproducible, independent of the grid; table and out 16-byte aligned; n_bags * L must fit 31 bits.
 * n_bags == 0 launches nothing.  Anything else is TT_ERR_INVALID_ARG before any launch.
 * Backward (one launch, two results): gs[b, :] = dy[b, :] * inv[b] (gs may be NULL for sum pooling - the caller then uses
 * dy itself; gs may be dy) and order_bags[j] = order[j] / L for the n_ids = n_bags * L positions of a tt_sparse_plan over
 * batch_ids: the plan's slot positions turned into bag indices.  The table is then updated by tt_sparse_sgd_f32 /
 * tt_sparse_adagrad_f32 / tt_adam_step_f32 (n_tables = 1, n_segs = 0) with grads = gs and order = order_bags: n_bags * dim
 * floats of gradient traffic, no per-token gradient rows, and the duplicate sums in the documented order (runs cut at global
 * multiples of 64 sorted slots, slots in ascending position): bit-identical to an expansion into per-token rows.           */
int tt_embedding_bag_fwd_f32(const float* table, int64_t table_rows, int32_t dim,
                             const int32_t* tokens, int64_t n_token_rows, int32_t L,
                             const int64_t* bag_rows, int64_t n_bags, int32_t pooling, int32_t accumulate,
                             float* out, int64_t* batch_ids, float* inv, int32_t* oob_flag, tt_stream_t stream);
int tt_embedding_bag_bwd_f32(const float* dy, const float* inv, int64_t n_bags, int32_t dim, int32_t L,
                             const int32_t* order, int64_t n_ids, float* gs, int32_t* order_bags, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * History bag (added to v10: a new symbol only, the version is unchanged) - the pooled user-history feature: the bag of items
 * a user interacted with, pooled into the query tower's input (TFRS Embedding -> GlobalAveragePooling1D in the query model).
 * tt_embedding_bag_fwd_f32 - every argument, rule and rounding above - with two optional extensions, one launch either way:
 * exclude [n_bags] int64 (may be NULL): LEAVE-ONE-OUT.  Every slot of bag b whose token equals exclude[b] is skipped, on every
 *   occurrence: it is written to batch_ids as -1 (the sort plan never sees it, it gets no gradient) and does not count towards
 *   cnt / inv.  The compare is on the slot's raw token in int64, in front of the range check: the result is, bit for bit, what
 *   tt_embedding_bag_fwd_f32 gives on a token matrix whose matching slots were set to -1.  A value that matches no token
 *   (-1, any negative, any value >= table_rows) excludes nothing and sets no flag.  A bag whose valid slots are all excluded
 *   is an empty bag: inv = 0 and nothing is added.
 * base_table [base_rows, dim] f32 (16-byte aligned) + base_ids [n_bags] int64, both NULL or both given; accumulate must be 0
 *   with them: out[b] = base_table[base_ids[b]] + pooled - the base row takes the place of the row accumulate 1 reads from
 *   out, with the same rounding sequence (pooled is scaled first, then one add), so the launch equals
 *   tt_embedding_gather_f32 into out followed by the accumulating bag launch, bit for bit.  base_ids[b] outside
 *   [0, base_rows) gives a zero base row and (unless it is -1) sets *oob_flag: tt_embedding_gather_f32's rule.  An empty
 *   bag's row is written as the base row itself.
 * With exclude and base both NULL the entry IS tt_embedding_bag_fwd_f32.  The backward launch and the table updates are
 * tt_embedding_bag_bwd_f32 and the sparse entries, unchanged.  TT_ERR_INVALID_ARG before any launch: everything the bag entry
 * rejects, a base half given, a base with accumulate 1, base_rows <= 0 or a misaligned base_table with a base.              */
int tt_history_bag_fwd_f32(const float* table, int64_t table_rows, int32_t dim,
                           const int32_t* tokens, int64_t n_token_rows, int32_t L,
                           const int64_t* bag_rows, int64_t n_bags, int32_t pooling, int32_t accumulate,
                           float* out, int64_t* batch_ids, float* inv, int32_t* oob_flag,
                           const int64_t* exclude, const float* base_table, int64_t base_rows, const int64_t* base_ids,
                           tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * History attention (added to v10: new symbols only, the version is unchanged) - the history bag pooled by a learned query
 * with a recency bias instead of a fixed scale (csrc/history_attn.hip).  attn [dim + L] f32 (16-byte aligned) = [a | p].
 * Forward, one launch.  table, tokens, bag_rows, n_bags, batch_ids, oob_flag, exclude and base_table / base_rows / base_ids are
 * tt_history_bag_fwd_f32's, rule for rule (-1 padding anywhere, out-of-range tokens skipped with the flag, leave-one-out on
 * the raw token, a -1 or out-of-range bag row or base id, empty bags); dim a multiple of 4 in 4..1024, L in 1..64.  For the
 * valid slots j of bag b, in ascending slot order:
 *   r_j = number of valid slots behind j (0: the newest kept item - counted after the exclusion, so the ranks stay contiguous)
 *   e_j = <table[token_j], a> * (1 / sqrt(dim)) + p[r_j]
 *   w   = softmax(e) over the valid slots (max-subtracted, hardware exponential);  pooled = sum_j w_j table[token_j]
 *   out[b] = base row + pooled (no base: pooled; an empty bag: the base row itself, or +0)
 * weights [n_bags, L] f32 (may be NULL): the normalised weights, exactly 0 in a skipped slot; a bag with one valid slot has
 * weight exactly 1 and pooled = that row.  pooled [n_bags, dim] f32 (may be NULL, 16-byte aligned): the pooled term without
 * the base row - what the backward launch takes G from.  A bag's bits depend on that bag alone: not on the grid, not on its
 * neighbours.  n_bags == 0 launches nothing; anything else is TT_ERR_INVALID_ARG before any launch (dim, L, n_bags * L beyond
 * 31 bits, a base half given, null or misaligned table / out / attn / pooled / base_table).
 * Backward, one launch, given dy = d out [n_bags, dim] and the forward's batch_ids, weights and pooled:
 *   G = <dy[b], pooled[b]>    t_j = <dy[b], h_j>    de_j = w_j (t_j - G)
 *   slot_grads[b * L + j, :] = w_j dy[b] + de_j a / sqrt(dim)        one gradient row PER SLOT; a skipped slot's row is untouched
 *   dattn_slabs [n_slabs][dim + L]: slab s = [sum de_j table[token_j] / sqrt(dim) | dp, dp[r_j] += de_j] over the bags
 *   [s * ceil(n_bags / n_slabs), ...) - every slab written in full (an empty one as zeros), no atomics, no pre-zeroing: the
 *   form tt_dense_seg / tt_adam_seg sum (slab_stride = dim + L).  tt_history_attention_num_slabs(n_bags) is a host query for a
 *   slab count that fills the chip (8 bags per slab, at most 1024); any n_slabs in 1..65536 is accepted.
 * The table is then updated by tt_sparse_plan over batch_ids (n_ids = n_bags * L; a skipped slot's id is -1) and
 * tt_sparse_sgd_f32 / tt_sparse_adagrad_f32 / tt_adam_step_f32 with grads = slot_grads and order = the plan's order;
 * d base_table[base_ids[b]] = dy[b].  Bit-reproducible for one (n_bags, n_slabs).                                            */
int tt_history_attention_fwd_f32(const float* table, int64_t table_rows, int32_t dim,
                                 const int32_t* tokens, int64_t n_token_rows, int32_t L,
                                 const int64_t* bag_rows, int64_t n_bags, const float* attn,
                                 float* out, int64_t* batch_ids, float* weights, float* pooled, int32_t* oob_flag,
                                 const int64_t* exclude, const float* base_table, int64_t base_rows, const int64_t* base_ids,
                                 tt_stream_t stream);
int tt_history_attention_bwd_f32(const float* table, int64_t table_rows, int32_t dim, int32_t L,
                                 const int64_t* batch_ids, const float* weights, const float* pooled, const float* dy,
                                 int64_t n_bags, const float* attn, float* slot_grads, float* dattn_slabs, int32_t n_slabs,
                                 tt_stream_t stream);
int32_t tt_history_attention_num_slabs(int64_t n_bags);

/* ---------------------------------------------------------------------------------------
 * Mixed negative sampling (added to v10: a new symbol only, the version is unchanged) - Yang et al. 2020: every step
 * appends n_neg items drawn from the whole corpus to the n_pos in-batch candidates (csrc/sample.hip).  One launch writes
 *   cand_ids[0 : n_pos]  = pos_ids
 *   cand_ids[n_pos + i]  = the draw of x = splitmix64 element (start + i) of the stream (seed, tensor_id) - the generator of
 *                          the synthetic inputs above (oracle/synth.py), the counter taken mod 2^64:
 *       bucket b = ((x >> 32) * n_items) >> 32                       (the uniform id of tt_fill_ids_i64)
 *       TT_SAMPLER_UNIFORM: id = b
 *       TT_SAMPLER_ALIAS:   u = (x & 0xFFFFFF) * 2^-24;  id = u < alias_thr[b] ? b : alias_idx[b]     (Walker's alias table:
 *                           alias_thr [n_items] f32 and alias_idx [n_items] int32, device pointers; n_items < 2^31)
 * and, only when item_freq is given (f32 [n_items], the probability of every item as an in-batch candidate),
 *   cand_prob[j] = ((float)n_pos * item_freq[id] + (float)n_neg * u_id) / (float)(n_pos + n_neg)        id = cand_ids[j]
 * for EVERY candidate, positive or sampled: the share of the step's expected candidate count that falls on the item, which
 * the scorer's cand_prob correction takes.  u_id = sampler_prob[id] (f32 [n_items], the item's probability under the
 * sampler; NULL: 1.0f / (float)n_items, the uniform sampler's).  f32, one rounding per operation, no contraction.
 * A candidate id outside [0, n_items) - a bad positive id (-1 included), a bad alias_idx entry - sets *oob_flag (device int32,
 * may be NULL), is written to cand_ids unchanged and gets cand_prob 1.0; the probability vectors are never read for it.
 * cand_prob is not touched when item_freq is NULL.  Bit-reproducible, independent of the grid.
 * TT_ERR_INVALID_ARG before any launch: n_items outside 1..2^32; n_pos or n_neg negative (or beyond 31 bits) or both 0; an
 * unknown sampler; the alias sampler without both arrays or with n_items >= 2^31; sampler_prob without item_freq; a null
 * pos_ids (n_pos > 0) / cand_ids / cand_prob (with item_freq).                                                             */
enum { TT_SAMPLER_UNIFORM = 0, TT_SAMPLER_ALIAS = 1 };
int tt_sample_candidates_i64(const int64_t* pos_ids, int64_t n_pos, int64_t n_items, int64_t n_neg, int32_t sampler,
                             const float* alias_thr, const int32_t* alias_idx, const float* item_freq,
                             const float* sampler_prob, uint64_t seed, uint64_t tensor_id, uint64_t start,
                             int64_t* cand_ids, float* cand_prob, int32_t* oob_flag, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Streaming item-frequency estimation (added to v10: a new symbol only, the version is unchanged) - Yi et al. 2019, Algorithms 2
 * and 3 (csrc/freq.hip): the sampling probability of the logQ correction from a hashed sketch of "steps since this item was last
 * a positive", updated by every batch - no offline count of the training split.
 * State: sketch, int64 [hashes, slots], zero-initialised.  A slot is ONE 64-bit word: the low 32 bits `last` (int32, the 1-based
 * step at which the slot was last hit, 0 = never), the high 32 bits the bits of `delta` (f32, the estimated gap in steps).
 * Hash: the slot of id under hash h is ((x >> 32) * slots) >> 32 with x = splitmix64 element (uint64)id of the stream
 * (seed, tensor_id + h) - the generator and the bucket rule of tt_fill_ids_i64 - so slots is any integer in 1..2^32.
 * One call, over ids int64 [n] at the 1-based `step`, behaves as if the following ran in order:
 *   1. update: every (h, slot) hit by an in-range id among ids[0 : n_update] (the step's positives) whose last != step is
 *      updated EXACTLY ONCE, however many ids or duplicates hit it:  gap = (float)(step - last);
 *      delta = last == 0 ? gap : (1 - alpha) * delta + alpha * gap;  last = step.   (f32, one rounding per operation, no
 *      contraction; 1 - alpha is formed once on the host in f32.)  A second call with the same step changes nothing.
 *   2. estimate, for EVERY j < n, after the update: d_h = last == 0 ? (float)step : delta of the id's slot under each hash,
 *      D = max over h (Algorithm 3: a collision can only shorten a gap, so the largest is the least contaminated); D >= 1.
 *   3. prob[j] = 1 / D                                                       (mix == 0), or
 *      prob[j] = (1 / D + (float)N * u_id) / (float)(B + N), B = n_update, N = n - n_update                  (mix == 1):
 *      tt_sample_candidates_i64's mixture with B * item_freq[id] replaced by the sketch's expected in-batch count 1 / D;
 *      u_id = sampler_prob[id] (f32 [n_items]; NULL: 1.0f / (float)n_items).  mix needs 1 <= n_update < n.
 * An id outside [0, n_items) updates nothing, gets prob 1.0 and sets *oob_flag (device int32, may be NULL).
 * One deviation from the paper: on a slot's FIRST sighting delta is the gap itself (step), not alpha * step - the paper's zero
 * start biases every estimate by (1 - alpha)^k, which never decays for tail items.  A property: a gap cannot be below one
 * step, so 1 / D saturates at 1 for items that occur several times per batch.
 * Launches: one over ids[0 : n_update] and, stream-ordered behind it, one over the rest (each only if non-empty).  Slots are
 * read and written with single 64-bit relaxed atomic accesses, so the result does not depend on how workgroups interleave;
 * bit-reproducible, independent of the grid.
 * TT_ERR_INVALID_ARG before any launch: hashes outside 1..4; slots or n_items outside 1..2^32; step outside 1..2^31-1; alpha
 * outside (0, 1]; n outside 0..2^31-1; n_update outside 0..n; mix not 0 / 1, or 1 without 1 <= n_update < n; sampler_prob
 * without mix; a null ids / sketch / prob.  n == 0 (with mix == 0) is a no-op that returns TT_OK.                          */
int tt_frequency_estimate_i64(const int64_t* ids, int64_t n, int64_t n_update, int64_t n_items, int64_t* sketch,
                              int32_t hashes, int64_t slots, int64_t step, float alpha, uint64_t seed, uint64_t tensor_id,
                              const float* sampler_prob, int32_t mix, float* prob, int32_t* oob_flag, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a5 — sparse optimizer on embedding rows (Keras SGD / Adagrad on IndexedSlices,
 * duplicates summed before the update; configs/data_config.yaml:63 learning_rate).
 *
 * tt_sparse_plan: stable sort of (id, position) by id.  Outputs
 *   sorted_ids [n_ids] int64 ascending, order [n_ids] int32 (positions, ascending inside equal ids).
 *   Every id outside [0, num_rows) (the padding id -1 included) is written to sorted_ids as the sentinel
 *   2^bits - 1 >= num_rows (bits = bit length of num_rows): such ids sort last, can never cut the run of a
 *   valid id, and the apply kernels skip them.
 * Only the ids are needed, so the plan can run before / beside the forward pass.  Up to
 * tt_sparse_plan_max_lds_ids() (16384) ids per table the sort is ONE launch of a hand-written LDS sort (n/128
 * workgroups per table, each sorting the ids of its own row range; tt_sparse_plan_batched sorts up to 4 tables —
 * user, item, hashed category — in that one launch) and needs no workspace; up to 16x that, 16384-id chunks are
 * radix-sorted by one launch into the workspace and a second launch merges them by rank; only longer lists fall back
 * to rocPRIM's device radix sort.
 *
 * tt_sparse_{sgd,adagrad}_f32: for every distinct id u (rows >= num_rows are skipped):
 *   g  = sum of grads[p, :] over the positions p of u in ascending p.  Order of the f32 adds: the run of u in
 *        the sorted list is cut at global multiples of 64 sorted slots; each piece is summed sequentially, then
 *        the pieces are added in order (a run inside one 64-slot block is a plain sequential sum).  The pieces
 *        of a run that crosses a block boundary are summed by different lane groups; the last one to arrive
 *        (a ticket in apply_ws) adds them in index order and applies the update — one launch in every case.
 *   apply_ws: tt_sparse_apply_workspace_bytes(n_ids, dim) bytes per table, 256-byte aligned (piece sums);
 *        ZERO it once after allocation — the kernels leave it zeroed.
 *   SGD:      w[u] = w[u] - fl(lr*g)
 *   Adagrad:  acc[u] += g*g ; w[u] -= fl(lr*g) / sqrt(acc[u] + eps)      (Keras 2.15)
 * In place.  The `2` forms update the user and the item table in one launch.
 * `order` is read only as an index into `grads`: row order[j] of grads is the gradient of sorted slot j; grads need not
 * have n_ids rows (tt_embedding_bag_bwd_f32 hands in bag indices: many slots share one gradient row).                 */
typedef struct tt_sparse_plan_args {
  const int64_t* ids;        /* [n_ids] */
  int64_t n_ids;
  int64_t num_rows;
  void* workspace;           /* tt_sparse_plan_workspace_bytes(n_ids) bytes; may be NULL when n_ids <= max_lds_ids */
  int64_t workspace_bytes;
  int64_t* sorted_ids;       /* [n_ids] out */
  int32_t* order;            /* [n_ids] out */
} tt_sparse_plan_args;
int32_t tt_sparse_plan_max_lds_ids(void);
int64_t tt_sparse_plan_workspace_bytes(int64_t n_ids);
int64_t tt_sparse_apply_workspace_bytes(int64_t n_ids, int32_t dim);
int tt_sparse_plan(const int64_t* ids, int64_t n_ids, int64_t num_rows,
                   void* workspace, int64_t workspace_bytes,
                   int64_t* sorted_ids, int32_t* order, tt_stream_t stream);
int tt_sparse_plan_batched(const tt_sparse_plan_args* tables, int32_t n_tables, tt_stream_t stream);
int tt_sparse_sgd_f32(float* table, int64_t num_rows, int32_t dim,
                      const float* grads, const int64_t* sorted_ids, const int32_t* order,
                      int64_t n_ids, float lr, void* apply_ws, tt_stream_t stream);
int tt_sparse_adagrad_f32(float* table, float* accum, int64_t num_rows, int32_t dim,
                          const float* grads, const int64_t* sorted_ids, const int32_t* order,
                          int64_t n_ids, float lr, float eps, void* apply_ws, tt_stream_t stream);
int tt_sparse_update2_f32(int32_t opt,
                          float* table_a, float* accum_a, int64_t rows_a, const float* grads_a,
                          const int64_t* sorted_ids_a, const int32_t* order_a,
                          float* table_b, float* accum_b, int64_t rows_b, const float* grads_b,
                          const int64_t* sorted_ids_b, const int32_t* order_b,
                          int32_t dim, int64_t n_ids, float lr, float eps,
                          void* apply_ws_a, void* apply_ws_b, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Row-sharded tables (multi-GPU): requester-side routing for the all-to-all exchange.
 * Row `id` lives on rank id % world at local row id / world.
 *   tt_route_by_owner_i64: stable partition of ids[n_ids] by owner into send_ids [world*cap] (local row ids,
 *     bucket o at [o*cap, (o+1)*cap), ascending position inside a bucket, padding -1) and
 *     pos_flat[p] = the slot of position p (or -1).  flags (device int32[2], may be NULL): [0] |= 1 when an id
 *     is outside [0,num_rows) (routed nowhere), [1] |= 1 when a bucket overflows `cap`.  world <= 16.
 *   tt_scatter_rows_f32: dst[idx[p], :] = src[p, :] for 0 <= idx[p] < dst_rows (per-position gradient rows
 *     into the send buffer; duplicates are summed later, on the owner, by the sparse optimizer).            */
int tt_route_by_owner_i64(const int64_t* ids, int64_t n_ids, int32_t world, int64_t num_rows, int32_t cap,
                          int64_t* send_ids, int64_t* pos_flat, int32_t* flags, tt_stream_t stream);
/* Several tables in one launch and ONE exchange: each rank keeps its shards of all tables in one combined
 * allocation (table t at rows [local_offset_t, local_offset_t + ceil(num_rows_t/world))), so the owner runs
 * one gather, one sort plan and one sparse update over every table's ids.  send_ids is
 * [world][n_tables][cap]: bucket (o, t) at ((o*n_tables + t)*cap ...), value id/world + local_offset_t,
 * padding -1; tables[t].pos_flat[p] = flat slot of position p in that buffer (or -1).  flags as above.   */
#define TT_ROUTE_MAX_TABLES 4
typedef struct {
  const int64_t* ids;       /* [n_ids] global row ids of this table            */
  int64_t num_rows;         /* global rows of this table                       */
  int64_t local_offset;     /* first row of this table in the owner's shard    */
  int64_t* pos_flat;        /* [n_ids] out                                     */
} tt_route_table;
int tt_route_tables_by_owner_i64(const tt_route_table* tables, int32_t n_tables, int64_t n_ids, int32_t world,
                                 int32_t cap, int64_t* send_ids, int32_t* flags, tt_stream_t stream);
int tt_scatter_rows_f32(const float* src, const int64_t* idx, int64_t n, int32_t dim,
                        float* dst, int64_t dst_rows, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a2 — MLP tower layers (Keras Dense; configs/data_config.yaml:56-57 *_tower_dims).
 * All matrices f32 row-major.  x [m,k], w [k,n] (Keras kernel layout), b [n], y [m,n].
 * k % 4 == 0 and n % 4 == 0; m arbitrary.  f32-input MFMA (exact f32 products).
 *
 *   fwd:  y = x@w + b ; relu != 0 applies max(.,0)
 *   bwd:  dz is dLoss/d(pre-activation) of this layer (the caller's upstream gradient,
 *         already masked by this layer's own ReLU — see dx_relu_src);
 *         dx = dz@w^T, and if dx_relu_src != NULL (the [m,k] output of the previous
 *         ReLU layer, i.e. x itself) dx is multiplied by (dx_relu_src > 0) so that it
 *         is directly the previous layer's dz;  dx may be NULL to skip it; dw_slabs AND db_slabs may
 *         both be NULL to skip the weight gradients (a caller that wants every dx before any dw, so the
 *         embedding gradients can travel while the dw GEMMs run, calls the layer twice).
 *         dw_slabs [n_slabs, k, n] and db_slabs [n_slabs, n] receive split-K partial
 *         sums of x^T@dz and colsum(dz); the dense update sums them in slab order.
 *         n_slabs = tt_dense_bwd_num_slabs(m).                                            */
int tt_dense_fwd_f32(const float* x, const float* w, const float* b, float* y,
                     int64_t m, int32_t k, int32_t n, int32_t relu, tt_stream_t stream);
/* With inverted dropout on the output (configs/data_config.yaml:58 dropout_rate): element (r, c) is dropped iff
 * the top 24 bits of the counter-based hash of (seed, tensor_id, counter_offset + r*n + c) are < round(rate*2^24);
 * kept elements are multiplied by 1/(1-rate).  Reproducible: oracle/synth.py::dropout_keep restates it.  The
 * backward pass needs no mask tensor: (y > 0) marks the kept, active units; pass dx_scale = 1/(1-rate) below. */
int tt_dense_fwd_dropout_f32(const float* x, const float* w, const float* b, float* y,
                             int64_t m, int32_t k, int32_t n, int32_t relu,
                             float drop_rate, uint64_t seed, uint64_t tensor_id, uint64_t counter_offset,
                             tt_stream_t stream);
int32_t tt_dense_bwd_num_slabs(int64_t m);
int tt_dense_bwd_f32(const float* x, const float* w, const float* dz,
                     float* dx, const float* dx_relu_src,
                     float* dw_slabs, float* db_slabs,
                     int64_t m, int32_t k, int32_t n, tt_stream_t stream);
/* Same, with dx additionally multiplied by dx_scale where dx_relu_src > 0 (dropout on the previous layer). */
int tt_dense_bwd_scaled_f32(const float* x, const float* w, const float* dz,
                            float* dx, const float* dx_relu_src, float dx_scale,
                            float* dw_slabs, float* db_slabs,
                            int64_t m, int32_t k, int32_t n, tt_stream_t stream);

/* Batched forms: the same layer of the user AND the item tower (identical shapes) in one launch each —
 * fwd: 1 launch, bwd: 1 launch (the dx tiles and the dw+db tiles of the layer side by side; 2 launches when
 * only dx or only dw is asked for) — instead of twice as many half-size launches.
 * `probs` is a HOST array of n_probs (1 or 2) entries.                                                     */
/* Embedding lookup FUSED into the layer (a1 + a2, the tower's first Dense): with a non-NULL `ids` the layer's input
 * x is never materialised — row r of x is row ids[r] of `table` [table_rows, k] (+ row ids2[r] of `table2`, the
 * hashed-category feature summed into the item tower's input; one f32 add per element), read straight into the
 * GEMM's LDS tiles by the forward pass (x @ w) and by the backward pass's dW = x^T @ dz.  Ids outside
 * [0, table_rows) give a zero row; -1 is a silent padding id, any other sets *oob_flag.  All-zero = no lookup.
 * Needs m <= 32768 (the ids of one dW split are staged in LDS).                                                  */
/* Row-range id lists (ABI v9; optional - all-zero = none).  tt_optimizer_step_ids_f32 gives every sorting workgroup one row
 * range [g*width, (g+1)*width) of a table, and each of them used to read ALL the batch's ids to find its own ~64.  The forward
 * lookup reads every id anyway: with `buckets` it also appends (id - g*width, batch position) to range g's list - one
 * returning atomic add on counts[g], one 8-byte store - and the optimizer launch of the SAME step, given the same descriptor,
 * reads only its own list (and falls back to the scan for a range whose list overflowed `cap`: counts[g] keeps counting).
 *   counts [groups][64] uint32, word 0 of each 256-byte line used (a counter per line: device-scope atomics on one line
 *          serialise): entries appended; ZERO before the first step - the optimizer launch resets every counter it reads
 *   pairs  [groups][cap] uint64: bits 0..31 local key, 32..47 batch position, 48..63 generation (entries of another
 *          generation - a forward pass whose optimizer step never ran - are ignored)
 * groups / width / cap must be the ones tt_optimizer_ids_geometry reports for the step (else the optimizer ignores the lists).
 * Lists exist for n_ids <= 16384, dim <= 128; filled by tt_tower_fwd2_batched_f32 and by tt_dense_fwd_batched_f32 (layer 0 with a
 * lookup).  One descriptor per table; tt_id_buckets_workspace_bytes() bytes hold one.                                          */
typedef struct tt_id_buckets {
  uint32_t* counts; uint64_t* pairs;
  int32_t groups; uint32_t width; int32_t cap; uint32_t gen;
} tt_id_buckets;
typedef struct tt_dense_lookup {
  const float* table;  const int64_t* ids;  int64_t table_rows;
  const float* table2; const int64_t* ids2; int64_t table2_rows;     /* optional */
  int32_t* oob_flag;                                                 /* optional */
  tt_id_buckets buckets;                                             /* optional: row-range lists of `ids` (forward pass only) */
} tt_dense_lookup;
/* ReLU sign bits (optional, n % 32 == 0): the forward pass can write, beside y, one bit per element — word
 * [row][col / 32] of a [m, n/32] uint32 array, bit col % 32 = (y[row][col] > 0) — and the backward pass of the NEXT layer
 * takes them as its dx mask (`dx_relu_bits`, [m, k/32]) instead of re-reading the whole activation through
 * `dx_relu_src`: 1/32 of the mask bytes (cfg3: 0.5 MB instead of 16.8 MB per step) and no 4-byte strided loads in
 * front of the dx tiles.  Same mask, same results bit for bit.                                                       */
typedef struct tt_dense_fwd_args {
  const float* x; const float* w; const float* b; float* y;
  uint64_t dropout_tensor_id;       /* counter stream of this problem's dropout mask (ignored at rate 0) */
  tt_dense_lookup lookup;           /* x may be NULL when lookup.ids is given */
  uint32_t* relu_bits;              /* optional [m, n/32]: sign bits of y (after ReLU / dropout), see above */
} tt_dense_fwd_args;
typedef struct tt_dense_bwd_args {
  const float* x; const float* w; const float* dz; float* dx; const float* dx_relu_src;
  float* dw_slabs; float* db_slabs;
  tt_dense_lookup lookup;           /* x may be NULL when lookup.ids is given (dW reads the table rows) */
  const uint32_t* dx_relu_bits;     /* optional [m, k/32]: the dx mask as sign bits; takes precedence over dx_relu_src */
} tt_dense_bwd_args;
int tt_dense_fwd_batched_f32(const tt_dense_fwd_args* probs, int32_t n_probs, int64_t m, int32_t k, int32_t n,
                             int32_t relu, float drop_rate, uint64_t seed, uint64_t counter_offset,
                             tt_stream_t stream);
int tt_dense_bwd_batched_f32(const tt_dense_bwd_args* probs, int32_t n_probs, float dx_scale,
                             int64_t m, int32_t k, int32_t n, tt_stream_t stream);

/* The forward pass of a TWO-layer tower in ONE launch (csrc/tower.hip): h = relu(x @ w0 + b0) [dropout], y = h @ w1 + b1 for
 * the user and the item tower together.  A workgroup owns 32 batch rows for both layers; the hidden tile stays in LDS (it
 * is still written to layer0[i].y - and its sign bits to layer0[i].relu_bits - because the backward pass reads them).
 * layer0[i] / layer1[i] are the per-layer descriptions tt_dense_fwd_batched_f32 takes (layer1[i].x must be layer0[i].y or
 * NULL; only layer 0 may carry a lookup); dropout applies to the hidden layer, with layer0[i].dropout_tensor_id and
 * counter_offset as there.  Bit-identical to the two tt_dense_fwd_batched_f32 calls.  Shapes: k0 % 32 == 0, k0 <= 512,
 * h and n1 in {128, 256} (tt_tower_fwd2_supported; otherwise TT_ERR_UNSUPPORTED - call the layers one by one).         */
int32_t tt_tower_fwd2_supported(int64_t m, int32_t k0, int32_t h, int32_t n1);
int tt_tower_fwd2_batched_f32(const tt_dense_fwd_args* layer0, const tt_dense_fwd_args* layer1, int32_t n_probs, int64_t m,
                              int32_t k0, int32_t h, int32_t n1, float drop_rate, uint64_t seed, uint64_t counter_offset,
                              tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * L2-normalised tower outputs (cosine scoring): tf.math.l2_normalize between a tower's last Dense layer and the scorer,
 * and its backward pass between the scorer's dq / dc and the tower's backward (csrc/normalize.hip).  Per row of x [rows, dim],
 * with s = sum x^2 (eps clamps the SUM OF SQUARES; TensorFlow's default is 1e-12):
 *   forward   y  = x * (1 / sqrt(max(s, eps)))                     (correctly rounded division and square root)
 *   backward  t  = sum x * dy;   s >= eps:  inv = 1 / sqrt(s),  dx = inv * (dy - x * (t * inv * inv))
 *                                s <  eps:  dx = dy * (1 / sqrt(eps))            (y = x / sqrt(eps) is linear there)
 * The backward pass takes x and dy and recomputes s and t from the registers it has just loaded: no saved norm, no extra
 * buffer, the same traffic (x, dy in; dx out) as a form that saves y.  dx MAY ALIAS dy: every lane reads the elements it
 * owns before it writes them and touches no others; x must not alias either output, y must not alias x.
 * Up to two problems (both towers) of one shape per launch; `probs` is a HOST array.  n_probs in 1..2; rows >= 0 (0: no
 * launch, TT_OK); dim % 4 == 0, 4 <= dim <= 1024; eps > 0; all pointers non-NULL and 16-byte aligned.  A group of lanes
 * sized to the row (8 lanes at dim 32 ... a whole wave from dim 256 on) reduces it with a fixed-order butterfly: no LDS,
 * no atomics, results bit-reproducible and independent of n_probs and of the grid.  HBM-bound: 8 * rows * dim bytes
 * per problem forward, 12 * rows * dim backward.                                                                       */
typedef struct tt_l2norm_fwd_args { const float* x; float* y; } tt_l2norm_fwd_args;
typedef struct tt_l2norm_bwd_args { const float* x; const float* dy; float* dx; } tt_l2norm_bwd_args;
int tt_l2_normalize_fwd_f32(const tt_l2norm_fwd_args* probs, int32_t n_probs, int64_t rows, int32_t dim, float eps,
                            tt_stream_t stream);
int tt_l2_normalize_bwd_f32(const tt_l2norm_bwd_args* probs, int32_t n_probs, int64_t rows, int32_t dim, float eps,
                            tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Dense numeric side features (added to v10: new symbols and structs only, the version is unchanged; csrc/features.hip) - the
 * Normalization -> concat -> Dense branch of a TFRS query / candidate model.  A fixed [feat_rows, F] f32 matrix per tower
 * (1 <= F <= 32); the row of the pair's id is normalised (Keras Normalization, with an optional clip), projected by a trained
 * [F, dim] kernel and written to / added into the tower's input rows:
 *   z_f      = clamp((x_f - mean_f) * inv_std_f, -clip, clip)          (no clamp when clip == 0; z_f = x_f with mean == NULL)
 *   acc_d    = 0;  for f = 0 .. F-1 ascending:  acc_d = acc_d + z_f * proj[f, d]
 *   out[b,d] = accumulate ? out[b, d] + acc_d : acc_d
 * every subtraction, product and sum a separate correctly rounded f32 operation in exactly this order (no fma): a NumPy f32
 * restatement gives the same bits.  ids[b] == -1: the row contributes z = 0 (z_out row zero) and sets no flag; any other id
 * outside [0, feat_rows) does the same and sets *oob_flag (may be NULL).  z_out [n, F] (may be NULL) keeps the normalised
 * values for the backward pass.  Up to two problems (both towers) per launch, every one with its own n and F; `probs` is a
 * HOST array.  TT_ERR_INVALID_ARG before any launch: n_probs outside 1..2, dim not a multiple of 4 in 4..1024, clip < 0,
 * F outside 1..32, mean / inv_std given one without the other, a NULL feat / proj / out (ids with n > 0), proj / out not
 * 16-byte aligned.  n == 0 in every problem: no launch, TT_OK.
 * The features themselves are not trained; the projection's gradient is the backward entry:
 *   dp_slabs[s, f, d] = sum of z[b, f] * dy[b, d] over the rows b of slab s = [s * R, min((s + 1) * R, n)), R = ceil(n / n_slabs)
 * Every slab is written in full - one without rows as zeros - so the caller never pre-zeroes: the [n_slabs][F * dim] form
 * tt_dense_seg / tt_adam_seg sum (slab_stride = F * dim).  tt_dense_features_num_slabs(n) is a host query for a slab count
 * that keeps the launch parallel (128-row slabs, at most 64); any n_slabs in 1..65535 is accepted.  No atomics: bits depend
 * on (n, n_slabs, dim) alone.  dy [n, dim] 16-byte aligned.                                                              */
typedef struct tt_dense_features_fwd_args {
  const float* feat;         /* [feat_rows, F]                                         */
  int64_t feat_rows;
  int32_t F;
  int32_t accumulate;        /* 0: out = product; 1: out += product                   */
  const int64_t* ids;        /* [n]                                                    */
  int64_t n;
  const float* mean;         /* [F] or NULL (then inv_std is NULL too)                 */
  const float* inv_std;      /* [F] or NULL                                            */
  const float* proj;         /* [F, dim]                                               */
  float* out;                /* [n, dim]                                               */
  float* z_out;              /* [n, F] or NULL                                         */
} tt_dense_features_fwd_args;
typedef struct tt_dense_features_bwd_args {
  const float* z;            /* [n, F]: z_out of the forward launch                    */
  const float* dy;           /* [n, dim]: gradient w.r.t. the tower's input rows       */
  int64_t n;
  int32_t F;
  int32_t n_slabs;
  float* dp_slabs;           /* [n_slabs, F, dim]                                      */
} tt_dense_features_bwd_args;
int tt_dense_features_fwd_f32(const tt_dense_features_fwd_args* probs, int32_t n_probs, int32_t dim, float clip,
                              int32_t* oob_flag, tt_stream_t stream);
int tt_dense_features_bwd_f32(const tt_dense_features_bwd_args* probs, int32_t n_probs, int32_t dim, tt_stream_t stream);
int32_t tt_dense_features_num_slabs(int64_t n);

/* ---------------------------------------------------------------------------------------
 * Rating-prediction head (added to v10: new symbols only, the version is unchanged; csrc/rating.hip) - the tfrs.tasks.Ranking
 * side of a joint retrieval + ranking model: one hidden ReLU layer over the pair's two tower outputs and a scalar output.
 * D = the scorer dim (32, 64, 128 or 256), H = the hidden width (a multiple of 32 in 32..256), n pairs:
 *   a[b,j]  = b1[j] + sum_i q[b,i] W1[i,j] + sum_i c[b,i] W1[D+i,j]      W1 [2D, H] row-major, b1 [H]
 *   h[b,j]  = max(a[b,j], 0)                                             h [n, H] is kept for the backward launch
 *   pred[b] = b2[0] + sum_j h[b,j] w2[j]                                 w2 [H], b2 [1]
 * One launch, no labels (train step, validation and serving share it): exact f32 products on the f32-input MFMA, the A
 * operand read straight from q and c (no [n, 2D] concat buffer), W1 streamed from global memory; a workgroup owns 32 rows
 * and neither reads nor writes past row n.
 * Backward, one launch, for the MSE loss L = (1/n) sum_valid w_b e_b^2 scaled by the caller (grad_scale = 2 rating_weight / n):
 *   e_b = pred[b] - rating[b];  valid_b = isfinite(rating[b]) (NaN: a missing label);  w_b = sample_weight[b] (NULL: 1)
 *   g_b = valid_b ? grad_scale w_b e_b : 0;      dh[b,j] = g_b w2[j] (h[b,j] > 0)     (built on the fly: never in HBM)
 *   dq[b,:] (+)= sum_j dh[b,j] W1[0:D, j];       dc[b,:] (+)= sum_j dh[b,j] W1[D:2D, j]   (accumulate: 1 adds, 0 overwrites)
 *   kslabs [n_slabs][2D H + H]:  dW1[i,j] = sum_b x[b,i] dh[b,j] (x = [q ; c], row-major), then dw2[j] = sum_b g_b h[b,j]
 *   bslabs [n_slabs][H + 1]:     db1[j] = sum_b dh[b,j], then db2 = sum_b g_b
 *   se_slabs [n_slabs]:          sum of w_b e_b^2 over the slab's valid rows (the caller forms the loss from these)
 * Slab s owns the rows [s * R, min((s + 1) * R, n)), R = ceil(n / n_slabs); every slab is written in full - one without rows
 * as zeros - so nothing is pre-zeroed: the form tt_dense_seg / tt_adam_seg sum (slab_stride = 2D H + H and H + 1).  Every row
 * of dq / dc is touched by exactly one workgroup per 32-column block; no atomics: bits depend on (n, n_slabs, D, H) alone.
 * An arbitrary upstream gradient g is expressed as pred = g, rating = 0, sample_weight = NULL, grad_scale = 1 (h is read
 * separately).  tt_rating_head_num_slabs(n) is a host query for a slab count that keeps the launch parallel (128-row slabs,
 * at most 64; the launch has n_slabs * 2D / 32 workgroups).
 * TT_ERR_INVALID_ARG before any launch: D not in {32, 64, 128, 256}, H not a multiple of 32 in 32..256, n < 0, n_slabs outside
 * 1..65535, and with n > 0 a NULL pointer (sample_weight excepted) or q / c / h / W1 / w2 / dq / dc not 16-byte aligned.
 * n == 0: no launch, TT_OK.                                                                                              */
int tt_rating_head_fwd_f32(const float* q, const float* c, int64_t n, int32_t D, int32_t H, const float* w1,
                           const float* b1, const float* w2, const float* b2, float* pred, float* h, tt_stream_t stream);
int tt_rating_head_bwd_f32(const float* q, const float* c, const float* h, const float* pred, const float* rating,
                           const float* sample_weight, float grad_scale, int64_t n, int32_t D, int32_t H,
                           const float* w1, const float* w2, float* dq, float* dc, int32_t accumulate,
                           float* kslabs, float* bslabs, float* se_slabs, int32_t n_slabs, tt_stream_t stream);
int32_t tt_rating_head_num_slabs(int64_t n);

/* ---------------------------------------------------------------------------------------
 * DCN-v2 cross layer (added to v10: new symbols and structs only, the version is unchanged; csrc/cross.hip) - tfrs.layers.dcn.Cross
 * (Wang et al. 2021) between a tower's summed input rows x0 and its Dense stack.  D = the embedding dim (a multiple of 32 in
 * 32..256), n rows, W [D, D] row-major as Keras stores a kernel ([in, out]), b [D]:
 *   u[r,j] = b[j] + sum_i x[r,i] W[i,j]                                  exact f32 products on the f32-input MFMA
 *   y[r,j] = x0[r,j] * u[r,j] + x[r,j]                                   product and sum two separately rounded f32 operations
 * One forward launch covers up to two problems (both towers), every one with its own n; `probs` is a HOST array.  A workgroup
 * owns 32 rows and neither reads nor writes past row n.  u_out (may be NULL: inference) keeps u for the backward launch.  x may
 * be x0 (layer 0).  y and u_out must not alias x, x0 or each other (pointer-equal aliases are refused).
 * Backward, ONE launch for up to two problems, for the upstream gradient g = dL/dy, with t = g * x0:
 *   x_is_x0 == 0 (upper layers):  dx = g + t W^T;   dx0 = accumulate_dx0 ? dx0 + g * u : g * u
 *   x_is_x0 == 1 (layer 0, x == x0):  dx = ((g + t W^T) + g * u) [+ dx0 when dx0 != NULL: read only]
 *   dw_slabs[s * slab_stride + i * D + j] = sum of x[r,i] t[r,j],   db_slabs[s * slab_stride + j] = sum of t[r,j]
 * over the rows r of slab s = [s * R, min((s + 1) * R, n)), R = ceil(n / n_slabs).  Every slab is written in full - one without
 * rows as zeros - so nothing is pre-zeroed; dw_slabs and db_slabs are the addresses of slab 0 and share slab_stride, so all
 * layers and both towers can write into one [n_slabs][slab_stride] array that tt_dense_seg / tt_adam_seg sum.  A problem with
 * n == 0 beside one with rows still writes its (zero) slabs.  No atomics: bits depend on (n, n_slabs, D) alone.
 * The launch holds the dW tiles and the dx tiles side by side: the dW tiles read g, x0 and x while dx is written, so dx MUST NOT
 * alias g, x0, x or u, and dx0 none of those nor dx (pointer-equal aliases are refused).
 * tt_cross_num_slabs(n) is a host query for a slab count that keeps the launch parallel (128-row slabs, at most 64; the launch
 * has n_slabs * D / 32 + ceil(n / 32) workgroups per problem); any n_slabs in 1..65535 is accepted.
 * TT_ERR_INVALID_ARG before any launch: n_probs outside 1..2, D not a multiple of 32 in 32..256, n < 0, n_slabs outside
 * 1..65535, slab_stride < D * D with more than one slab, and with n > 0 a NULL pointer (u_out; dx0 with x_is_x0 excepted), a
 * pointer that is not 16-byte aligned, x_is_x0 with x != x0, or one of the aliases above.  n == 0 in every problem: no launch,
 * TT_OK.                                                                                                                    */
typedef struct tt_cross_fwd_args {
  const float* x0;           /* [n, D]: the summed input rows                          */
  const float* x;            /* [n, D]: x_l (== x0 at layer 0)                         */
  const float* w;            /* [D, D]                                                 */
  const float* b;            /* [D]                                                    */
  float* u_out;              /* [n, D] or NULL                                         */
  float* y;                  /* [n, D]: x_{l+1}                                        */
  int64_t n;
} tt_cross_fwd_args;
typedef struct tt_cross_bwd_args {
  const float* x0;           /* [n, D]                                                 */
  const float* x;            /* [n, D]: x_l (== x0 with x_is_x0)                       */
  const float* u;            /* [n, D]: u_out of the forward launch                    */
  const float* w;            /* [D, D]                                                 */
  const float* g;            /* [n, D]: gradient w.r.t. y                              */
  float* dx;                 /* [n, D]: gradient w.r.t. x (x_is_x0: w.r.t. x0, whole)  */
  float* dx0;                /* [n, D]: written / accumulated; x_is_x0: read only, may be NULL */
  float* dw_slabs;           /* slab s: D * D floats at dw_slabs + s * slab_stride     */
  float* db_slabs;           /* slab s: D floats at db_slabs + s * slab_stride         */
  int64_t n;
  int64_t slab_stride;
  int32_t n_slabs;
  int32_t x_is_x0;
  int32_t accumulate_dx0;    /* x_is_x0 == 0 only                                      */
} tt_cross_bwd_args;
int tt_cross_fwd_f32(const tt_cross_fwd_args* probs, int32_t n_probs, int32_t D, tt_stream_t stream);
int tt_cross_bwd_f32(const tt_cross_bwd_args* probs, int32_t n_probs, int32_t D, tt_stream_t stream);
int32_t tt_cross_num_slabs(int64_t n);

/* ---------------------------------------------------------------------------------------
 * Layer normalisation of the tower hidden layers (added to v10: new symbols and structs only, the version is unchanged;
 * csrc/layernorm.hip) - Keras LayerNormalization between a hidden Dense layer (run without activation) and its ReLU.  Per row
 * of z [rows, dim], with gamma and beta [dim]:
 *   mu = mean(z)   var = mean((z - mu)^2)   r = 1 / sqrt(var + eps)   xhat = (z - mu) * r        (biased variance, two-pass)
 *   y  = dropout(relu(xhat * gamma + beta))         product and sum rounded separately; division and square root correctly rounded
 * relu != 0 applies the ReLU; drop_rate > 0 applies inverted dropout with the stream of tt_dense_fwd_batched_f32: key
 * (seed, dropout_tensor_id), element (r, c) at counter_offset + r * dim + c, dropped iff the top 24 bits of its hash are below
 * round(drop_rate * 2^24), kept entries times 1 / (1 - drop_rate).  relu_bits (optional) receives the sign bits of y in the
 * format tt_dense_fwd_args.relu_bits documents ([rows, dim/32] words, bit c % 32 of word [r][c / 32] = (y[r][c] > 0)).
 * Backward, for dn = dL/d(xhat * gamma + beta) - what the dx epilogue of the layer above writes when it masks by the sign bits:
 *   g = dn * gamma   dz = r * ((g - mean(g)) - xhat * mean(g * xhat))
 *   dgamma_slabs[s * slab_stride + c] = sum of dn[r,c] * xhat[r,c],   dbeta_slabs[s * slab_stride + c] = sum of dn[r,c]
 * over the rows r of slab s = [s * R, min((s + 1) * R, rows)), R = ceil(rows / n_slabs).  mu and r are recomputed from z: no
 * saved statistics.  Every slab is written in full - one without rows as zeros - and only its dim floats behind each of the two
 * addresses; dgamma_slabs and dbeta_slabs are the addresses of slab 0 and share slab_stride, so all layers and both towers can
 * write into one [n_slabs][slab_stride] array that one tt_dense_seg / tt_adam_seg sums.  A problem with rows == 0 beside one
 * with rows still writes its (zero) slabs.  dz MAY ALIAS dn: every lane reads the elements it owns before it writes them and
 * touches no others.  y must not alias z, dz must not alias z (pointer-equal aliases are refused).
 * Up to two problems (both towers) per launch, every one with its own rows; `probs` is a HOST array.  A group of lanes sized
 * to the row (8 lanes at dim 32 ... a whole wave from dim 256 on) holds it in registers and reduces it with a fixed-order
 * butterfly: no atomics; row r of y and of dz depends on row r alone and is bit-identical across runs, n_probs, the grid and
 * the number of rows; the slabs' bits depend on (rows, n_slabs, dim) alone.  The backward launch has one workgroup per slab and
 * problem: tt_layer_norm_num_slabs(rows) is a host query for a count that keeps it parallel (32-row slabs, at most 256); any
 * n_slabs in 1..65535 is accepted.  HBM-bound: 8 * rows * dim bytes per problem forward, 12 * rows * dim backward.
 * TT_ERR_INVALID_ARG before any launch: n_probs outside 1..2, dim not a multiple of 32 in 32..1024, eps <= 0, drop_rate outside
 * [0, 1), rows < 0, n_slabs outside 1..65535, slab_stride < 2 * dim with more than one slab, and for a problem with rows a NULL
 * pointer (relu_bits excepted), a pointer that is not 16-byte aligned (the slabs need 4) or one of the aliases above.  rows == 0
 * in every problem: no launch, TT_OK.                                                                                        */
typedef struct tt_layer_norm_fwd_args {
  const float* z;            /* [rows, dim]: the Dense layer's pre-activation          */
  const float* gamma;        /* [dim]                                                  */
  const float* beta;         /* [dim]                                                  */
  float* y;                  /* [rows, dim]                                            */
  uint32_t* relu_bits;       /* [rows, dim/32] or NULL                                 */
  uint64_t dropout_tensor_id;/* counter stream of this problem's dropout mask (ignored at rate 0) */
  int64_t rows;
} tt_layer_norm_fwd_args;
typedef struct tt_layer_norm_bwd_args {
  const float* z;            /* [rows, dim]                                            */
  const float* gamma;        /* [dim]                                                  */
  const float* dn;           /* [rows, dim]                                            */
  float* dz;                 /* [rows, dim]; may be dn                                 */
  float* dgamma_slabs;       /* slab s: dim floats at dgamma_slabs + s * slab_stride   */
  float* dbeta_slabs;        /* slab s: dim floats at dbeta_slabs + s * slab_stride    */
  int64_t rows;
} tt_layer_norm_bwd_args;
int tt_layer_norm_fwd_f32(const tt_layer_norm_fwd_args* probs, int32_t n_probs, int32_t dim, float eps, int32_t relu,
                          float drop_rate, uint64_t seed, uint64_t counter_offset, tt_stream_t stream);
int tt_layer_norm_bwd_f32(const tt_layer_norm_bwd_args* probs, int32_t n_probs, int32_t dim, float eps, int32_t n_slabs,
                          int64_t slab_stride, tt_stream_t stream);
int32_t tt_layer_norm_num_slabs(int64_t rows);

/* Dense parameter update over up to TT_MAX_DENSE_SEGS segments in one launch.
 *   g = sum_s grad_slabs[s*slab_stride + i] (s ascending) + 2*l2*w[i]
 *   SGD: w -= fl(lr*g);  Adagrad: acc += g*g; w -= fl(lr*g)/sqrt(acc+eps)
 * If grad_out != NULL the summed gradient (WITHOUT the l2 term) is written there and,
 * when apply == 0, nothing else happens (the multi-GPU path all-reduces grad_out and
 * calls again with n_slabs = 1).  `segs` is a HOST array.                                 */
#define TT_MAX_DENSE_SEGS 16
typedef struct tt_dense_seg {
  float* param;              /* [count]                                   */
  float* accum;              /* [count] Adagrad accumulator or NULL (SGD) */
  const float* grad_slabs;   /* [n_slabs][slab_stride]                    */
  float* grad_out;           /* [count] or NULL                           */
  int64_t count;
  int64_t slab_stride;
  int32_t n_slabs;
  float l2;                  /* l2_regularization (configs/data_config.yaml:59); 0 for biases */
} tt_dense_seg;
int tt_dense_update_f32(const tt_dense_seg* segs, int32_t n_segs, int32_t opt, int32_t apply,
                        float lr, float eps, tt_stream_t stream);
/* ---------------------------------------------------------------------------------------
 * Global-norm gradient clipping (added to v10: new symbols and one struct only, the version is unchanged; csrc/clip.hip) -
 * tf.clip_by_global_norm over ALL gradient buffers of a step in two launches, whatever their number:
 *   sumsq = sum over dense buffers, over e in [0, count), of (sum_s data[s * slab_stride + e])^2    (slabs added in f32, s ascending)
 *         + sum over row buffers, over rows r, of f_r * |data[r, :]|^2
 *   norm  = sqrtf(sumsq)    scale = clip_norm / fmaxf(norm, clip_norm)   (IEEE division; exactly 1 when norm <= clip_norm; NaN
 *   when norm is not finite)    every buffer *= scale in place: all n_slabs slabs of a dense buffer ([0, count) of each, never
 *   the padding up to slab_stride), every row of a row buffer (also those with f_r == 0).
 * The factor of row r is f_r = weight + w(mode): TT_CLIP_ROWS 0; the bag modes count n_r = the entries >= 0 of slot_ids[r, 0..L)
 * and add n_r (TT_CLIP_BAG_SUM), 1 / n_r (TT_CLIP_BAG_MEAN) or 1 (TT_CLIP_BAG_SQRTN), 0 for an empty bag - the squared norm of
 * the per-occurrence gradient rows of a pooled embedding bag whose pooled-row gradient is data[r]; TT_CLIP_SLOT_MASK adds 1
 * where slot_ids[r] >= 0 (one id per row).  `weight` counts the tables that consume the row as it stands (an input gradient
 * shared by k id tables: k).  A row with f_r == 0 is not read by the norm: it may hold anything, also non-finite values.
 * Launch 1 writes one f32 partial per workgroup into `workspace` (wave shuffles, then LDS; no atomics); in launch 2 every
 * workgroup adds the partials in one fixed order (in f64), workgroup 0 writes stats[0] = norm and stats[1] = scale, and all of
 * them scale (nothing is read or stored when scale == 1).  Both grids depend on the buffers' shapes alone: equal inputs give
 * equal bits.  Nothing is read back to the host.  16-byte loads where data is 16-byte aligned and slab_stride % 4 == 0, scalar
 * loads for a dense buffer's last count % 4 elements and for unaligned dense buffers.  `bufs` is a HOST array of up to
 * TT_CLIP_MAX_BUFFERS entries, passed to the kernels by value.  No buffers, or only empty ones: no launch, stats = {0, 1}.
 * tt_clip_workspace_bytes: a host query (>= 256, a multiple of 256; -1 for an invalid list) - the workspace needs no
 * initialisation.  HBM: reads every gradient byte once, and once more with a write where scale != 1.
 * TT_ERR_INVALID_ARG before any launch: a NULL bufs / stats / workspace, n_bufs outside 0..TT_CLIP_MAX_BUFFERS, clip_norm <= 0 or
 * not finite, an unknown mode, n_slabs < 1, count / rows < 0, slab_stride < count with more than one slab, dim < 4 or
 * dim % 4 != 0, L < 1 in a bag mode, and for a buffer with elements a NULL data, a NULL slot_ids where the mode reads them, a
 * row buffer that is not 16-byte aligned or a dense one that is not 4-byte aligned.  TT_ERR_WORKSPACE: workspace_bytes too small. */
#define TT_CLIP_MAX_BUFFERS (8 + TT_MAX_DENSE_SEGS)
enum { TT_CLIP_DENSE = 0, TT_CLIP_ROWS = 1, TT_CLIP_BAG_SUM = 2, TT_CLIP_BAG_MEAN = 3, TT_CLIP_BAG_SQRTN = 4, TT_CLIP_SLOT_MASK = 5 };
typedef struct tt_clip_buffer {
  float* data;               /* dense: slab s at data + s * slab_stride; rows: [rows, dim]          */
  const int64_t* slot_ids;   /* bag modes: [rows, L]; TT_CLIP_SLOT_MASK: [rows]; else ignored       */
  int64_t rows;              /* row buffers                                                         */
  int64_t count;             /* dense: floats per slab                                              */
  int64_t slab_stride;       /* dense: floats between two slabs                                     */
  int32_t dim;               /* row buffers: a multiple of 4                                        */
  int32_t L;                 /* bag modes: slots per row                                            */
  int32_t n_slabs;           /* dense: >= 1                                                         */
  int32_t mode;              /* TT_CLIP_*                                                           */
  float weight;              /* row buffers: the constant part of f_r (>= 0)                        */
  int32_t reserved;
} tt_clip_buffer;
int64_t tt_clip_workspace_bytes(const tt_clip_buffer* bufs, int32_t n_bufs);
int tt_clip_global_norm_f32(const tt_clip_buffer* bufs, int32_t n_bufs, float clip_norm, void* workspace, int64_t workspace_bytes,
                            float* stats, tt_stream_t stream);

/* tt_dense_bwd_batched_f32 with a dense parameter update RIDING in the same launch (ABI v9): `segs` (apply = 1 semantics of
 * tt_dense_update_f32) must belong to ANOTHER layer - in a backward pass, the layer above, whose gradient slabs the previous
 * backward launch completed; a segment whose slabs this launch writes or whose weights it reads is refused.  The update's
 * blocks are the first workgroups of the dx+dw launch: no launch of their own, and their slab traffic (cfg3: 9 of the step's
 * 18 MB) leaves the optimizer launch, whose HBM burst is the embedding rows'.  Same arithmetic, bit for bit.  With dx or dw
 * alone (two launches anyway) the update runs as its own launch behind them.                                            */
int tt_dense_bwd_batched_update_f32(const tt_dense_bwd_args* probs, int32_t n_probs, float dx_scale, int64_t m, int32_t k, int32_t n,
                                    const tt_dense_seg* segs, int32_t n_segs, int32_t opt, float lr, float eps, tt_stream_t stream);

/* Two layers' backward passes in ONE launch (r04): `upper` = layer l (k1 -> n), `lower` = layer l-1 (k0 -> k1), upper[i].dx
 * must BE lower[i].dz.  The same tiles as two tt_dense_bwd_batched_f32 calls, results identical bit for bit; the lower layer's
 * tiles wait, inside the launch, for the 64-row blocks of dz they read (agent-scope release / acquire on a counter per row
 * block in `workspace`: tt_tower_bwd2_workspace_bytes(m) bytes, 256-byte aligned, ZEROED ONCE - the launch leaves it zeroed).
 * What it saves is the boundary between the two launches (the platform's ~4 us + one launch's tail + the other's ramp).  The
 * wait is bounded: if it ever ran out, int32 word [4 * (m / 64)] of the workspace is set and the results of that step are wrong.
 * Both layers need dx and dw_slabs; only the lower layer may carry the fused lookup.  tt_tower_bwd2_supported: m % 64 == 0
 * and the batch splits of the dW GEMMs (tt_dense_bwd_num_slabs) whole numbers of 64-row blocks.                         */
int32_t tt_tower_bwd2_supported(int64_t m, int32_t k0, int32_t k1, int32_t n);
int64_t tt_tower_bwd2_workspace_bytes(int64_t m);
int tt_tower_bwd2_batched_f32(const tt_dense_bwd_args* upper, const tt_dense_bwd_args* lower, int32_t n_probs, float dx_scale_upper,
                              float dx_scale_lower, int64_t m, int32_t k0, int32_t k1, int32_t n, void* workspace, tt_stream_t stream);

/* The whole optimizer of a train step in ONE launch: the fused sparse update of up to 3 embedding tables (user, item,
 * hashed category; same dim and n_ids, each with its own sort plan and apply workspace) AND the dense update of every
 * tower segment (apply = 1 semantics of tt_dense_update_f32).  Same arithmetic, bit for bit, as tt_sparse_update2_f32 /
 * tt_sparse_{sgd,adagrad}_f32 followed by tt_dense_update_f32; the two halves are independent and memory-bound, so one
 * launch overlaps them and saves a launch boundary.  `tables` and `segs` are HOST arrays.                          */
typedef struct tt_sparse_table {
  float* table; float* accum;            /* [rows, dim]; accum NULL for SGD        */
  int64_t rows;
  const float* grads;                    /* [n_ids, dim] per-position gradient rows */
  const int64_t* sorted_ids; const int32_t* order;   /* tt_sparse_plan outputs      */
  void* apply_ws;                        /* tt_sparse_apply_workspace_bytes(n_ids, dim), zeroed once */
} tt_sparse_table;
int tt_optimizer_step_f32(int32_t opt, const tt_sparse_table* tables, int32_t n_tables, int32_t dim, int64_t n_ids,
                          const tt_dense_seg* segs, int32_t n_segs, float lr, float eps, tt_stream_t stream);

/* The same step from the RAW ids (n_ids <= tt_optimizer_ids_max_ids() = 65536, else TT_ERR_UNSUPPORTED): no
 * tt_sparse_plan launch and no sorted ids in HBM — the sorting workgroups of each table (one per row range) apply the
 * update to their own rows inside the one optimizer launch.  Same results, bit for bit, as tt_sparse_plan_batched +
 * tt_optimizer_step_f32 (same piece boundaries at global multiples of 64 sorted slots).  Lists of more than
 * tt_sparse_plan_max_lds_ids() (16384) ids take the long-list kernel (r04: ids scanned in chunks, the LDS list keeps
 * 16384 slots; a row range that holds more ids than that - a degenerate batch - is sorted in a global scratch inside
 * apply_ws, which tt_sparse_apply_workspace_bytes sizes for it).                                                   */
int32_t tt_optimizer_ids_max_ids(void);
typedef struct tt_sparse_table_ids {
  float* table; float* accum;            /* [rows, dim]; accum NULL for SGD        */
  int64_t rows;
  const float* grads;                    /* [n_ids, dim] per-position gradient rows */
  const int64_t* ids;                    /* [n_ids] the batch's ids, unsorted       */
  void* apply_ws;                        /* tt_sparse_apply_workspace_bytes(n_ids, dim) */
  tt_id_buckets buckets;                 /* optional (ABI v9): the row-range lists this step's forward lookup filled */
} tt_sparse_table_ids;
/* The row ranges tt_optimizer_step_ids_f32 will use for these tables (HOST outputs, [n_tables] each): table t is cut into
 * groups[t] ranges of width[t] rows; *cap = entries per list (0: this shape takes no lists - dim > 128 or n_ids > 16384).   */
int tt_optimizer_ids_geometry(const int64_t* table_rows, int32_t n_tables, int32_t dim, int64_t n_ids,
                              const tt_dense_seg* segs, int32_t n_segs, int32_t* groups, uint32_t* width, int32_t* cap);
int64_t tt_id_buckets_workspace_bytes(void);      /* one table's counts + pairs, 256-byte aligned inside */
/* A trainer's skew probe (r04): out_max[t] (DEVICE, [n_tables]) = the largest number of this batch's ids that fall into ONE
 * of table t's row ranges (the ranges of tt_optimizer_ids_geometry).  The one-launch optimizer gives a range to one
 * workgroup: ids uniform over the rows put n_ids / groups in each, a vocabulary in order of frequency puts thousands into
 * the first (cfg3, ids ~ rows * u^4: launch 12 -> 169 us).  Run every few dozen steps, copy the words to pinned host memory
 * without waiting, and take tt_sparse_plan_batched + tt_optimizer_step_f32 while a range holds more than ~384 ids.
 * ids: HOST array of n_tables device pointers.  One launch, one workgroup per table.                                    */
int tt_id_range_load(const int64_t* const* ids, const int64_t* table_rows, int32_t n_tables, int32_t dim, int64_t n_ids,
                     const tt_dense_seg* segs, int32_t n_segs, int32_t* out_max, tt_stream_t stream);
int tt_optimizer_step_ids_f32(int32_t opt, const tt_sparse_table_ids* tables, int32_t n_tables, int32_t dim, int64_t n_ids,
                              const tt_dense_seg* segs, int32_t n_segs, float lr, float eps, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Lazy Adam (added to v10: new symbols only, the version is unchanged) - TF-Addons LazyAdam / torch.optim.SparseAdam with
 * Keras Adam's defaults (configs/data_config.yaml:63 learning_rate 0.001 is Keras Adam's step size): the sparse update of up
 * to 3 embedding tables AND the dense update of every tower segment in one call (csrc/adam.hip).  Only the rows of this
 * batch's ids are touched - every other row keeps w, m and v bit for bit; ids outside [0, rows) (the padding id -1
 * included) are skipped; the bias correction comes from the 1-based global step.
 * Arithmetic (f32, one rounding per operation, no contraction).  The library computes on the HOST, in f64, each rounded once
 * to f32:  omb1 = 1 - beta1,  omb2 = 1 - beta2,  alpha_t = lr * sqrt(1 - beta2^step) / (1 - beta1^step)   (lr, beta1, beta2
 * widened from the f32 values of tt_adam_hyper).  For every distinct id u of a table (every element of a segment):
 *   m' = m + (g - m) * omb1;    v' = v + (g*g - v) * omb2;    w' = w - (alpha_t * m') / (sqrt(v') + eps)
 * evaluated in exactly that order.  Sparse g: the sum of the gradient rows of u in the order of tt_sparse_{sgd,adagrad}_f32
 * (runs cut at global multiples of 64 sorted slots, pieces sequential, pieces added in index order): bit-identical to the g SGD
 * and Adagrad see.  Dense g = slab 0 + slab 1 + ... (ascending, starting AT slab 0), then + (2*l2)*w, as tt_dense_update_f32.
 * Consumes tt_sparse_plan / tt_sparse_plan_batched outputs (every table: the same dim and n_ids).  As for the sparse entries, row
 * order[j] of grads is the gradient of sorted slot j; grads need not have n_ids rows.  `tables`, `segs` and `h`
 * are HOST data.  n_tables in 0..3 (0: dense only), n_segs in 0..TT_MAX_DENSE_SEGS (0: sparse only); n_ids == 0 with
 * n_segs == 0 is a no-op.  dim % 4 == 0; step >= 1; beta1, beta2 in [0, 1); eps > 0; m and v non-NULL; table, m, v, grads
 * 16-byte aligned: anything else is TT_ERR_INVALID_ARG before any launch.
 * Two stream-ordered launches and no communication inside either (no tickets, no wait between workgroups): the first sums
 * every piece and updates the runs that lie inside one 64-slot block; the second finishes the runs that cross a block boundary
 * from the piece sums the first stored in `workspace` and carries the dense segments as extra workgroups.
 * workspace: tt_adam_workspace_bytes(n_ids, dim) bytes PER TABLE (0 for n_ids == 0), 256-byte aligned; needs NO
 * initialisation (the second launch reads only what the first wrote in the same call).                              */
typedef struct tt_adam_table {
  float* table; float* m; float* v;      /* [rows, dim] parameters, first and second moment */
  int64_t rows;
  const float* grads;                    /* [n_ids, dim] per-position gradient rows */
  const int64_t* sorted_ids; const int32_t* order;   /* tt_sparse_plan outputs      */
  void* workspace;                       /* tt_adam_workspace_bytes(n_ids, dim)     */
} tt_adam_table;
typedef struct tt_adam_seg {
  float* param; float* m; float* v;      /* [count]                                 */
  const float* grad_slabs;               /* [n_slabs][slab_stride]                  */
  int64_t count;
  int64_t slab_stride;
  int32_t n_slabs;
  float l2;                              /* l2_regularization; 0 for biases         */
} tt_adam_seg;
typedef struct tt_adam_hyper {
  float lr, beta1, beta2, eps;           /* Keras defaults: 0.001, 0.9, 0.999, 1e-7 */
  int64_t step;                          /* 1-based global step                     */
} tt_adam_hyper;
int64_t tt_adam_workspace_bytes(int64_t n_ids, int32_t dim);
int tt_adam_step_f32(const tt_adam_table* tables, int32_t n_tables, int32_t dim, int64_t n_ids,
                     const tt_adam_seg* segs, int32_t n_segs, const tt_adam_hyper* h, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Row-wise Adagrad (added to v10: new symbols and one struct only, the version is unchanged; csrc/rowwise.hip) - the "exact
 * row-wise" Adagrad of FBGEMM / TorchRec for embedding tables, with THIS project's epsilon placement: ONE accumulator float per
 * table row, fed with the mean of the row's squared gradient.  The sparse update of up to 3 embedding tables AND the
 * element-wise Adagrad update of every dense segment in one call.  Only the rows of this batch's ids are read or written - every
 * other row keeps w AND its accumulator bit for bit; ids outside [0, rows) (the plan's sentinel and the padding id -1 included)
 * are skipped.
 * Arithmetic (f32, one rounding per operation, no contraction: __fadd_rn, __fmul_rn, __fdiv_rn, sqrtf).  For every distinct
 * valid id u of a table:
 *   g      = the sum of the gradient rows of u in the order of tt_sparse_{sgd,adagrad}_f32 (runs cut at global multiples of 64
 *            sorted slots, pieces sequential, pieces added in index order): bit-identical to the g SGD, Adagrad and Adam see
 *   q_j    = g_j * g_j
 *   S      = sum_j q_j                       in the fixed order below
 *   s      = S * inv_dim                     inv_dim = 1.0f / (float)dim, formed once on the host
 *   a'[u]  = a[u] + s                        a: [rows] f32 (the caller initialises it, e.g. to Keras's 0.1)
 *   w'[u]  = w[u] - (lr * g) / sqrt(a'[u] + eps)          eps INSIDE the root, as tt_sparse_adagrad_f32 (Keras), not
 *                                                         FBGEMM's sqrt(a) + eps
 * Order of S - a function of dim alone, the same in both launches: a lane group of lpr = min(32, dim/4 rounded up to a power
 * of two) lanes owns the row; lane l holds the float4 chunks c = l, l + lpr, ... (< dim/4); it forms p_l by adding its q values
 * one after the other, chunks in ascending c, elements in ascending order inside a chunk, the sum starting AT its first value;
 * a lane with no chunk (dim = 96: 32 lanes, 24 chunks) has p_l = +0; then the group runs a butterfly p_l = p_l + p_{l xor off}
 * for off = 1, 2, 4, ... < lpr, after which every lane holds the same bits: S.  (All terms are >= 0, so an idle lane's +0 is
 * exact.)  tests/rowwise_check.py restates exactly this in NumPy f32.
 * Dense segments: the existing element-wise Adagrad of tt_dense_update_f32 (opt = TT_OPT_ADAGRAD, apply = 1; `accum` non-NULL;
 * grad_out, when given, receives the summed gradient as there): bit-identical to it.
 * Consumes tt_sparse_plan / tt_sparse_plan_batched outputs (every table: the same dim and n_ids).  Row order[j] of grads is the
 * gradient of sorted slot j; grads need not have n_ids rows.  `tables` and `segs` are HOST data.  n_tables in 0..3 (0: dense
 * only), n_segs in 0..TT_MAX_DENSE_SEGS (0: sparse only); n_ids == 0 with n_segs == 0 is a no-op.  Null pointers, dim % 4 != 0,
 * rows <= 0, eps <= 0, a non-finite lr, a table or grads not 16-byte aligned, a workspace not 256-byte aligned:
 * TT_ERR_INVALID_ARG before any launch.  dim > 512 (more than 4 float4 chunks per lane): TT_ERR_UNSUPPORTED before any launch.
 * Two stream-ordered launches and no communication inside either (no tickets, no wait between workgroups, no atomics): the
 * first sums every piece and reduces and updates the runs that lie inside one 64-slot block; the second finishes the runs that
 * cross a block boundary from the piece sums the first stored in `workspace` and carries the dense segments as extra workgroups.
 * workspace: tt_rowwise_adagrad_workspace_bytes(n_ids, dim) bytes PER TABLE (0 for n_ids == 0), 256-byte aligned; needs NO
 * initialisation (the second launch reads only what the first wrote in the same call).                              */
typedef struct tt_rowwise_table {
  float* table;                          /* [rows, dim] parameters                  */
  float* row_accum;                      /* [rows] one accumulator per row          */
  int64_t rows;
  const float* grads;                    /* per-position gradient rows; row order[j] belongs to sorted slot j */
  const int64_t* sorted_ids; const int32_t* order;   /* tt_sparse_plan outputs      */
  void* workspace;                       /* tt_rowwise_adagrad_workspace_bytes(n_ids, dim) */
} tt_rowwise_table;
int64_t tt_rowwise_adagrad_workspace_bytes(int64_t n_ids, int32_t dim);
int tt_rowwise_adagrad_step_f32(const tt_rowwise_table* tables, int32_t n_tables, int32_t dim, int64_t n_ids,
                                const tt_dense_seg* segs, int32_t n_segs, float lr, float eps, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * The WHOLE train step as one call (ABI v8): what `train-model` (pyproject.toml:67, src/training/train.py - declared,
 * never written) would run per batch.  A HOST struct of pointers describes the step once - every buffer is caller-owned
 * and fixed from step to step; per step the caller only rewrites the id pointers, the dropout row counter and the optional
 * per-pair inputs - and tt_train_step_f32 enqueues, on `stream`, exactly the launches the separate entry points would:
 *   for each layer l:            tt_dense_fwd_batched_f32(fwd[l], 2, ...)       (layer 0 reads the embedding rows itself;
 *                                two-layer towers of supported shapes: ONE tt_tower_fwd2_batched_f32 launch instead)
 *   scorer + loss + dq, dc:      tt_retrieval_fwd_bwd_f32 / _bf16x3_f32         (q, c = fwd[n_layers-1][*].y; dq, dc = bwd[n_layers-1][*].dz)
 *   for each layer l, last first: tt_dense_bwd_batched_f32(bwd[l], 2, ...)
 *   optimizer:                   tt_optimizer_step_ids_f32(tables, segs)       (sort + duplicate sums + sparse update + dense update)
 * Eight launches for two 2-layer towers of a fused shape (nine otherwise); no other work, no allocation, no synchronisation.
 * It exists for the HOST side: a caller that reaches the library through an FFI (ctypes: ~7 us per call) pays that once per
 * step instead of once per launch - cfg1 (B 256) is 7 launches of a few us each.  Results are identical to the separate
 * calls, bit for bit.
 * Both towers must have the same layer shapes (the batched launches); batch <= 65536 (tt_optimizer_step_ids_f32) and
 * <= 32768 with a fused lookup.                                                                                       */
#define TT_MAX_TOWER_LAYERS 8
typedef struct tt_train_step {
  int64_t batch;                                   /* pairs per step = rows of every activation                    */
  int32_t n_layers;                                /* Dense layers per tower                                       */
  int32_t dims[TT_MAX_TOWER_LAYERS + 1];           /* embedding_dim, then the width of every layer                 */
  tt_dense_fwd_args fwd[TT_MAX_TOWER_LAYERS][2];   /* [layer][0 = user tower, 1 = item tower]; hidden layers: ReLU */
  tt_dense_bwd_args bwd[TT_MAX_TOWER_LAYERS][2];
  float dropout_rate;                              /* configs/data_config.yaml:58; 0 = none                        */
  uint64_t dropout_seed;
  uint64_t dropout_row0;                           /* first global batch row of this step: layer l's counter offset = row0 * dims[l+1] */
  int32_t scorer_precision;                        /* 0 = exact f32 products, 1 = bf16x3                           */
  float inv_temperature;                           /* 1 / retrieval.temperature (configs/data_config.yaml:70)      */
  const float* sample_weight;                      /* [batch] or NULL                                              */
  const float* cand_prob;                          /* [batch] or NULL (candidate_sampling_probability)             */
  const int64_t* cand_ids;                         /* [batch] or NULL (remove_accidental_hits)                     */
  void* retrieval_ws; int64_t retrieval_ws_bytes;  /* tt_retrieval_workspace_bytes(batch, batch, dims[n_layers])   */
  float* lse; float* per_row; float* loss;         /* [batch], [batch], [1]                                        */
  int32_t opt;                                     /* TT_OPT_SGD / TT_OPT_ADAGRAD                                  */
  int32_t n_tables;                                /* 2, or 3 with the hashed category table                       */
  tt_sparse_table_ids tables[3];
  int32_t n_segs;
  tt_dense_seg segs[TT_MAX_DENSE_SEGS];
  float lr, eps;
  void* id_bucket_ws;                              /* optional (ABI v9): n_tables * tt_id_buckets_workspace_bytes() bytes, 256-byte   */
  int64_t id_bucket_ws_bytes;                      /* aligned, ZEROED once: the forward lookup hands the optimizer launch its row-range id lists */
} tt_train_step;
int tt_train_step_f32(const tt_train_step* step, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * a3 + a4 — batched dot-product scorer fused with the in-batch sampled-softmax loss
 * (tfrs.tasks.Retrieval.call: matmul(q, c^T) / temperature, optional sampling-probability
 * correction and accidental-hit removal, CategoricalCrossentropy(from_logits=True,
 * reduction=SUM); configs/data_config.yaml:69-70).  Softmax probabilities never reach HBM (see tt_retrieval_fwd_bwd_f32 for the
 * raw dot products the exact-f32 training entry keeps between its passes).
 *
 *   s_ij   = <q_i, c_j> * inv_temperature  - log(clip(cand_prob_j, 1e-6, 1))
 *            (+ -inf where cand_ids_j == cand_ids_{i+diag_offset} and j != i+diag_offset)
 *   lse_i  = log sum_j exp(s_ij)
 *   row_i  = w_i * (lse_i - s_{i,i+diag_offset}) ;  loss = sum_i row_i
 *   dq     = grad_scale * sum_j  w_i/T (softmax_ij - [j == i+diag_offset]) c_j ;  dc likewise.
 *
 * q [nq,dim], c [nc,dim] f32 row-major; dim in {32,64,128,256}; nq + diag_offset <= nc.
 * sample_weight [nq], cand_prob [nc], cand_ids [nc] (int64) may each be NULL.
 * hard_thr [nq] (may be NULL): per-query thresholds from tt_retrieval_hard_negative_thresholds_f32 — only the
 * positive and the negatives scoring at or above the threshold take part (tfrs num_hard_negatives).
 * Outputs: lse [nq], per_row [nq], loss [1]; dq [nq,dim], dc [nc,dim].
 * Workspace: tt_retrieval_workspace_bytes(nq, nc, dim) bytes, 256-byte aligned.  For the fused training entries this
 * INCLUDES the raw dot products of pass 1, ceil(nq/32) * ceil(nc/32) blocks of 4 KB = 4*nq*nc bytes (268 MB at 8192 x
 * 8192, 4.3 GB at 32768 x 32768; ABI v5 and later - a workspace sized by an older library is refused with
 * TT_ERR_WORKSPACE).  Both precisions keep them, at every dim (ABI v8; bf16x3 at dim 256 recomputed through v7).    */
int64_t tt_retrieval_workspace_bytes(int64_t nq, int64_t nc, int32_t dim);
/* Host query: the number of slices a scorer pass cuts its streamed side into for this shape (pass 0: stationary q - loss + dq,
 * forward, rank; 1: stationary c - dc with the products recomputed; 2: dc from the stored products).  r04: chosen by a model of
 * the launch (rounds of resident workgroups) instead of "double until 512 workgroups" - batch 8200 ran 0.879 ms against 0.558
 * for 8192 because 8 of 520 workgroups ran a second round alone; every power-of-two shape keeps its r03 value.               */
int32_t tt_retrieval_num_splits(int64_t nq, int64_t nc, int32_t dim, int32_t pass);
/* the part of it the forward-only (tt_retrieval_fwd_f32) and separate-backward (tt_retrieval_bwd_f32) entries need: no
 * [nq][nc] logit buffer (only the fused training entries keep the raw dot products between their two passes) */
int64_t tt_retrieval_fwd_workspace_bytes(int64_t nq, int64_t nc, int32_t dim);
/* What tt_retrieval_rank_f32 alone needs (no gradient slabs: those make the full workspace as large as the candidate
 * corpus once nc >= 65536).                                                                                   */
int64_t tt_retrieval_rank_workspace_bytes(int64_t nq, int64_t nc, int32_t dim);
int tt_retrieval_fwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                         int64_t diag_offset, float inv_temperature,
                         const float* sample_weight, const float* cand_prob, const int64_t* cand_ids,
                         const float* hard_thr,
                         void* workspace, int64_t workspace_bytes,
                         float* lse, float* per_row, float* loss, tt_stream_t stream);
int tt_retrieval_bwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                         int64_t diag_offset, float inv_temperature,
                         const float* sample_weight, const float* cand_prob, const int64_t* cand_ids,
                         const float* hard_thr, const float* lse, float grad_scale,
                         void* workspace, int64_t workspace_bytes,
                         float* dq, float* dc, tt_stream_t stream);

/* tfrs.tasks.Retrieval(num_hard_negatives=k) / tfrs.layers.loss.HardNegativeMining: thr[i] separates the k
 * highest-scoring negatives of query i (after temperature, sampling-probability correction and accidental-hit
 * removal) from the rest (midpoint between the k-th and the next lower logit; ties at the k-th value are all kept;
 * fewer than k negatives: everything is kept).  scratch: nq*nc floats (a logit row block, materialised).             */
int tt_retrieval_hard_negative_thresholds_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                              int64_t diag_offset, float inv_temperature,
                                              const float* cand_prob, const int64_t* cand_ids,
                                              int32_t num_hard_negatives,
                                              void* workspace, int64_t workspace_bytes,
                                              float* scratch, int64_t scratch_bytes,
                                              float* thr, tt_stream_t stream);

/* Fused training form: loss AND both gradients in two passes over the logits instead of three
 * (pass 1: online softmax with the candidate-weighted sum -> lse, per_row, loss, dq;  pass 2: dc).
 * Same semantics and outputs as tt_retrieval_fwd_f32 followed by tt_retrieval_bwd_f32.
 * Both entries keep the raw dot products [nq][nc] (f32) in the workspace between the passes — pass 2 reads them
 * back instead of recomputing them (half its matrix-pipe work; 6*nq*nc*dim executed FLOPs in total instead of 8) —
 * which is why tt_retrieval_workspace_bytes includes 4*nq*nc bytes; tt_retrieval_fwd_workspace_bytes is enough for the
 * forward-only and separate-backward entries.                                                                        */
int tt_retrieval_fwd_bwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                             int64_t diag_offset, float inv_temperature,
                             const float* sample_weight, const float* cand_prob, const int64_t* cand_ids,
                             const float* hard_thr, float grad_scale, void* workspace, int64_t workspace_bytes,
                             float* lse, float* per_row, float* loss, float* dq, float* dc,
                             tt_stream_t stream);

/* The same fused training form with every matrix product on the bf16 matrix cores through a three-way split of the
 * f32 operands (x = hi + mid + lo, each bf16, residuals exact): "bf16x3", an f32-EMULATED precision — 6 bf16 products
 * per logit term (error ~2^-24 relative), 3 per gradient term (~2^-16), f32 accumulation, f32 softmax; inputs and
 * outputs stay f32 and the results meet the same 1e-4 bars as the exact-f32 form (tests/test_gpu_parity.py).  2.7x
 * fewer matrix-pipe cycles than v_mfma_f32_32x32x2_f32.  dim must be 128 or 256 (else TT_ERR_UNSUPPORTED: use the f32 form). */
int tt_retrieval_fwd_bwd_bf16x3_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                    int64_t diag_offset, float inv_temperature,
                                    const float* sample_weight, const float* cand_prob, const int64_t* cand_ids,
                                    const float* hard_thr, float grad_scale, void* workspace, int64_t workspace_bytes,
                                    float* lse, float* per_row, float* loss, float* dq, float* dc,
                                    tt_stream_t stream);
/* The forward-only (validation) pass and the metric (rank) pass in the same f32-emulated precision: both are pure GEMM1, so
 * the 6-product bf16 split (2^-24 relative on every logit) is the whole kernel.  Arguments as tt_retrieval_fwd_f32 /
 * tt_retrieval_rank_f32; dim in {128, 256}.                                                                          */
int tt_retrieval_fwd_bf16x3_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                int64_t diag_offset, float inv_temperature, const float* sample_weight,
                                const float* cand_prob, const int64_t* cand_ids, const float* hard_thr,
                                void* workspace, int64_t workspace_bytes, float* lse, float* per_row, float* loss,
                                tt_stream_t stream);
int tt_retrieval_rank_bf16x3_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                 float inv_temperature, const float* cand_prob, const int64_t* pos_index,
                                 void* workspace, int64_t workspace_bytes, int32_t* rank, tt_stream_t stream);

/* Retrieval metrics (configs/data_config.yaml:71 top_k_eval; tfrs.metrics.FactorizedTopK's role):
 * rank[i] = number of candidates j != pos_index[i] with s_ij > s_{i,pos_index[i]} over ALL nc candidates
 * (nc may be the whole item corpus; nq <= or > nc both allowed).  Recall@K = mean(rank < K),
 * NDCG@K = mean([rank < K] / log2(rank + 2)).  Workspace: tt_retrieval_rank_workspace_bytes(nq, nc, dim).     */
int tt_retrieval_rank_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                          float inv_temperature, const float* cand_prob, const int64_t* pos_index,
                          void* workspace, int64_t workspace_bytes, int32_t* rank, tt_stream_t stream);
/* The same metric pass on the IN-BATCH candidates - tfrs.tasks.Retrieval(batch_metrics=[top-k categorical accuracy]):
 * rank[i] = number of candidates j != i + diag_offset whose logit (after temperature, -log clip(cand_prob) and, with
 * cand_ids, accidental-hit removal: the scores the loss sees) is strictly above the positive's; top-k accuracy =
 * mean(rank < k).  Workspace: tt_retrieval_rank_workspace_bytes(nq, nc, dim).                                        */
int tt_retrieval_batch_rank_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim, int64_t diag_offset,
                                float inv_temperature, const float* cand_prob, const int64_t* cand_ids,
                                void* workspace, int64_t workspace_bytes, int32_t* rank, tt_stream_t stream);

/* Pairwise retrieval losses over the in-batch negatives (added to v10: new symbols only, the version is unchanged): BPR /
 * pairwise logistic (Rendle 2009) and the pairwise hinge (triplet) loss, on the logits the softmax above sees.
 *
 *   s_ij  = <q_i, c_j> * inv_temperature - log(clip(cand_prob_j, 1e-6, 1))          (cand_prob NULL: no correction)
 *   pos_i = s_{i, i+diag_offset}
 *   N_i   = { j != i+diag_offset :  not (cand_ids given and cand_ids_j == cand_ids_{i+diag_offset})
 *                                   and not (hard_thr given and s_ij below hard_thr_i) } ;   n_i = |N_i|
 *   x_ij  = pos_i - s_ij
 *   phi   = TT_PAIRWISE_LOGISTIC: softplus(-x) = max(-x, 0) + log1p(exp(-|x|))       phi' = -sigmoid(-x)
 *           TT_PAIRWISE_HINGE:    max(0, margin - x)                                 phi' = -[x < margin]   (x == margin: 0)
 *   r_i   = 1 / max(n_i, 1)  (TT_PAIRWISE_MEAN)   or   1  (TT_PAIRWISE_SUM)
 *   row_i = w_i * r_i * sum_{j in N_i} phi(x_ij) ;   loss = sum_i row_i              (w = sample_weight, NULL: 1)
 *   h_ij  = -w_i * r_i * phi'(x_ij) for j in N_i, else 0 ;   H_i = sum_j h_ij
 *   dq_i  = grad_scale * inv_temperature * (sum_j h_ij c_j - H_i c_{i+diag_offset})
 *   dc_j  = grad_scale * inv_temperature * (sum_i h_ij q_i - [j == i'+diag_offset] H_i' q_i')
 *
 * A row without negatives (n_i = 0) has row_i = 0 and no gradient.  hard_thr is what
 * tt_retrieval_hard_negative_thresholds_f32 returns (the comparison is the scorer's, on its log2-domain logits).  margin is
 * read by the hinge only but must be finite.  Arguments and limits as tt_retrieval_fwd_f32 / tt_retrieval_fwd_bwd_f32 (there
 * is no lse); exact f32 products only.  Two passes over the logits (stationary q, then stationary c, which recomputes the
 * products: 8*nq*nc*dim executed FLOPs), no atomics - the results are bit-identical run to run - and no [nq, nc] array:
 * the workspace (256-byte aligned, tt_retrieval_pairwise_workspace_bytes; 0 for a degenerate shape) holds row terms,
 * per-split row partials and the gradient slabs, and is never larger than tt_retrieval_workspace_bytes plus the row terms. */
#define TT_PAIRWISE_LOGISTIC 0
#define TT_PAIRWISE_HINGE 1
#define TT_PAIRWISE_MEAN 0
#define TT_PAIRWISE_SUM 1
int64_t tt_retrieval_pairwise_workspace_bytes(int64_t nq, int64_t nc, int32_t dim);
int tt_retrieval_pairwise_fwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                  int64_t diag_offset, float inv_temperature,
                                  const float* sample_weight, const float* cand_prob, const int64_t* cand_ids,
                                  const float* hard_thr, void* workspace, int64_t workspace_bytes,
                                  float* per_row, float* loss, int32_t kind, float margin, int32_t reduction,
                                  tt_stream_t stream);
int tt_retrieval_pairwise_fwd_bwd_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim,
                                      int64_t diag_offset, float inv_temperature,
                                      const float* sample_weight, const float* cand_prob, const int64_t* cand_ids,
                                      const float* hard_thr, float grad_scale, void* workspace, int64_t workspace_bytes,
                                      float* per_row, float* loss, float* dq, float* dc,
                                      int32_t kind, float margin, int32_t reduction, tt_stream_t stream);

/* Exact top-K retrieval (tfrs.layers.factorized_top_k.BruteForce; ABI v10): the k best candidates of every query,
 * scored and selected in one pass over the corpus (no [nq x nc] score matrix) and merged across corpus splits.
 * score[i][j] = q_i . c_j (plain dot product, exact f32 products on the f32 MFMA).  q [nq, dim], c [nc, dim] f32, 16-byte
 * aligned; nq >= 1, 1 <= nc < 2^31, dim in {32, 64, 128, 256}, 1 <= k <= TT_TOPK_MAX_K, k <= nc.
 * out_scores f32 [nq, k], out_idx int64 [nq, k]: score descending, equal scores by ascending candidate index (also at the
 * cut at position k): the answer is unique, and a query's row is bit-identical whatever the batch it is sent in.
 * Exclusions (optional; both NULL or both set): CSR excl_offsets int64 [nq + 1] (non-decreasing, within excl_idx),
 * excl_idx int64 sorted ascending within each query's segment; duplicates and values outside [0, nc) match nothing.
 * Excluded candidates never enter the result; when fewer than k candidates remain the tail is (-inf, -1).
 * Workspace (256-byte aligned): tt_retrieval_topk_workspace_bytes(nq, nc, dim, k) (0 for arguments the call refuses). */
#define TT_TOPK_MAX_K 256
int64_t tt_retrieval_topk_workspace_bytes(int64_t nq, int64_t nc, int32_t dim, int32_t k);
int tt_retrieval_topk_f32(const float* q, const float* c, int64_t nq, int64_t nc, int32_t dim, int32_t k,
                          const int64_t* excl_offsets, const int64_t* excl_idx, void* workspace, int64_t workspace_bytes,
                          float* out_scores, int64_t* out_idx, tt_stream_t stream);

/* IVF approximate top-K retrieval (added to v10: new symbols only, the version is unchanged): tt_retrieval_topk_f32's
 * contract restricted to the items of the nprobe inverted lists whose centroids score highest for the query (the
 * lists tt_retrieval_topk_f32(q, centroids, nlist, dim, nprobe) returns).  Index: centroids f32 [nlist, dim]; list_offsets int64 [nlist + 1] (0, non-decreasing, ending at n);
 * list_vectors f32 [n, dim], the items reordered so that list l is rows list_offsets[l] .. list_offsets[l + 1]; list_ids
 * int32 [n], the original item id of every reordered row, distinct.  q, centroids, list_vectors 16-byte aligned.
 * out_scores f32 [nq, k], out_idx int64 [nq, k] (ORIGINAL ids): score descending, equal scores by ascending original id
 * (also at the cut); a pair's score is bit-identical to tt_retrieval_topk_f32's; with nprobe = nlist the result equals
 * tt_retrieval_topk_f32 over the whole corpus.  Exclusions as tt_retrieval_topk_f32, holding original ids; fewer than k
 * candidates in the probed lists: the tail is (-inf, -1).  Limits: dim in {32, 64, 128, 256}, 1 <= k <= TT_TOPK_MAX_K,
 * 1 <= nprobe <= min(nlist, TT_TOPK_MAX_K), 1 <= n < 2^31.  Launches only (no synchronisation, no copy to the host).
 * Workspace (256-byte aligned): tt_ivf_search_workspace_bytes(...) (0 for arguments the call refuses). */
int64_t tt_ivf_search_workspace_bytes(int64_t nq, int64_t nlist, int64_t n, int32_t dim, int32_t k, int32_t nprobe);
int tt_ivf_search_f32(const float* q, int64_t nq, const float* centroids, int64_t nlist, const int64_t* list_offsets,
                      const float* list_vectors, const int32_t* list_ids, int64_t n, int32_t dim, int32_t k, int32_t nprobe,
                      const int64_t* excl_offsets, const int64_t* excl_idx, void* workspace, int64_t workspace_bytes,
                      float* out_scores, int64_t* out_idx, tt_stream_t stream);

/* Int8-quantised top-K retrieval with an exact f32 re-rank (added to v10: new symbols only, the version is unchanged).
 * tt_quantize_rows_i8: per row of x f32 [n, dim], amax = max|x|, scale = amax / 127.0f (one IEEE f32 division),
 * code = clamp(rintf(x / scale), -127, 127) (half to even); a row with amax == 0 gets scale 0 and all-zero codes.
 * codes int8 [n, dim], scales f32 [n]; x and codes 16-byte aligned; dim in {32, 64, 128, 256}.  Inputs must be finite.
 *
 * tt_retrieval_topk_i8_f32, stage 1 (scan): the query rows are quantised with the same formula (qc, qscale);
 * iscore[i][j] = sum_d qc[i][d] * codes[j][d] in int32 (exact in f32); key = float(iscore) * scales[j] (one f32
 * multiply); the k1 candidates of a query are its best by (key descending, index ascending), also at the cut.  Excluded
 * ids (CSR as tt_retrieval_topk_f32) never take a candidate slot.
 * Stage 2 (finish): with c f32 [nc, dim], every candidate gets the f32 score tt_retrieval_topk_f32 gives that pair, bit
 * for bit, and the best k by (score descending, index ascending) are written.  With c == NULL there is no re-rank, k1 == k
 * is required, and the output is the stage-1 order with scores key * qscale_i.  Fewer than k candidates left: the tail is
 * (-inf, -1).  A query's row is bit-identical alone or in any batch.
 * Limits: dim in {32, 64, 128, 256}, 1 <= k <= k1 <= min(TT_TOPK_MAX_K, nc), nc < 2^31; q, codes and c 16-byte aligned.
 * Launches only (no synchronisation, no copy to the host).  Every refusal is TT_ERR_INVALID_ARG before any launch.
 * Workspace (256-byte aligned): tt_retrieval_topk_i8_workspace_bytes(...) (0 for arguments the call refuses). */
int tt_quantize_rows_i8(const float* x, int64_t n, int32_t dim, int8_t* codes, float* scales, tt_stream_t stream);
int64_t tt_retrieval_topk_i8_workspace_bytes(int64_t nq, int64_t nc, int32_t dim, int32_t k, int32_t k1);
int tt_retrieval_topk_i8_f32(const float* q, const int8_t* codes, const float* scales, const float* c, int64_t nq, int64_t nc,
                             int32_t dim, int32_t k, int32_t k1, const int64_t* excl_offsets, const int64_t* excl_idx,
                             void* workspace, int64_t workspace_bytes, float* out_scores, int64_t* out_idx,
                             tt_stream_t stream);

/* Int8 IVF (added to v10: new symbols only, the version is unchanged): tt_retrieval_topk_i8_f32 restricted to the rows of
 * the nprobe inverted lists tt_ivf_search_f32 probes.  Index: centroids, list_offsets and list_ids exactly as
 * tt_ivf_search_f32; list_codes int8 [n, dim] and list_scales f32 [n], the tt_quantize_rows_i8 output of the items in list
 * order; c (nullable) the f32 corpus [n, dim] in ORIGINAL id order (the row of original id i is c + i * dim: the re-rank
 * gathers by the ids stage 1 produced).
 * Probes: the lists tt_retrieval_topk_f32(q, centroids, nprobe) returns (f32 scores; centroids are not quantised).
 * Stage 1: the query is quantised by tt_quantize_rows_i8's formula; key = float(int32 dot) * list_scales[row] (one f32
 * multiply); a candidate's id is list_ids[row]; the k1 candidates are the best by (key descending, original id ascending),
 * also at the cut; excluded original ids (CSR as tt_retrieval_topk_f32) never take a slot.
 * Stage 2: with c, every candidate gets tt_retrieval_topk_f32's score of that pair, bit for bit, and the best k by (score
 * descending, id ascending) are written; with c == NULL, k1 == k is required and the output is the stage-1 order with
 * scores key * qscale.  Fewer than k candidates left: the tail is (-inf, -1).
 * Hence: with nprobe == nlist the output equals tt_retrieval_topk_i8_f32 over the whole corpus (codes, scales and c in
 * original order), bit for bit; with fewer probes it equals that call over the union of the probed lists gathered in
 * ascending original id; a query's row is identical alone, in any batch and on any run.
 * Limits: dim in {32, 64, 128, 256}, 1 <= k <= k1 <= min(TT_TOPK_MAX_K, n), 1 <= nprobe <= min(nlist, TT_TOPK_MAX_K),
 * n < 2^31, nq * nprobe <= 2^31 - 1; q, centroids, list_codes and c 16-byte aligned, the others to their element size.
 * Every refusal is TT_ERR_INVALID_ARG before any launch, except a short workspace: TT_ERR_WORKSPACE, as tt_ivf_search_f32.
 * Launches only (no synchronisation, no copy to the host).  All row offsets are 64-bit (n * dim may exceed 2^31 bytes).
 * Workspace (256-byte aligned): tt_ivf_search_i8_workspace_bytes(...) (0 for arguments the call refuses). */
int64_t tt_ivf_search_i8_workspace_bytes(int64_t nq, int64_t nlist, int64_t n, int32_t dim, int32_t k, int32_t k1,
                                         int32_t nprobe);
int tt_ivf_search_i8_f32(const float* q, int64_t nq, const float* centroids, int64_t nlist, const int64_t* list_offsets,
                         const int8_t* list_codes, const float* list_scales, const int32_t* list_ids, const float* c, int64_t n,
                         int32_t dim, int32_t k, int32_t k1, int32_t nprobe, const int64_t* excl_offsets,
                         const int64_t* excl_idx, void* workspace, int64_t workspace_bytes, float* out_scores, int64_t* out_idx,
                         tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Time-of-interaction context (added to v10: new symbols only, the version is unchanged; csrc/time_context.hip).
 * timestamps int64 [n]: whole seconds since the Unix epoch, UTC; INT64_MIN = no timestamp.  field_mask: bit 0 hour (24 rows),
 * bit 1 day of week (7), bit 2 month (12), bit 3 period (buckets rows, 1..4096; buckets must be 0 without bit 3).  The F enabled
 * fields, in that order, own consecutive row blocks of ONE table [R, dim] f32, R = the sum of their row counts (table_rows must
 * equal it).  Row of a pair within a field's block - integer arithmetic, floor division, so negative timestamps work:
 *   days = floor(t / 86400);  hour = (t - 86400 days) / 3600;  day of week = (days + 3) mod 7 (Monday 0; 1970-01-01: Thursday)
 *   month - 1 by civil-from-days: z = days + 719468, era = floor(z / 146097), doe = z - 146097 era,
 *     yoe = (doe - doe/1460 + doe/36524 - doe/146096) / 365, doy = doe - (365 yoe + yoe/4 - yoe/100), mp = (5 doy + 2) / 153,
 *     month = mp < 10 ? mp + 3 : mp - 9
 *   period = floor(clamp(t - time_min, 0, span) * buckets / (span + 1)), span = time_max - time_min (0 <= span < 2^40)
 * Forward, one launch:  s = ((row_0 + row_1) + row_2) + row_3 over the enabled fields in order (a pair without a timestamp:
 * s = +0, its indices are -1), then
 *   accumulate 0, no base: out[p] = s;   accumulate 1: out[p] = out[p] + s;
 *   base_table [base_rows, dim] + base_ids [n] (both or neither; accumulate must be 0): out[p] = base_table[base_ids[p]] + s,
 *   a base id outside [0, base_rows) giving a zero row and (unless it is -1) setting *oob_flag: tt_embedding_gather_f32's rule.
 * idx_out int32 [n, F] (may be NULL): the F indices of every pair, for the backward launch.  dim a multiple of 4 in 4..512;
 * table, out and base_table 16-byte aligned; n < 2^31.  n == 0 launches nothing.  Launches only.
 * Backward, one launch, NO atomics: grad[off_f + r][c] = sum of dy[p][c] over the pairs p with idx[p, f] == r, for every
 * field f and every row r of it - EVERY row of grad [R, dim] is written in full (a row nobody hit: zeros; the caller does not
 * clear it; n == 0 writes all zeros).  An index that is negative or >= the field's row count matches nothing.  The order of
 * the sum is a fixed function of (n, idx), bit-identical across runs: 32 sub-sums, sub-sum g over the matching positions
 * p = g, g + 32, g + 64, ... in ascending order starting from +0, then (((s_0 + s_1) + s_2) + ... + s_31).
 * dy and grad 16-byte aligned.  Anything else is TT_ERR_INVALID_ARG before any launch.                                     */
int tt_time_context_fwd_f32(const int64_t* timestamps, int64_t n, const float* table, int64_t table_rows, int32_t dim,
                            int32_t field_mask, int32_t buckets, int64_t time_min, int64_t time_max,
                            float* out, int32_t accumulate, const float* base_table, int64_t base_rows,
                            const int64_t* base_ids, int32_t* idx_out, int32_t* oob_flag, tt_stream_t stream);
int tt_time_context_bwd_f32(const int32_t* idx, const float* dy, int64_t n, int32_t dim, int32_t field_mask,
                            int32_t buckets, int64_t table_rows, float* grad, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * MMR diversified re-ranking with per-group caps (added to v10: a new symbol only, the version is unchanged; csrc/mmr.hip) -
 * Maximal Marginal Relevance (Carbonell & Goldstein 1998) over the pool of candidates a top-K call returned.
 * Per query: scores f32 [k1] (best first) and idx int64 [k1] (rows of c, -1 = padding) as every index writes them; c f32
 * [nc, dim], the corpus in ORIGINAL row order; groups int32 [nc] (NULL: no cap) with max_per_group = m (0: no cap; groups is
 * then not read); lambda in [0, 1]; k <= k1.  Every operation is ONE IEEE f32 operation, rounded once:
 *   valid(j)  = 0 <= idx[j] < nc and scores[j] finite; an invalid candidate is never read from c and never picked
 *   dot(a, b) = four partial sums s_e, e = d mod 4, from +0: s_e = s_e + a[d] * b[d] for d ascending (product rounded, then the
 *               sum), joined as (s0 + s1) + (s2 + s3)
 *   n2_j = dot(c_j, c_j);  inv_j = n2_j > 0 ? 1 / sqrt(n2_j) : 0
 *   lo, hi = min, max of the valid scores;  rel_j = hi > lo ? (s_j - lo) / (hi - lo) : 0
 *   pen_j = 0, cnt_j = 0, om = 1 - lambda; then for t = 0 .. k - 1:
 *     eligible(j) = valid, unpicked and - with m > 0 and groups[idx[j]] >= 0 - cnt_j < m
 *     p = the eligible j with the largest val_j = lambda * rel_j - om * pen_j, ties to the lower position j; none: stop
 *     out_scores[t] = scores[p] (the ORIGINAL score: the list need not be monotone), out_idx[t] = idx[p]
 *     every valid j: sim = (dot(c_j, c_p) * inv_j) * inv_p;  pen_j = max(pen_j, sim)  (cosine, floored at 0);
 *                    cnt_j += 1 where groups[idx[j]] == groups[idx[p]] >= 0
 *   the unfilled tail is (-inf, -1).
 * Hence lambda = 1 without a cap returns the first k valid candidates unchanged; a group id of -1 is never capped; a
 * query's row is bit-identical alone, in any batch and on any run.  c must be finite.
 * One launch, one workgroup per query, no workspace, no atomics, nothing copied to the host; nq == 0 launches nothing.
 * Refused with TT_ERR_INVALID_ARG before any launch: a null pointer (groups excepted), nq < 0 (or > 2^31 - 1), k1 outside
 * 1..TT_TOPK_MAX_K, k outside 1..k1, dim not a multiple of 4 in 4..1024, nc outside 1..2^31 - 1, lambda outside [0, 1] or
 * NaN, max_per_group < 0, max_per_group > 0 with groups == NULL, c not 16-byte aligned.  Profiling tag: mmr.             */
int tt_mmr_rerank_f32(const float* scores, const int64_t* idx, int64_t nq, int32_t k1, const float* c, int64_t nc, int32_t dim,
                      const int32_t* groups /* NULL: no cap */, int32_t max_per_group, float lambda, int32_t k,
                      float* out_scores, int64_t* out_idx, tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * GRU encoder of the user history (added to v10: new symbols only, the version is unchanged; csrc/history_gru.hip) - Keras
 * GRU(units = dim, reset_after = True), zero initial state, mask-aware stepping over the kept slots of a bag in slot order (the
 * newest kept item is the last step).  W, U [dim, 3 dim] f32 row-major with the gate column blocks z | r | n, b_i, b_r [3 dim]:
 *   a = x_t W + b_i     g = h U + b_r     z = sigmoid(a_z + g_z)     r = sigmoid(a_r + g_r)     n = tanh(a_n + r g_n)
 *   h <- z h + (1 - z) n              a skipped slot leaves h untouched, bit for bit; a bag without a kept slot: h = 0
 * dim a multiple of 32 in 32..256, L in 1..64, n_bags * L < 2^31.  All f32; the products run on the f32-input MFMA.
 * tt_history_gru_resolve_f32, one launch: batch_ids [n_bags * L] (may be NULL) = every slot's token, -1 where skipped, and
 *   x [n_bags * L, dim] = the slot's table row, zeros where skipped - tokens, bag_rows, exclude and *oob_flag follow
 *   tt_history_attention_fwd_f32's rules (padding, out-of-range tokens and bag rows, the excluded token).
 * The input projection a = x W + b_i over all n_bags * L rows is tt_dense_fwd_batched_f32 (m = n_bags * L, k = dim, n = 3 dim).
 * tt_history_gru_fwd_f32, one launch: out[b] = base_table[base_ids[b]] + h_final (base_table / base_ids both or neither; a base
 *   id out of range: a zero row and, unless -1, the flag; a bag without a kept slot: the base row itself).  gates
 *   [n_bags * L, 3 dim], gn [n_bags * L, dim] and hprev [n_bags * L, dim] (all three or none) keep what the backward needs:
 *   z | r | n and g_n of every KEPT slot (a skipped slot's row of gates is its row of a, its row of gn zeros) and h_{t-1} of
 *   every slot - all three written in full.  gates may BE a (in place); no other buffers may alias.  A bag's bits depend on
 *   that bag alone.
 * tt_history_gru_bwd_f32, one launch, slots in reverse from dh = dy [n_bags, dim]:
 *   dn = dh (1 - z)   dz = dh (h_{t-1} - n)   da_n = dn (1 - n^2)   da_z = dz z (1 - z)   da_r = da_n g_n r (1 - r)
 *   da [n_bags * L, 3 dim] = [da_z | da_r | da_n]    dg [n_bags * L, 3 dim] = [da_z | da_r | da_n r]    dh <- z dh + dg U^T
 *   every row of da and dg is written (a skipped slot: zeros, dh carried).  Then, through tt_dense_bwd_batched_f32:
 *   slot_grads = da W^T (one row per slot, what the sort plan over batch_ids feeds the sparse optimizers), dW = x^T da,
 *   db_i = sum da, dU = hprev^T dg, db_r = sum dg - as slabs the dense segments sum.
 * No atomics (but the flag), nothing read back, bit-identical run to run.  n_bags == 0 launches nothing; anything else wrong is
 * TT_ERR_INVALID_ARG before any launch.                                                                                    */
int tt_history_gru_resolve_f32(const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                               int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags,
                               const int64_t* exclude, float* x, int64_t* batch_ids, int32_t* oob_flag, tt_stream_t stream);
int tt_history_gru_fwd_f32(const float* a, const int64_t* batch_ids, int64_t n_bags, int32_t L, int32_t dim,
                           const float* u, const float* b_r, float* out, const float* base_table, int64_t base_rows,
                           const int64_t* base_ids, int32_t* oob_flag, float* gates, float* gn, float* hprev,
                           tt_stream_t stream);
int tt_history_gru_bwd_f32(const int64_t* batch_ids, const float* gates, const float* gn, const float* hprev,
                           const float* dy, int64_t n_bags, int32_t L, int32_t dim, const float* u, float* da, float* dg,
                           tt_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Multi-head self-attention encoder of the user history (added to v10: new symbols only, the version is unchanged;
 * csrc/history_selfattn.hip) - one causal attention block read at the last position: the newest kept item n of a bag is the one
 * query.  With x_j the table rows of the kept slots, r_j the kept slots behind j, heads H, Wqk [dim, H dim], Wvo [H dim, dim],
 * p [H, L], all f32 row-major:
 *   T = x_n Wqk     e_hj = <x_j, T_h> / sqrt(dim) + p[h, r_j]     w_h = softmax_j(e_h)     P_h = sum_j w_hj x_j
 *   out[b] = base row + concat_h(P_h) Wvo            a bag without a kept slot: the base row itself
 * dim a multiple of 32 in 32..256, L in 1..64, heads in {1, 2, 4, 8}, n_bags * L < 2^31.  The two products over n_bags rows are
 * tt_dense_fwd_batched_f32 (T: m = n_bags, k = dim, n = H dim, no bias; O: k = H dim, n = dim) and, backward,
 * tt_dense_bwd_batched_f32 ((dP, dWvo) from dy and (dxn, dWqk) from dT).
 * tt_history_self_attention_resolve_f32, one launch: batch_ids [n_bags * L] = every slot's token, -1 where skipped, newest
 *   [n_bags] = the slot of n (-1: no kept slot), xn [n_bags, dim] = its row (+0 for such a bag) - tokens, bag_rows, exclude and
 *   *oob_flag follow tt_history_attention_fwd_f32's rules; base_ids (may be NULL) [n_bags] only sets the flag for an id outside
 *   0..base_rows other than -1.
 * tt_history_self_attention_pool_fwd_f32, one launch: from batch_ids, t [n_bags, H dim] and p: pooled [n_bags, H, dim] and weights
 *   [n_bags, H, L] - exactly 0 in a skipped slot, exactly 1 for a single kept slot, both written in full.  A slot's row is
 *   loaded once for all heads; a bag's bits depend on that bag alone.
 * tt_history_self_attention_combine_f32, one launch, in place: out[b] = base_table[base_ids[b]] + out[b] (a base id out of range: a
 *   zero row), and for newest[b] < 0 the base row itself.
 * tt_history_self_attention_pool_bwd_f32, one launch, with dpooled [n_bags, H, dim] = dy Wvo^T:
 *   G_h = <dP_h, P_h>    t_hj = <dP_h, x_j>    de_hj = w_hj (t_hj - G_h)
 *   slot_grads[b L + j] = sum_h (w_hj dP_h + de_hj T_h / sqrt(dim))   one row per KEPT slot, a skipped slot's row untouched
 *   dt [n_bags, H dim]: dT_h = sum_j de_hj x_j / sqrt(dim), every row written;    dp[h, r_j] += de_hj as dp_slabs [n_slabs, H L]
 *   over contiguous bags, every slab written in full and summed in a fixed order - the form tt_dense_seg / tt_adam_seg sum
 *   (slab_stride = H L).  tt_history_self_attention_num_slabs(n_bags) is a host query for a good n_slabs.
 * tt_history_self_attention_query_grad_f32, one launch: slot_grads[b L + newest[b]] += dxn[b] where newest[b] >= 0 (dxn = dT Wqk^T).
 * No atomics (but the flag), no workspace to zero, nothing read back, bit-identical run to run.  n_bags == 0 launches nothing;
 * anything else wrong is TT_ERR_INVALID_ARG before any launch.                                                             */
int tt_history_self_attention_resolve_f32(const float* table, int64_t table_rows, int32_t dim, const int32_t* tokens,
                                          int64_t n_token_rows, int32_t L, const int64_t* bag_rows, int64_t n_bags,
                                          const int64_t* exclude, const int64_t* base_ids, int64_t base_rows, int64_t* batch_ids,
                                          int32_t* newest, float* xn, int32_t* oob_flag, tt_stream_t stream);
int tt_history_self_attention_pool_fwd_f32(const float* table, int64_t table_rows, int32_t dim, int32_t L, int32_t heads,
                                           const int64_t* batch_ids, int64_t n_bags, const float* t, const float* p, float* pooled,
                                           float* weights, tt_stream_t stream);
int tt_history_self_attention_combine_f32(float* out, const int32_t* newest, int64_t n_bags, int32_t dim, const float* base_table,
                                          int64_t base_rows, const int64_t* base_ids, tt_stream_t stream);
int32_t tt_history_self_attention_num_slabs(int64_t n_bags);
int tt_history_self_attention_pool_bwd_f32(const float* table, int64_t table_rows, int32_t dim, int32_t L, int32_t heads,
                                           const int64_t* batch_ids, const float* weights, const float* pooled, const float* dpooled,
                                           const float* t, int64_t n_bags, float* slot_grads, float* dt, float* dp_slabs,
                                           int32_t n_slabs, tt_stream_t stream);
int tt_history_self_attention_query_grad_f32(const int32_t* newest, const float* dxn, int64_t n_bags, int32_t L, int32_t dim,
                                             float* slot_grads, tt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TWOTOWER_HIP_H */
