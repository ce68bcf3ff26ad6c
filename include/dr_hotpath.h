/*
 * dr_hotpath.h — C-ABI of the MI355X-native embedding-lookup + feature-interaction hot path.
 *
 * The reference (LongmaoTeamTf/deep_recommenders) is pure Python over TensorFlow and has no
 * FFI of its own; the drop-in boundary is therefore the set of TF-op clusters
 * its Python classes invoke.  Each entry point below replaces one such cluster and cites the
 * reference call site it stands behind (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless marked [host]; the caller allocates all
 *     inputs and outputs; the library holds no state between calls;
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous and stream-ordered,
 *     no hidden synchronisation, re-entrant across streams;
 *   - return value: DR_OK (0) or a negative DR_E* code; nothing throws across the boundary;
 *   - ids are int64, -1 = "missing" (TF drops -1 / "" before lookup);
 *   - all floating point is IEEE fp32 ("f32" in bench.py's dtype field).
 *
 * Layout of categorical inputs ("columns"): a batch is an int64 matrix ids[B, C]; field f owns the
 * contiguous columns [col_start[f], col_start[f+1]) (its bag, padded with -1), C = col_start[F].
 * All F embedding tables live in ONE fp32 slab table[R, D]; field f's rows start at row_base[f].
 * The first-order ("linear"/"indicator") weights use the same row numbering: lin_w[R].
 */
#ifndef DR_HOTPATH_H
#define DR_HOTPATH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_OK 0
#define DR_EINVAL (-1)   /* bad argument (null pointer, negative size, unsupported D)     */
#define DR_ELAUNCH (-2)  /* hipLaunch / runtime error (hipGetLastError() != hipSuccess)  */
#define DR_ESHAPE (-3)   /* shape contract violated (e.g. x0 / x dim mismatch, k > n)    */

typedef void* dr_stream_t; /* hipStream_t */

/* Library self-description: returns the gfx arch string the kernels were compiled for. */
const char* dr_version(void);

/* How the fp32 GEMMs of the tower and cross layers (dr_linear_fwd / _bwd_dx / _bwd_dx_fm / _bwd_dw, dr_cross_fwd) and the
 * top-K score kernels (dr_scores_nt, the scan inside dr_topk_mips -- always the same mode, so equal candidates tie) form
 * their products.  Inputs, outputs and accumulators are fp32 in both modes; the reference's own ops are tf.matmul on
 * fp32 tensors (keras/models/ranking/deepfm.py:30-34, dcn.py:81-88), compared at 1e-5 on the loss.
 *   DR_GEMM_BF16X3      (default) every operand value x is split exactly into three bf16 terms x0 + x1 + x2 and a * b is
 *                       accumulated as a0b0 + a0b1 + a1b0 + a0b2 + a1b1 + a2b0 on v_mfma_f32_32x32x16_bf16 (each bf16
 *                       product is exact in the fp32 accumulator; the dropped terms are < 2^-24 |ab|).  Measured error
 *                       against an fp64 reference is equal to or below the native path's (tests/test_gpu_kernels.py).
 *   DR_GEMM_NATIVE_F32  v_mfma_f32_32x32x2_f32 products.
 * dr_set_gemm_mode returns the previous mode (DR_EINVAL for an unknown one); the setting is process-wide and read at
 * launch time.  Environment override of the initial value: DR_GEMM_MODE=native | bf16x3. */
#define DR_GEMM_BF16X3 0
#define DR_GEMM_NATIVE_F32 1
int32_t dr_set_gemm_mode(int32_t mode);
int32_t dr_get_gemm_mode(void);

/* The operand split of the register-split GEMMs under DR_GEMM_BF16X3 (the dr_bf3_* / dr_h2_* families below): how many low-precision
 * terms carry one fp32 operand value.
 *   DR_GEMM_SPLIT_F16X2   (default) two fp16 terms of x * 2^k, three matrix instructions per fragment pair (dr_h2_*; 22 significant
 *                         bits per operand, whole-GEMM error against fp64 at or below the six-product split's: DESIGN.md §3)
 *   DR_GEMM_SPLIT_BF16X3  three bf16 terms, six matrix instructions per fragment pair (dr_bf3_*)
 * The dr_bf3_* and dr_h2_* entry points are explicit and ignore this setting; it is the ONE switch the callers that choose between
 * them consult -- the engines of the host package at construction, and dr_topk_mips (the exact scan picks dr_h2_* or dr_bf3_*) at
 * every call.  dr_set_gemm_split returns the previous value (DR_EINVAL for an unknown one); process-wide.  Environment override of
 * the initial value, parsed here and nowhere else: DR_GEMM_SPLIT=f16x2 (or unset) | anything else = bf16x3. */
#define DR_GEMM_SPLIT_BF16X3 0
#define DR_GEMM_SPLIT_F16X2 1
int32_t dr_set_gemm_split(int32_t split);
int32_t dr_get_gemm_split(void);

/* ------------------------------------------------------------------------------------------
 * K1  hash-bucket column:  id = int64( FarmHash::Fingerprint64(as_string(key)) mod N )
 * replaces [TF] categorical_column_with_hash_bucket ->
 *   string_to_hash_bucket_fast(as_string(x), N)
 * reference call sites: examples/train_fm_on_movielens_estimator.py:12-13,20-21;
 *   examples/train_deepfm_on_movielens_keras.py:13-14,21-22; tests/keras/test_fm.py:70-73
 * keys[B, C] int64; col_buckets[C] uint64: N for a hashed column, 0 = pass the value through
 * unchanged (column already holds ids, e.g. from dr_vocab_lookup_*).  key == -1 -> id -1.
 * Bit-exact integer path.
 * ---------------------------------------------------------------------------------------- */
int dr_hash_bucket_i64(const int64_t* keys, int64_t B, int32_t C, const uint64_t* col_buckets,
                       int64_t* ids_out, dr_stream_t stream);

/* Same for byte strings in CSR form (bytes + offsets[n+1]); "" -> id -1. One bucket count. */
/* ids [B, F] int64 -> out [F][B] int32, field-major (what dr_bf3_wgrad_emb reads: one 128-byte line per 32 examples of a field) */
int dr_ids_transpose_i32(const int64_t* ids, int64_t B, int32_t F, int32_t* out, dr_stream_t stream);
int dr_hash_bucket_bytes(const uint8_t* bytes, const int64_t* offsets, int64_t n,
                         uint64_t num_buckets, int64_t* ids_out, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K2  vocabulary-list column: id = position of key in vocab, OOV -> -1 (default_value=-1,
 * num_oov_buckets=0).  replaces [TF] categorical_column_with_vocabulary_list
 * reference call sites: examples/train_fm_on_movielens_estimator.py:14-19,22-23
 * ---------------------------------------------------------------------------------------- */
int dr_vocab_lookup_i64(const int64_t* keys, int64_t n, const int64_t* vocab, int32_t vocab_len,
                        int64_t* ids_out, dr_stream_t stream);
int dr_vocab_lookup_bytes(const uint8_t* bytes, const int64_t* offsets, int64_t n,
                          const uint8_t* vocab_bytes, const int64_t* vocab_offsets,
                          int32_t vocab_len, int64_t* ids_out, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K3 (+K5, K6 fused)  embedding gather + mean-pool forward.
 * replaces, in ONE pass: [TF] safe_embedding_lookup_sparse(combiner='mean') x F
 *   (keras/models/ranking/fm.py:48-51,57-61; deepfm.py:25-28,39-43; estimator/.../fm.py:48-52),
 *   tf.stack / tf.concat (fm.py:62; deepfm.py:44-45), the first-order term
 *   DenseFeatures(indicator)->Dense(1) / linear_model (fm.py:16-20,47,55; estimator fm.py:43-44)
 *   and the FM second-order term (fm.py:28-35; estimator fm.py:22-26).
 *
 *   concat[b, f*D + d] = mean over valid ids of field f of table[row_base[f]+id, d]  (0 if empty)
 *   sum_x[b, d]        = sum_f concat[b, f*D+d]                                   (optional)
 *   fm_logit[b]        = lin_bias[0] + sum over valid ids lin_w[row] + 0.5*sum_d(sum_x^2 - sum_f x^2)
 *
 * col_start[F+1] (device, int32) may be NULL when every field is single-valued (then C == F).
 * concat has leading dimension ld_concat (>= F*D) so the caller can append dense features.
 * lin_w may be NULL (no first-order term); lin_bias is a 1-element device array (the trained bias) or
 * NULL; sum_x / fm_logit may be NULL (pure lookup).
 * D must be a multiple of 4, 4 <= D <= 256.
 * flags: 0, or DR_POOL_FIRST_ORDER_ONLY: fm_logit = lin_bias + sum w (no second-order term) -- the "wide" logit of
 * WDL (`tf.feature_column.linear_model`, estimator/models/ranking/wide_and_deep.py:30-32 of the reference).
 * ---------------------------------------------------------------------------------------- */
#define DR_POOL_FIRST_ORDER_ONLY 1
int dr_emb_pool_fwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start,
                    const int64_t* row_base, const float* table, int32_t D,
                    const float* lin_w, const float* lin_bias,
                    float* concat, int64_t ld_concat, float* sum_x, float* fm_logit,
                    int32_t flags, dr_stream_t stream);
/* Per-field first-order outputs (FNN, estimator/models/ranking/fnn.py:53-64: a bias-free Dense(1) over every indicator
 * column's multi-hot input, concatenated):  out[b][f] = sum over the bag of field f of lin_w[row_base[f] + id]  (ids < 0
 * skipped).  bwd: dst_lin[row] += scale * d_out[b][f] for every id of the bag (fp32 atomics). */
int dr_lin_fields_fwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start,
                      const int64_t* row_base, const float* lin_w, float* out, int64_t ld_out,
                      dr_stream_t stream);
int dr_lin_fields_bwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start,
                      const int64_t* row_base, const float* d_out, int64_t ld_dout, float scale,
                      float* dst_lin, dr_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * K4  transposed scatter-add backward of K3 (autodiff of the lookup: IndexedSlices ->
 * unsorted_segment_sum into the variable; implicit in optimizer.minimize / model.fit:
 * examples/train_fm_on_movielens_estimator.py:51-52, examples/train_deepfm_on_movielens_keras.py:49).
 *
 *   g[b,f,:]   = d_concat[b, f*D:(f+1)*D] + d_fm_logit[b] * (sum_x[b,:] - concat[b, f*D:(f+1)*D])
 *   for every valid id of (b,f):  dst_table[row,:] += scale * g[b,f,:] / bag_count(b,f)
 *                                  dst_lin[row]    += scale * d_fm_logit[b]
 *   dst_bias[0] += scale * sum_b d_fm_logit[b]                       (dst_bias may be NULL)
 *
 * dst_table / dst_lin are either gradient buffers (scale = 1) or the parameters themselves
 * (scale = -learning_rate: fused SGD step, no gradient materialised).  d_concat may be NULL
 * (FM only), d_fm_logit may be NULL (pure lookup backward), dst_lin may be NULL.  concat == sum_x == NULL with d_fm_logit
 * given: the logit was first-order only (DR_POOL_FIRST_ORDER_ONLY), its gradient reaches dst_lin / dst_bias only.
 * Accumulation uses hardware fp32 atomics; rows touched once are bit-exact.
 * ---------------------------------------------------------------------------------------- */
int dr_emb_pool_bwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start,
                    const int64_t* row_base, int32_t D,
                    const float* d_concat, int64_t ld_dconcat,
                    const float* concat, int64_t ld_concat, const float* sum_x,
                    const float* d_fm_logit, float scale,
                    float* dst_table, float* dst_lin, float* dst_bias, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K4, deterministic form (single-valued fields, C == F <= 64): build the slot plan once per batch
 * (dr_emb_sort_slots -- depends only on ids, so it can run on a side stream): flag the slots whose row is unique in
 * the batch and group the slots of shared rows by row; dr_emb_pool_bwd_sorted then applies
 *     dst_table[row,:] += scale * sum_slots grad[b, f*D:(f+1)*D]      dst_lin[row] += scale * sum_slots d_fm_logit[b]
 *     dst_bias[0]      += scale * sum_b d_fm_logit[b]
 * with (a) a streaming pass in example order doing ONE plain read-modify-write per unique row, and (b) a
 * segmented pass in sorted order for rows hit by several slots.  Per-slot gradient = grad[b, f*D:(f+1)*D]
 * (+ d_fm_logit[b] * (sum_x[b,:] - concat[b, f*D:(f+1)*D]) when concat / sum_x are given, as in
 * dr_emb_pool_bwd; pass NULL when `grad` already holds it).  slot_lin_grad[n] (may be NULL) replaces d_fm_logit[b]
 * as the per-slot first-order gradient -- the owner side of the sharded exchange receives gradients per slot.  Rows hit by <= 32 slots are bit-reproducible; hotter rows are cut into
 * pieces that combine with fp32 atomics.
 * The plan (csrc/emb_plan.hip; hand-written, no library sort): unique_flags[n] uint8 (indexed by slot = b*F + f);
 * dup_count[2] int32 = {number of work-list entries, length L of the sorted arrays}; sorted_rows[0..L) int64 ascending with
 * sorted_slots[0..L) int32 ordered by slot inside a row; dup_heads[n] int32 = the duplicate pass's work list (sorted positions
 * heading a piece of a multiply-hit row).  L is either the number of slots on shared rows (claim path: an open-addressed
 * table claims every row, the few shared-row slots are sorted by one block in LDS -- uniform ids) or n with missing ids
 * carrying num_rows at the end (radix path: shared-row slots beyond the LDS list, n > 2^24 or num_rows >= 2^31 - 1); the
 * choice is made on the device, the host never waits.  Arrays must hold n entries either way.  workspace >=
 * dr_emb_sort_workspace_bytes(n) bytes.  dr_emb_plan_set_small_limit(limit): largest shared-row list the LDS sort takes
 * (default / maximum 16384; 0 forces the radix path whenever a row is shared) -- returns the previous value, process-wide.
 * ---------------------------------------------------------------------------------------- */
int64_t dr_emb_sort_workspace_bytes(int64_t n);
int32_t dr_emb_plan_set_small_limit(int32_t limit);
int dr_emb_sort_slots(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, int64_t num_rows,
                      int64_t* sorted_rows, int32_t* sorted_slots, uint8_t* unique_flags,
                      int32_t* dup_heads, int32_t* dup_count, void* workspace, int64_t workspace_bytes,
                      dr_stream_t stream);
/* Round 6 -- K1, the field-major ids and the slot plan of one batch in ONE chain (the engines' next-batch prefetch):
 * dr_hash_bucket_i64(keys [B, F], col_buckets -> ids_out [B, F]), dr_ids_transpose_i32(ids_out -> ids_t_out [F, B] int32; ids_t_out may be
 * NULL) and dr_emb_sort_slots(ids_out, ...), bit for bit, with hash, transpose, composite keys and partition histogram as one kernel when
 * F <= 64 and the geometry fits the composite key (otherwise the three entry points are called one after the other).  Replaces the same
 * reference lines as K1 ([TF] categorical_column_with_hash_bucket, examples/train_fm_on_movielens_estimator.py:12-13,20-21) and the
 * plan (the grouping half of unsorted_segment_sum in the autodiff of keras/models/ranking/fm.py:57-61). */
int dr_hash_sort_slots(const int64_t* keys, int64_t B, int32_t F, const uint64_t* col_buckets, int64_t* ids_out,
                       int32_t* ids_t_out, const int64_t* row_base, int64_t num_rows, int64_t* sorted_rows,
                       int32_t* sorted_slots, uint8_t* unique_flags, int32_t* dup_heads, int32_t* dup_count, void* workspace,
                       int64_t workspace_bytes, dr_stream_t stream);
/* dr_hash_sort_slots issued in two parts on ONE stream, for a caller that records an event between them (the next forward needs only the
 * ids; the plan has one reader, K4).  parts & 1: every launch that writes ids_out / ids_t_out (the fused front kernel; in the fallback
 * geometries dr_hash_bucket_i64 + dr_ids_transpose_i32).  parts & 2: the rest of the plan; it reads what part 1 left in ids_out, sorted_rows
 * and the workspace, which nothing may touch in between.  parts == 3: dr_hash_sort_slots, launch for launch. */
int dr_hash_sort_slots_parts(const int64_t* keys, int64_t B, int32_t F, const uint64_t* col_buckets, int64_t* ids_out,
                             int32_t* ids_t_out, const int64_t* row_base, int64_t num_rows, int64_t* sorted_rows,
                             int32_t* sorted_slots, uint8_t* unique_flags, int32_t* dup_heads, int32_t* dup_count, void* workspace,
                             int64_t workspace_bytes, int32_t parts, dr_stream_t stream);
int dr_emb_pool_bwd_sorted(const int64_t* ids, const int64_t* row_base, const int64_t* sorted_rows,
                           const int32_t* sorted_slots, const uint8_t* unique_flags,
                           const int32_t* dup_heads, const int32_t* dup_count, int64_t B, int32_t F,
                           int32_t D, int64_t num_rows, const float* grad, int64_t ld_grad,
                           const float* concat, int64_t ld_concat, const float* sum_x,
                           const float* d_fm_logit, const float* slot_lin_grad, float scale,
                           float* dst_table, float* dst_lin, float* dst_bias, float* x_sorted,
                           const float* lin_old_t, int32_t parts, uint32_t* table_amax, dr_stream_t stream);
/* The FM term (sum_x, d_fm_logit given) needs x[b, f, :] of every slot: for a slot that owns its row it is the row's own value
 * (read by the update anyway); for slots that SHARE a row it comes from `concat` if the forward stored it, else from
 * x_sorted [B * F, D], where dr_emb_snapshot_sorted_rows has placed -- before the update starts -- the row of every work-list
 * head at the head's sorted position (one row per piece of a shared row: 5.6 K rows for uniform ids at config 3)
 * (round 3: the fused first layer no longer stores concat, the wgrad gathers its operand from the tables -- dr_bf3_wgrad_emb).
 * (With the deterministic SGD update below the snapshot is not needed: x is then read from the table inside the update -- no row
 * is written before its reader has it.  The Adam variant and DR_K4_DETERMINISTIC=0 still read the snapshot.)
 * x_sorted also makes the SGD update of HOT rows (more than 32 slots of the batch, cut into pieces of 32 that run in parallel)
 * deterministic: with x_sorted == NULL the pieces combine with fp32 atomics (order-dependent rounding); with x_sorted given each
 * piece parks its sum in its own row of x_sorted (overwriting the snapshot it has consumed) and a second small launch inside
 * the call adds a row's pieces in sorted order and updates the row once -- the same batch then gives the same bits, whatever
 * the id distribution.  (The Adam variant always sums a row's slots in one lane group and never used atomics.) */
/* parts -- the call in two halves, for callers that time or overlap them separately: 1 = the update kernel, 2 = the ordered combination
 * of hot rows' parked pieces, 3 = both (the whole update).  Part 2 must follow part 1 on the same stream before the tables are read;
 * it is a no-op without x_sorted.  Two more bits select what part 1 covers; parts must lie in 1..15 with (parts & 3) != 0 (DR_EINVAL
 * otherwise). */
/* parts | 8: the slots whose row is unique in the batch were updated elsewhere (dr_h2_dgrad_emb_sgd) -- only the duplicate pass, the
 * hot rows and the first-order bias run here; `grad` need hold the rows of the non-unique slots only.
 * lin_old_t [F, B] (field-major, may be NULL): the first-order weights as the forward of THIS step read them (lin_vals_t of
 * dr_bf3_emb_linear_fwd).  A row unique in the batch then gets dst_lin[row] = lin_old + scale * g as ONE write instead of a
 * read-modify-write (K4 is bound by 128-byte line operations; this removes one of eight per slot).  Valid only if nothing wrote
 * dst_lin since that forward; ignored with slot_lin_grad.
 * table_amax (may be NULL): running amax record of dst_table -- raised to the largest |value| this call writes into the table (the
 * f16x2 GEMMs, dr_h2_emb_linear_fwd / dr_h2_wgrad_emb, scale the table rows by it). */
/* parts | 4: first-order weights of rows unique in the batch are NOT updated by the call; dr_emb_lin_update_unique applies exactly that
 * part (dst_lin[row] += scale * gradient for every slot whose unique flag is set), on any stream between the head's backward and
 * the next forward.  Why: a random 4-byte read-modify-write fetches a 128-byte line -- 0.27 GB of K4's 1.64 GB at config 3 -- and
 * beside a matrix-bound GEMM that traffic is free. */
int dr_emb_lin_update_unique(const int64_t* ids, const uint8_t* unique_flags, int64_t B, int32_t F, const int64_t* row_base,
                             const float* d_fm_logit, const float* slot_lin_grad, float scale, float* dst_lin, dr_stream_t stream);
int dr_emb_snapshot_sorted_rows(const int64_t* sorted_rows, const int32_t* dup_heads, const int32_t* dup_count,
                                const float* table, int32_t D, int64_t num_rows, float* x_sorted, dr_stream_t stream);

/* SURVEY.md section 8f rank 1 -- the optimizer of the reference's own examples (tf.train.AdamOptimizer(0.01),
 * examples/train_fm_on_movielens_estimator.py:51-52; tf.keras.optimizers.Adam(), examples/train_deepfm_on_movielens_keras.py:44)
 * fused into the sorted K4: every row the batch touches gets ONE Adam update from the SUM of its slots' gradients
 *   m = b1 m + (1-b1) g ;  v = b2 v + (1-b2) g^2 ;  w -= lr_t m / (sqrt(v) + eps),   lr_t = lr sqrt(1-b2^t) / (1-b1^t)
 * (lr_t computed by the caller).  `grad` is the gradient of the mean loss (no scale).  m_table / v_table [R, D] and
 * m_lin / v_lin [R] are the moment slabs.  Rows the batch does not touch keep their moments (row-wise "lazy" Adam):
 * equal to TF's Adam on the first step and for rows touched on every step; TF decays m/v of the whole variable each step
 * (SURVEY App. B15), which is a full pass over the 66 GB table at config 3.  The first-order bias is a dense parameter:
 * dr_adam_step.  Deterministic (a row's slots are summed by one lane group in sorted order). */
/* (round 4) m_lin / v_lin may be the two columns of ONE [R, 2] array -- pass v_lin == m_lin + 1 -- and are then addressed with a row
 * stride of 2: a row's first-order moments share a cache line (one line operation to read, one to write, instead of two each).  The
 * same convention holds for dr_adam_catchup_rows.
 * lin_old_t (may be NULL) and table_amax (may be NULL): as in dr_emb_pool_bwd_sorted. */
int dr_emb_pool_bwd_sorted_adam(const int64_t* ids, const int64_t* row_base, const int64_t* sorted_rows,
                                const int32_t* sorted_slots, const uint8_t* unique_flags,
                                const int32_t* dup_heads, const int32_t* dup_count, int64_t B, int32_t F,
                                int32_t D, int64_t num_rows, const float* grad, int64_t ld_grad,
                                const float* concat, int64_t ld_concat, const float* sum_x,
                                const float* d_fm_logit, const float* slot_lin_grad, float lr_t, float beta1,
                                float beta2, float eps, float* table, float* m_table, float* v_table,
                                float* lin_w, float* m_lin, float* v_lin, float* x_sorted, const float* lin_old_t,
                                uint32_t* table_amax, dr_stream_t stream);
/* Dense Adam step (same formula) over a flat parameter buffer; grad is multiplied by grad_scale first. */
/* TF's NON-lazy sparse Adam, evaluated lazily (examples/train_fm_on_movielens_estimator.py:51-52: tf.train.AdamOptimizer decays
 * m / v of the WHOLE variable and moves every row on every step).  row_step[R] int32 (zero-initialised) counts
 * the optimizer steps a row has received; dr_adam_catchup_rows brings the rows named by ids[n] (field of slot p = p % F, -1 =
 * missing) to `upto` steps by replaying their missed decay-only steps  m *= b1 ; v *= b2 ; w -= lr_s m / (sqrt(v) + eps)
 * (lr_s = lr sqrt(1 - b2^s) / (1 - b1^s)) in order, and stamps them `stamp`.  Before the forward of step t: upto = t - 1,
 * stamp = t, then dr_emb_pool_bwd_sorted_adam applies step t -- every value the model reads equals TF's dense update.  To
 * export the tables: upto = stamp = steps taken, over all rows.  One replayer per row and call (atomic exchange of the stamp).
 * D: 4 .. 256, a multiple of 4, as for the kernels that share the tables (DR_EINVAL otherwise). */
int dr_adam_catchup_rows(const int64_t* ids, int64_t n, int32_t F, const int64_t* row_base, int32_t D, float* table,
                         float* m_table, float* v_table, float* lin_w, float* m_lin, float* v_lin, int32_t* row_step,
                         int32_t upto, int32_t stamp, float lr, float beta1, float beta2, float eps, dr_stream_t stream);
int dr_adam_step(float* param, const float* grad, float* m, float* v, int64_t n, float lr_t, float beta1,
                 float beta2, float eps, float grad_scale, dr_stream_t stream);

/* Dense FTRL-Proximal step in TensorFlow's formulation -- tf.train.FtrlOptimizer(0.01, l1_regularization_strength=0.5), the
 * optimizer of WDL's wide part in examples/train_wdl_on_movielens_estimator.py:66-70 (TF defaults: learning_rate_power -0.5,
 * accumulators initialised to 0.1, l2 0):
 *   accum' = accum + g^2 ;  linear += g - (accum'^-p - accum^-p) / lr * w ;  w = |linear| > l1 ? (sign(linear) l1 - linear) /
 *   (accum'^-p / lr + 2 l2) : 0.   grad is multiplied by grad_scale first. */
int dr_ftrl_step(float* param, const float* grad, float* accum, float* linear, int64_t n, float lr,
                 float lr_power, float l1, float l2, float grad_scale, dr_stream_t stream);



/* ------------------------------------------------------------------------------------------
 * K6  stand-alone FM second-order term on a caller-provided [B, F, D] tensor
 * replaces keras FM.call (keras/models/ranking/fm.py:28-35) and estimator fm(x)
 * (estimator/models/feature_interaction/fm.py:10-26).
 *   out[b] = 0.5 * sum_d( (sum_f x)^2 - sum_f x^2 )      dx = d_out[b] * (sum_f x - x)
 * ---------------------------------------------------------------------------------------- */
int dr_fm2_fwd(const float* x, int64_t B, int32_t F, int32_t D, float* out, dr_stream_t stream);
int dr_fm2_bwd(const float* x, const float* d_out, int64_t B, int32_t F, int32_t D, float* dx,
               dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K7  Dense layer on fp32 MFMA (v_mfma_f32_32x32x2_f32: exact f32 products, k-ordered accumulation).
 * replaces tf.keras.layers.Dense / tf.layers.dense (keras/models/ranking/deepfm.py:30-34;
 * estimator/models/feature_interaction/dnn.py:17-29) and, with N = 1, the FM layer's first-order
 * Dense(1) on an explicit multi-hot matrix (keras/models/ranking/fm.py:16-20,26,37)  [K5].
 *
 *   fwd     y[M,N]  = act(x[M,K] @ W[K,N] + b[N])           act: 0 linear, 1 relu; b may be NULL
 *   bwd_dx  dx[M,K] = (dy[M,N] @ W^T) * (relu_src > 0)  (+ dx if accumulate)
 *           dy is the PRE-activation gradient of this layer; relu_src[M,K] (may be NULL) is this
 *           layer's input when that input is itself a relu output — so the product is directly the
 *           pre-activation gradient of the layer below (relu' folded into the producer's epilogue).
 *   bwd_dw  dstW[K,N] += scale * x^T @ dy ;  dstb[N] += scale * colsum(dy)
 *           split over the batch dimension: dst is a zeroed gradient buffer (scale = 1) or the
 *           parameter itself (scale = -lr, fused SGD).  With a workspace of
 *           dr_linear_bwd_dw_workspace_bytes() the split partials are combined by a deterministic
 *           reduce kernel; with workspace == NULL they combine with fp32 atomics.  dstb may be NULL.
 * All matrices row-major with explicit leading dimensions; 16-byte aligned bases with pitches that are
 * multiples of 4 floats take the float4 load path, anything else a scalar-load path.
 * ---------------------------------------------------------------------------------------- */
int dr_linear_fwd(const float* x, int64_t ld_x, const float* W, int64_t ld_w, const float* b,
                  int64_t M, int32_t K, int32_t N, int32_t act, float* y, int64_t ld_y,
                  dr_stream_t stream);
int dr_linear_bwd_dx(const float* dy, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M,
                     int32_t K, int32_t N, const float* relu_src, int64_t ld_relu_src,
                     int32_t accumulate, float* dx, int64_t ld_dx, dr_stream_t stream);
/* dr_linear_fwd_splitk: y += x W for few output tiles and a long reduction (the in-batch softmax's dq = G c of
 * keras/models/retrieval/sbcnm.py:120-163's backward: G [B, B], c [B, 128]): the reduction is split over the grid into `workspace`
 * (dr_linear_fwd_splitk_workspace_bytes) and the slices are summed in a fixed order.  Accumulates into y (zero it for a plain
 * product). */
int64_t dr_linear_fwd_splitk_workspace_bytes(int64_t M, int32_t K, int32_t N);
int dr_linear_fwd_splitk(const float* x, int64_t ld_x, const float* W, int64_t ld_w, int64_t M, int32_t K, int32_t N,
                         float* y, int64_t ld_y, float* workspace, int64_t workspace_bytes, dr_stream_t stream);

/* dgrad of the first tower layer with the FM second-order gradient folded into the epilogue:
 *   dx[m, j] = (dy @ W^T)[m, j] + d_fm_logit[m] * (sum_x[m, j % D] - concat[m, j])   for j < FD (= F*D)
 * (autodiff of keras/models/ranking/fm.py:28-35 + deepfm.py:46 in one stream), so K4 reads one gradient. */
int dr_linear_bwd_dx_fm(const float* dy, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M,
                        int32_t K, int32_t N, const float* d_fm_logit, const float* sum_x,
                        const float* concat, int64_t ld_concat, int32_t D, int32_t FD, float* dx,
                        int64_t ld_dx, dr_stream_t stream);
int64_t dr_linear_bwd_dw_workspace_bytes(int64_t M, int32_t K, int32_t N);
int dr_linear_bwd_dw(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t M,
                     int32_t K, int32_t N, float scale, float* dstW, int64_t ld_w, float* dstb,
                     float* workspace, int64_t workspace_bytes, dr_stream_t stream);
/* Fused backward of a NARROW layer (N <= 32, e.g. the Dense(32) that precedes Dense(1) in the reference's
 * towers, keras/models/ranking/deepfm.py:30-34, estimator/models/feature_interaction/dnn.py:17-29): one pass over x
 * produces  dx = (dy @ W^T) * (x > 0 if relu_mask)  and the fused SGD step  dstW += scale * x^T dy,
 * dstb += scale * colsum(dy)  (dx uses the pre-update W even when dstW == W).  Deterministic.
 * Domain: N <= 32, K in {128, 256, 512}, M a multiple of 32, x/dx rows 4*(K/128)-byte aligned; anything else returns
 * DR_ESHAPE and the caller uses dr_linear_bwd_dx + dr_linear_bwd_dw.
 * parts (1..3) and dx_amax (may be NULL): see "in two halves" below. */
int64_t dr_linear_bwd_narrow_workspace_bytes(int64_t M, int32_t K, int32_t N);
int dr_linear_bwd_narrow(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, const float* W,
                         int64_t ld_w, int64_t M, int32_t K, int32_t N, int32_t relu_mask, float scale,
                         float* dstW, int64_t ld_dstw, float* dstb, float* dx, int64_t ld_dx,
                         void* workspace, int64_t workspace_bytes, int32_t parts, uint32_t* dx_amax, dr_stream_t stream);

/* Fused tower head: the last hidden layer (H <= 32 units), the Dense(1) output that follows it, the FM logit, the loss,
 * and the backward of the Dense(1) -- i.e. keras/models/ranking/deepfm.py:30-34,41-47 `Dense(32, relu)`, `Dense(1)`,
 * `sigmoid(fm + dnn)` plus the loss of examples/train_deepfm_on_movielens_keras.py:43 /
 * examples/train_deepfm_on_movielens_estimator.py:47, in one GEMM launch:
 *   h      = act(x @ W1 + b1)                       [M, H]   (written to h_out if not NULL)
 *   logit  = h @ w2 + b2 + extra_logit              [M]      (w2[n] at w2[n * ld_w2]; extra_logit may be NULL)
 *   prob, loss, d_logit = BCE(logit, labels, loss_mode) as dr_bce_fwd_bwd  (d_logit = d mean-loss / d logit)
 *   d_h    = d_logit (x) w2 * act'(h)               [M, H]   (gradient for dr_linear_bwd_narrow / _bwd_dx)
 *   dst_w2 += scale * h^T d_logit ;  dst_b2 += scale * sum(d_logit)
 *            dst_* = the parameters themselves with scale = -lr (fused SGD; d_h always uses the pre-update w2), or
 *            gradient buffers with scale = 1 (data-parallel: all-reduce, then apply); NULL / scale = 0: skipped
 * n_total (0 = M): the number of examples the loss is a mean over, when these M rows are one slice of a larger batch
 * (micro-batches): loss_out = sum(l) / n_total, d_logit = dl/dlogit / n_total.
 * Deterministic.  H > 32 returns DR_ESHAPE (use dr_linear_fwd x2 + dr_bce_fwd_bwd + dr_linear_bwd_*).
 * parts (1..3): see "in two halves" below. */
int64_t dr_tower_head_workspace_bytes(int64_t M);
int dr_tower_head_fwd_bwd(const float* x, int64_t ld_x, const float* W1, int64_t ld_w1, const float* b1,
                          int64_t M, int64_t n_total, int32_t K, int32_t H, int32_t act, const float* w2,
                          int64_t ld_w2, const float* b2, const float* extra_logit, const float* labels,
                          int32_t loss_mode, float scale, float* dst_w2, int64_t ld_dst_w2, float* dst_b2, float* h_out, int64_t ld_h,
                          float* prob, float* d_logit, float* d_h, int64_t ld_dh, float* loss_out, void* workspace,
                          int64_t workspace_bytes, int32_t parts, dr_stream_t stream);
/* The whole tower tail in ONE pass over x (round 5): dr_tower_head_fwd_bwd (act = relu) and dr_linear_bwd_narrow (relu_mask = 1) of the
 * SAME layer W1 [K, H] -- in the reference's towers the last hidden layer, Dense(H <= 32, relu), is at once the head's first factor and
 * the layer whose backward follows (keras/models/ranking/deepfm.py:30-34,41-47; estimator/models/feature_interaction/dnn.py:17-29):
 *   h = relu(x W1 + b1); logit = h w2 + b2 + extra_logit; prob, loss, d_logit = BCE(logit, labels, loss_mode) (mean over n_total, 0 = M);
 *   d_h = d_logit (x) w2 * (h > 0)  (written if d_h != NULL);   dx = (d_h W1^T) * (x > 0);
 *   dst_w1 += scale * x^T d_h;  dst_b1 += scale * colsum(d_h);  dst_w2 += scale * h^T d_logit;  dst_b2 += scale * sum(d_logit).
 * Both products use the pre-update W1 / w2 even when dst_* are the parameters themselves (scale = -lr: fused SGD); with gradient
 * buffers scale = 1.  parts = 1: the one-pass kernel (prob, d_logit, d_h, dx, per-block partials), 2: the two fixed-order reduces that
 * apply the partials (may run on another stream; must finish before the next part 1 over the same workspace), 3: both.  dx_amax (may
 * be NULL): receives max |dx| as float bits -- the f16x2 GEMMs' record of dx (parts = 3: stored by the reduce launch, no reset needed;
 * part 1 alone: reset and raised by the kernel, complete when part 1 is).  Deterministic.
 * Domain: H <= 32, K in {128, 256}, M a multiple of 32; anything else returns DR_ESHAPE (use the two calls it replaces).  Results equal those two calls' up to the summation order of the K-long dot products. */
int64_t dr_tower_tail_workspace_bytes(int64_t M, int32_t K);
int dr_tower_tail_fused(const float* x, int64_t ld_x, const float* W1, int64_t ld_w1, const float* b1, int64_t M, int64_t n_total,
                        int32_t K, int32_t H, const float* w2, int64_t ld_w2, const float* b2, const float* extra_logit,
                        const float* labels, int32_t loss_mode, float scale, float* dst_w1, int64_t ld_dst_w1, float* dst_b1,
                        float* dst_w2, int64_t ld_dst_w2, float* dst_b2, float* prob, float* d_logit, float* d_h, int64_t ld_dh,
                        float* dx, int64_t ld_dx, float* loss_out, void* workspace, int64_t workspace_bytes, int32_t parts,
                        uint32_t* dx_amax, dr_stream_t stream);

/* dr_linear_bwd_narrow / dr_tower_head_fwd_bwd in two halves (round 4): parts = 1 the main kernel (everything the rest of the step
 * reads: dx; prob, d_logit, d_h), parts = 2 the small reduce that applies the per-block partials to the weights (and writes the
 * loss), 3 = both (the whole call); any other value is DR_EINVAL.  Part 2 may run on ANOTHER stream -- the engine keeps the three
 * reduce kernels of a step off its training stream; it must finish before anything reads the updated weights and before the next
 * part 1 over the same workspace.
 * dx_amax of dr_linear_bwd_narrow (may be NULL): the call also leaves max |dx| as float bits in dx_amax[0] (reset and rebuilt by
 * part 1): the amax record of dx for the f16x2 GEMMs (dr_h2_linear_nt / dr_h2_wgrad_emb below). */

/* ------------------------------------------------------------------------------------------
 * K8  DCN cross layer (keras/models/ranking/dcn.py:70-88):
 *   prod = x @ W + b + diag_scale * x (:81,:85-86) ;  out = x0 * prod + x (:88)
 * One GEMM with the whole combine fused in the epilogue; `prod_out` (may be NULL) saves prod for
 * the backward.  W == NULL: "prod given" in prod_out (low-rank form :83 = two dr_linear_fwd calls,
 * then this with W NULL adds bias-free combine).  x0, x, out, prod share leading dimension ld.
 * bwd (elementwise part): d_prod = d_out * x0 ; d_x0 += d_out * prod ; d_x += d_out + diag_scale*d_prod;
 * the GEMM parts are dr_linear_bwd_dx(d_prod, W, accumulate=1 -> d_x) and dr_linear_bwd_dw(x, d_prod).
 * d_prod_amax (may be NULL): dr_cross_combine_bwd also leaves max |d_prod| as float bits in d_prod_amax[0] (reset first, also
 * when M == 0): the amax record of d_prod for the f16x2 GEMMs that take it as an operand (the cross layer's dgrad
 * and wgrad: dr_h2_linear_nt, dr_h2_wgrad).
 * ---------------------------------------------------------------------------------------- */
int dr_cross_fwd(const float* x0, const float* x, int64_t ld, const float* W, int64_t ld_w,
                 const float* b, float diag_scale, int64_t M, int32_t Dm, float* out,
                 float* prod_out, dr_stream_t stream);
int dr_cross_combine_bwd(const float* x0, const float* prod, const float* d_out, int64_t M,
                         int32_t Dm, int64_t ld, float diag_scale, float* d_prod, float* d_x0_accum,
                         float* d_x_accum, uint32_t* d_prod_amax, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K11  fused sigmoid + binary cross-entropy (+ gradient wrt the logit).
 * mode 0: tf.losses.sigmoid_cross_entropy(labels, logits)  (examples/train_fm_on_movielens_estimator.py:46)
 * mode 1: tf.losses.log_loss(labels, sigmoid(logits))      (examples/train_deepfm_on_movielens_estimator.py:47)
 * mode 2: tf.keras.losses.binary_crossentropy(labels, sigmoid(logits)) (examples/train_deepfm_on_movielens_keras.py:43)
 * logit[i] = logits[i] + logits_b[i*ld_b] (logits_b may be NULL): DeepFM's fm_outputs + dnn_outputs
 * (keras/models/ranking/deepfm.py:46) is summed here instead of in a separate pass.
 * prob[n] = sigmoid(logit) (may be NULL); d_logit[n] = d(mean loss)/d logit (may be NULL);
 * loss_out[1] = mean loss (deterministic two-stage reduction; workspace >= 1024 floats).
 * ---------------------------------------------------------------------------------------- */
int dr_bce_fwd_bwd(const float* logits, const float* logits_b, int64_t ld_b, const float* labels,
                   int64_t n, int32_t mode, float* prob, float* d_logit, float* loss_out,
                   float* workspace, dr_stream_t stream);
/* unfused forms for callers that hold probabilities (the reference models return sigmoid outputs:
 * keras/models/ranking/fm.py:64, deepfm.py:47; estimator/models/ranking/deepfm.py:43) */
int dr_sigmoid_fwd(const float* x, int64_t n, float* y, dr_stream_t stream);
int dr_sigmoid_bwd(const float* y, const float* dy, int64_t n, float* dx, dr_stream_t stream);
/* mode 1 = log_loss, mode 2 = keras binary_crossentropy, on probabilities; d_prob = d(mean loss)/dp */
int dr_bce_prob_fwd_bwd(const float* prob, const float* labels, int64_t n, int32_t mode, float* d_prob,
                        float* loss_out, float* workspace, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K9  in-batch sampled-softmax retrieval loss (Retrieval.call, keras/models/retrieval/sbcnm.py:120-151)
 *   scores = q @ c^T (:129); labels = eye (:134); optional -log(p_j) (:86), duplicate-id mask
 *   (+MIN_FLOAT = finfo(f32).min/100, :66-75), * 1/temperature (:148-149);
 *   loss = CCE(from_logits, reduction=SUM) = sum_i w_i * (logsumexp_j s_ij - s_ii)   (:100-102,151)
 * The B x B score matrix is never materialised in the forward: the MFMA GEMM's epilogue reduces each
 * 32-column group to (max, sum-exp) partials, a finalize pass combines them.
 *   row_lse[B], pos_score[B] (= s_ii) are outputs the backward reuses; loss_out[1].
 * Backward: dr_inbatch_softmax_grad_scores writes G = d_loss * w_i * (softmax_ij - delta_ij) / T into a
 *   caller-provided [B, ld_g] buffer; then dq = G @ c is dr_linear_fwd(G, c) and dc = G^T @ q is
 *   dr_linear_bwd_dw(G, q) — two plain GEMMs.  cand_prob / cand_ids / sample_weight may be NULL.
 * ---------------------------------------------------------------------------------------- */
int64_t dr_inbatch_softmax_workspace_bytes(int64_t B);
int dr_inbatch_softmax_fwd(const float* q, const float* c, int64_t B, int32_t D, const float* cand_prob,
                           const int64_t* cand_ids, const float* sample_weight, float inv_temperature,
                           float* row_lse, float* pos_score, float* loss_out, float* workspace,
                           int64_t workspace_bytes, dr_stream_t stream);
int dr_inbatch_softmax_grad_scores(const float* q, const float* c, int64_t B, int32_t D,
                                   const float* cand_prob, const int64_t* cand_ids,
                                   const float* sample_weight, float inv_temperature, const float* row_lse,
                                   float d_loss, float* G, int64_t ld_g, float* workspace,
                                   int64_t workspace_bytes, dr_stream_t stream);
/* Round 5: in the f16x2 operand split (dr_get_gemm_split) both score passes run on the register-split kernel with the LSE /
 * softmax-gradient epilogues (three fp16 products per fp32 product, scores never leave the tile) whenever D % 4 == 0, D <= 512,
 * B >= 256 and the workspace (256-byte aligned, dr_inbatch_softmax_workspace_bytes) is there: it also holds the candidates' two fp16
 * planes and both amax records.  dr_inbatch_softmax_grad_scores with workspace NULL / workspace_bytes 0 (or too small) stays on
 * the fp32 kernel; the forward's workspace may be reused (its contents are not needed). */

/* ------------------------------------------------------------------------------------------
 * K10  exact top-K maximum-inner-product search (BruteForce.call factorized_top_k.py:316-334,
 * Streaming.call :178-260): scores = q @ cand^T, k largest per query, descending, ties -> lower candidate
 * index first ([TF] tf.math.top_k).  The [Bq, N] score matrix is never materialised: candidates are scored
 * in chunks (dr_scores_nt into `workspace`) and folded into a running sorted list per query
 * (dr_topk_select).  k <= 128.  out_scores[Bq,k] fp32, out_index[Bq,k] int64 (candidate position +
 * index_base, -1 = empty slot).  init = 1 starts a new search, init = 0 continues one (Streaming's
 * per-batch map + reduce, :201-233).  Returns DR_ESHAPE if init && k > N (the reference's
 * "input must have at least k columns", :13-23).
 * A CONTINUED search (init = 0) must be handed its batches with non-decreasing index_base, as Streaming does (its counter-based row
 * ids, :244-254): the chunk GEMM's filter epilogue keeps a candidate only if its score is strictly above the row's current k-th
 * best, so a candidate that TIES that score wins its lower-index tie only against entries of LATER batches -- with index_base going
 * backwards an equal-score, lower-index candidate could be dropped or kept depending on where a chunk boundary falls.
 * dr_topk_merge: merge two sorted lists per row, list a wins ties (Streaming's reduce; cross-rank merge).
 * ---------------------------------------------------------------------------------------- */
int dr_scores_nt(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t M, int32_t N, int32_t D,
                 float* out, int64_t ld_out, dr_stream_t stream);
int dr_topk_select(const float* scores, int64_t ld, int64_t Bq, int64_t n, int32_t k, int64_t index_base,
                   int32_t init, float* out_scores, int64_t* out_index, dr_stream_t stream);
int64_t dr_topk_workspace_bytes(int64_t Bq, int64_t N, int32_t k);
int dr_topk_mips(const float* q, int64_t Bq, const float* cand, int64_t N, int32_t D, int32_t k,
                 int64_t index_base, int32_t init, float* out_scores, int64_t* out_index,
                 float* workspace, int64_t workspace_bytes, dr_stream_t stream);
/* The corpus side of an index (BruteForce.index factorized_top_k.py:275-297 / Streaming's candidates: candidates are handed over ONCE,
 * queries arrive many times).  dr_topk_index_build derives, once, what the f16x2 scan of dr_topk_mips derives from the corpus on
 * every call -- its amax record and the two fp16 planes of cand * 2^k -- into `index` (256-byte aligned, dr_topk_index_bytes(N, D)
 * bytes; D a multiple of 4, <= 512).  dr_topk_mips_indexed(q, ..., cand, index, ...) is dr_topk_mips with that work skipped: same
 * arguments, same result bit for bit (the planes and the record are the ones the call would have made); `cand` must still be the
 * corpus the index was built from -- the scan reads it instead of the index whenever it does not run in the f16x2 split
 * (dr_get_gemm_split) or falls back to the generic kernel.  The index must be rebuilt when the corpus changes. */
int64_t dr_topk_index_bytes(int64_t N, int32_t D);
int dr_topk_index_build(const float* cand, int64_t N, int32_t D, void* index, int64_t index_bytes, dr_stream_t stream);
int dr_topk_mips_indexed(const float* q, int64_t Bq, const float* cand, const void* index, int64_t N, int32_t D, int32_t k,
                         int64_t index_base, int32_t init, float* out_scores, int64_t* out_index,
                         float* workspace, int64_t workspace_bytes, dr_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * SURVEY.md section 8f rank 4 -- IVF-Flat approximate top-K, the GPU counterpart of the reference's `Faiss` index
 * (keras/models/retrieval/factorized_top_k.py:337-461: faiss.IndexIVFFlat(faiss.IndexFlatIP(d), d, nlist,
 * faiss.METRIC_INNER_PRODUCT), `searcher.nprobe = nprobe`, `searcher.search(queries, k)`).
 *   dr_ivf_pack: builds the index storage.  `order` = candidate numbers grouped by list (list l = order[list_start[l] ..
 *                list_start[l+1])), `blk_off[l]` = first 64-vector block of list l (lists padded to whole blocks),
 *                packed[(blk*D + d)*64 + lane] = component d of the vector in slot (blk, lane), packed_ids its identifier
 *                (ids[src] or src; -1 in padding slots).
 *   dr_ivf_scan: probes[q, 0..nprobe) = lists to scan for query q (any negative entry is skipped); exact inner products
 *                over those lists, top k (score descending, ties by identifier ascending); slots that find fewer than k
 *                vectors keep score -inf / index -1 (faiss returns -1 labels there too).
 * ---------------------------------------------------------------------------------------- */
/* dr_ivf_build_lists (round 4): the grouping half of `index.add` (factorized_top_k.py:374-391) -- a STABLE counting sort of the N
 * vectors by their coarse assignment: order[list_start[l] .. list_start[l+1]) = the vectors of list l in input order (so equal scores
 * tie on the lower candidate number, as in the exact search); an assignment outside [0, nlist) drops its vector.  nlist <= 8192;
 * workspace >= dr_ivf_build_workspace_bytes(N, nlist).  Integer, bit-exact. */
int64_t dr_ivf_build_workspace_bytes(int64_t N, int32_t nlist);
int dr_ivf_build_lists(const int64_t* assign, int64_t N, int32_t nlist, int64_t* order, int64_t* list_start, void* workspace,
                       int64_t workspace_bytes, dr_stream_t stream);
int dr_ivf_pack(const float* cand, int64_t N, int32_t D, const int64_t* order, const int64_t* list_start,
                const int64_t* blk_off, int32_t nlist, int64_t total_blocks, const int64_t* ids, float* packed,
                int64_t* packed_ids, dr_stream_t stream);
int dr_ivf_scan(const float* q, int64_t Bq, int32_t D, const int64_t* probes, int32_t nprobe,
                const int64_t* blk_off, const float* packed, const int64_t* packed_ids, int32_t k,
                float* out_scores, int64_t* out_index, dr_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * IVF-PQ (csrc/ivf_pq.hip): the index EBR serves from (Huang et al., KDD 2020, section 4) -- IVF lists of product-quantised
 * residuals, inner product.  256 codewords per sub-quantiser, m sub-quantisers, dsub = D / m.
 * Domain of all three: m % 4 == 0, 4 <= m <= 64, D % m == 0, D / m <= 64, D <= 1024, 1 <= k <= 128, nprobe >= 1, kin <= 128.
 *   dr_pq_encode:   codes_out[i, j / 4] bits 8 * (j % 4) = the codeword of codebooks[j] ([m, 256, dsub]) nearest to sub-vector j of
 *                   x[i] - centroids[assign[i]] (squared L2 summed over ascending d in fp32, no fused multiply-add; ties to the
 *                   lower code).  assign and centroids both NULL: x is the residual already (the assignment step of codebook
 *                   training).  An assign outside [0, nlist) encodes as zeros.
 *   dr_ivfpq_scan:  packed_codes[(blk * (m/4) + w) * 64 + lane] = word w of the vector in slot (blk, lane) of dr_ivf_pack's layout,
 *                   packed_rows its candidate row (-1: padding).  score = probe_scores[q, p] + sum_j LUT[j][code_j] added in
 *                   ascending j, LUT[j][c] = fmaf chain of q_j . codebooks[j][c] over ascending d from 0 (built in LDS per query).
 *                   Top k by score descending, ties to the lower row; a probe < 0 is skipped; fewer than k members leave
 *                   (-inf, -1).  Bit-identical from run to run and independent of the batch.
 *   dr_rerank_topk: exact fp32 inner products of q[b] with cand[rows[b, t]] (rows < 0 or >= N: none), top k with the row numbers,
 *                   score descending, ties to the lower row.
 * ---------------------------------------------------------------------------------------- */
int dr_pq_encode(const float* x, const int64_t* assign, const float* centroids, int32_t nlist, const float* codebooks,
                 int64_t N, int32_t D, int32_t m, uint32_t* codes_out, dr_stream_t stream);
int dr_ivfpq_scan(const float* q, const int64_t* probes, const float* probe_scores, const int64_t* blk_off,
                  const uint32_t* packed_codes, const int64_t* packed_rows, const float* codebooks, int64_t Bq,
                  int32_t D, int32_t m, int32_t nprobe, int32_t k, float* out_scores, int64_t* out_rows,
                  dr_stream_t stream);
int dr_rerank_topk(const float* q, const float* cand, const int64_t* rows, int64_t Bq, int64_t N, int32_t D, int32_t kin,
                   int32_t k, float* out_scores, int64_t* out_rows, dr_stream_t stream);
int dr_topk_merge(const float* sa, const int64_t* ia, int32_t ka, const float* sb, const int64_t* ib,
                  int32_t kb, int64_t Bq, int32_t k, float* out_scores, int64_t* out_index,
                  dr_stream_t stream);
/* small retrieval ops: positive scores sum(q*c, axis=1) (factorized_top_k.py:494-495); identifier gather
 * (:334); _take_long_axis (:26-41) / _gather_elements_along_row (sbcnm.py:15-30); _exclude's penalty
 * (:57-62); FactorizedTopK's in_top_k counting (:499-512, [TF] B14); and the sbcnm helper layers on explicit
 * logits: out = logits - log(p_j) (:86) + (dup_ij - labels_ij) * MIN_FLOAT (:66-75) + labels_ij * scale (:44) */
int dr_rowdot(const float* a, const float* b, int64_t B, int32_t D, float* out, dr_stream_t stream);
/* out[r, :] = x[r, :] * f(s[r]) for contiguous [M, D] matrices -- the row scalings of the `Faiss` index (factorized_top_k.py:370-371,
 * 450-451: faiss.normalize_L2; :372: index.train's centroid update).  mode 0: f = s.  mode 1: f = 1 / sqrt(s), rows with s == 0 unchanged
 * (s = dr_rowdot(x, x): L2 normalisation that leaves zero rows alone).  mode 2: f = 1 / s, rows with s == 0 taken from `fallback`
 * [M, D] (centroid = member sum / member count; an empty cluster keeps its previous centroid).  out may alias x. */
int dr_rows_scale(const float* x, const float* s, int32_t mode, const float* fallback, int64_t M, int32_t D, float* out,
                  dr_stream_t stream);
int dr_gather_i64(const int64_t* src, int64_t nsrc, const int64_t* idx, int64_t n, int64_t* out,
                  dr_stream_t stream);
int dr_take_along_rows_f32(const float* arr, int64_t ld, int64_t B, int32_t C, const int64_t* idx, int32_t K,
                           float* out, dr_stream_t stream);
int dr_take_along_rows_i64(const int64_t* arr, int64_t ld, int64_t B, int32_t C, const int64_t* idx,
                           int32_t K, int64_t* out, dr_stream_t stream);
int dr_topk_hits(const float* pos, const float* topk, int64_t B, int32_t K, const int32_t* ks, int32_t nk,
                 uint64_t* hits, dr_stream_t stream);
int dr_exclude_adjust(const float* scores, const int64_t* ids, int64_t B, int32_t K, const int64_t* exclude,
                      int32_t E, float* adjusted, dr_stream_t stream);
int dr_logits_adjust(const float* logits, const float* labels, int64_t B, int32_t C, const float* cand_prob,
                     const int64_t* cand_ids, float add_label_scale, float* out, dr_stream_t stream);
/* CCE(from_logits=True, reduction=SUM) on an explicit [B, C] logits / labels pair (the hard-negative branch,
 * sbcnm.py:145-151): row_loss[B] scratch, loss_out[1] = sum_i w_i * (lse_i * sum_j y_ij - sum_j y_ij s_ij / T).
 * B = 0 is an empty batch as for every other entry point: DR_OK, loss_out[0] = 0, nothing else touched (the backward: nothing written). */
int dr_softmax_ce_rows(const float* logits, const float* labels, int64_t B, int32_t C, float inv_temperature,
                       const float* sample_weight, float* row_loss, float* loss_out, dr_stream_t stream);

/* Backward of dr_softmax_ce_rows: g[r][j] = w_r * inv_temperature * d_loss * (sum_j(labels) * softmax_j - labels[r][j]).
 * cols == NULL: out is [B, >= C] dense.  cols [B, C] (the columns HardNegativeMining kept, sbcnm.py:41-49 of the reference):
 * the gradient is scattered to out[r][cols[r][j]] of a pre-zeroed [B, ld_out] score-gradient matrix, from which
 * dq = G c and dc = G^T q follow as in the default path. */
int dr_softmax_ce_rows_bwd(const float* logits, const float* labels, int64_t B, int32_t C,
                           float inv_temperature, const float* sample_weight, float d_loss,
                           const int64_t* cols, float* out, int64_t ld_out, dr_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * Row-sharded tables over N ranks (new design — the reference is single-process; the
 * exchange mirrors no reference code).  owner(id) = id % world; on the owner, field f's shard holds
 * rows_per_shard rows and id lives at local row f*rows_per_shard + id / world.
 *
 * dr_shard_bucket_ids: stable counting sort of the n = B*C (example, column) slots by owner:
 *   counts[world]   slots routed to each rank (device int64; the all-to-all split sizes)
 *   send_rows[n]    owner-local row of every slot, grouped by owner (missing ids travel as -1)
 *   pos[n]          position of slot p = b*C + c inside send_rows (the inverse map: rows come back from
 *                   the all-to-all in send order, so K3 over `pos` as ids re-assembles example order)
 *   workspace       dr_shard_bucket_workspace_bytes(n, world) bytes.  world <= 16.  Integer, bit-exact.
 * dr_rows_gather / dr_rows_scatter_add: owner side of the forward / backward exchange (packed [n, D]
 *   rows + first-order weights); scatter accumulates with fp32 atomics (dst += scale * grad).
 * dr_axpy: y += alpha * x, applies an all-reduced dense gradient.
 * ---------------------------------------------------------------------------------------- */
int64_t dr_shard_bucket_workspace_bytes(int64_t n, int32_t world);
/* Requester-side de-duplication of the exchange (round 4): what [TF] safe_embedding_lookup_sparse's `unique` does inside the lookup
 * reached from keras/models/ranking/fm.py:57-61 -- a row that several slots of a micro-batch look up travels once each way.
 * dr_shard_dedup_slots: rep[p] = the lowest slot looking up the same row as slot p (p itself for an unshared row or a missing id), from
 *   the slot plan of the micro-batch's ids (dr_emb_sort_slots over the global rows row_base[f] + id, with the same num_rows).
 * dr_shard_bucket_ids with rep given (may be NULL: every slot gets a send slot): only the representatives get a send slot (counts
 *   sum to the number of distinct rows) and pos[p] = pos[rep[p]] for every other slot.  Integer, bit-exact. */
int dr_shard_dedup_slots(const int64_t* sorted_rows, const int32_t* sorted_slots, const int32_t* dup_count, int64_t n,
                         int64_t num_rows, int64_t* rep, dr_stream_t stream);
int dr_shard_bucket_ids(const int64_t* ids, const int64_t* rep, int64_t n, int32_t C, int64_t rows_per_shard,
                        int32_t world, int64_t* counts, int64_t* send_rows, int64_t* pos, int64_t* workspace,
                        dr_stream_t stream);
int dr_rows_gather(const int64_t* rows, int64_t n, const float* table, int32_t D, const float* lin_w,
                   float* out_rows, float* out_lin, dr_stream_t stream);
int dr_rows_scatter_add(const int64_t* rows, int64_t n, const float* grads, int32_t D,
                        const float* lin_grads, float scale, float* table, float* lin_w,
                        dr_stream_t stream);
int dr_axpy(int64_t n, float alpha, const float* x, float* y, dr_stream_t stream);
/* requesting-rank half of the backward exchange: per-slot gradient rows written straight into the all-to-all send
 * layout (pos is a permutation, every destination is written exactly once):
 *   out_rows[pos[b,f],:] = d_concat[b, f*D:(f+1)*D] + d_fm_logit[b] * (sum_x[b,:] - concat[b, f*D:(f+1)*D]) ;
 *   out_lin[pos[b,f]] = d_fm_logit[b] ;  bias_sum[0] += sum_b d_fm_logit[b].
 *   concat / sum_x / d_fm_logit / out_lin / bias_sum may be NULL.
 * unique_flags (may be NULL) selects the form for a de-duplicated exchange: pos maps the slots of a shared row to ONE destination;
 * unique_flags [B * F] (the slot plan's flags of the micro-batch) says which slots own their row -- those store, the others ADD with
 * fp32 atomics (their order is not fixed).  out_rows / out_lin must then be zero-filled by the caller. */
int dr_emb_pack_grads(const int64_t* pos, const uint8_t* unique_flags, int64_t B, int32_t F, int32_t D, const float* d_concat,
                      int64_t ld_dconcat, const float* concat, int64_t ld_concat, const float* sum_x,
                      const float* d_fm_logit, float* out_rows, float* out_lin, float* bias_sum, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * K7p  first (wide) tower layer on PRE-SPLIT operands -- the "planes" form of the bf16x3 product mode.
 * Replaces the same reference ops as dr_linear_fwd / _bwd_dx / _bwd_dw (keras/models/ranking/deepfm.py:30-34,
 * estimator/models/feature_interaction/dnn.py:17-29 and their autodiff) for the one layer whose operands are large:
 * the producers of x (K3, dr_emb_pool_fwd_planes), of dy (dr_linear_bwd_narrow / dr_linear_bwd_dx with planes_out) and of W
 * (dr_bf3_split after each update) write every fp32 value v as three bf16 planes v0 + v1 + v2 (v0 = bf16(v),
 * v1 = bf16(v - v0), v2 = bf16(v - v0 - v1): exact, (v2 + v1) + v0 == v), so the GEMM stages tiles with LDS-DMA and does no
 * conversion work.  Results equal the bf16x3 mode of dr_linear_*: fp32 operands, six bf16 products per fp32 product,
 * fp32 accumulation.
 * Operand format: planes[p][row][col], p = 0..2, bf16; `ld` elements per row (multiple of 8), `plane_stride` elements
 * between planes (multiple of 8), base 16-byte aligned.
 *   dr_bf3_split    fp32 [R, C] -> planes (transpose = 1 writes planes[p][row_offset + c][col_offset + r])
 *   dr_bf3_join     planes -> fp32 (exact inverse; tests)
 *   dr_bf3_gemm_nt  C[m, n] = act(sum_k A[m, k] B[n, k] + bias[n]) (then zeroed where mask[m, n] <= 0);  K = padded
 *                   reduction length (multiple of 32), columns [true K, K) of BOTH operands' planes must be zero.
 *                   forward: A = x planes, B = W^T planes;  dgrad: A = dy planes, B = W planes.
 *   dr_bf3_gemm_tn  dst[f, n] += scale * sum_r X[r, f] Y[r, n];  dstb[n] += scale * y_colsum[n]  (split over r into
 *                   `workspace`, fixed-order reduce: deterministic).  Rows [R, roundup(R, 32)) of both operands' planes must
 *                   exist and be zero.  wgrad: X = x planes, Y = dy planes.
 * ---------------------------------------------------------------------------------------- */
int dr_bf3_split(const float* src, int64_t ld_src, int64_t R, int32_t C, void* planes, int64_t plane_stride,
                 int64_t ld_planes, int64_t row_offset, int64_t col_offset, int32_t transpose,
                 dr_stream_t stream);
int dr_bf3_join(const void* planes, int64_t plane_stride, int64_t ld_planes, int64_t R, int32_t C, float* dst,
                int64_t ld_dst, dr_stream_t stream);
int dr_bf3_gemm_nt(const void* a_planes, int64_t a_plane_stride, int64_t a_ld, const void* b_planes,
                   int64_t b_plane_stride, int64_t b_ld, int64_t M, int32_t N, int32_t K, const float* bias,
                   int32_t act, const float* mask, int64_t ld_mask, float* C, int64_t ldc, dr_stream_t stream);
/* dr_bf3_linear_nt: the same product with the ACTIVATION operand left in fp32 -- C[m, n] (+)= act(sum_k A[m, k] B[n, k] + bias[n])
 * (zeroed where mask[m, n] <= 0), A fp32 [M, K] row-major (lda % 4 == 0, 16-byte aligned), B planes [3][N][b_ld] with
 * b_ld >= roundup(K, 32) and columns [K, roundup(K, 32)) zero.  Each wave loads its 32 rows of A from HBM straight into
 * registers and splits them there; only B (the weights: W^T planes for the forward, W planes for the dgrad) is staged through
 * the LDS.  This is the form the engines use: activations and their producers are untouched, the weights' planes are refreshed
 * by dr_bf3_split after each update. */
int dr_bf3_linear_nt(const float* A, int64_t lda, const void* b_planes, int64_t b_plane_stride, int64_t b_ld, int64_t M,
                     int32_t N, int32_t K, const float* bias, int32_t act, const float* mask, int64_t ld_mask,
                     int32_t accumulate, float* C, int64_t ldc, dr_stream_t stream);
/* The sharded engine's first-layer dgrad and dr_emb_pack_grads in ONE launch (round 3): the gradient of slot (m, f) of F 64-wide
 * embeddings -- sum_k dy[m][k] W[64 f + d][k] + d_fm_logit[m] (sum_x[m][d] - x[m][64 f + d]) -- is written straight to
 * out_rows[pos[m, f], d], the all-to-all send layout (autodiff of keras/models/ranking/deepfm.py:44-45 + fm.py:23-37 of the
 * reference into the gradient exchange); d_concat never exists.  w_planes: W as planes [3][N rows][b_ld] (N = input features
 * >= 64 F; columns behind the embeddings are dropped).  out_lin (may be NULL)[pos[m, f]] = d_fm_logit[m]; bias_sum (may be NULL)
 * += sum_m d_fm_logit[m] in a fixed order; sum_x == NULL: no FM term.  pos: a permutation of the M F slots. */
int dr_bf3_linear_nt_pack(const float* dy, int64_t ld_dy, const void* w_planes, int64_t plane_stride, int64_t b_ld, int64_t M,
                          int32_t N, int32_t K, const int64_t* pos, int32_t F, const float* d_fm_logit, const float* sum_x,
                          const float* x, int64_t ld_x, float* out_rows, float* out_lin, float* bias_sum, dr_stream_t stream);
/* The same in the f16x2 operand mode (round 5): dy with its amax record, W as two fp16 planes (dr_h2_split) with theirs.  The epilogue
 * stages each 32 x 32 accumulator block through the LDS and moves float4s with 8 lanes per row: a row's 32 columns of a field are one
 * 128-byte line of its destination row and of the x row it reads.  x, sum_x (both required), out_rows 16-byte aligned, ld_x % 4 == 0.
 * Domain: M a multiple of 256 and M * F < 2^25; outside it DR_ESHAPE (the caller runs dr_h2_linear_nt + dr_emb_pack_grads). */
int dr_h2_linear_nt_pack(const float* dy, int64_t ld_dy, const uint32_t* dy_amax, const void* w_planes, int64_t plane_stride,
                         int64_t b_ld, const uint32_t* w_amax, int64_t M, int32_t N, int32_t K, const int64_t* pos, int32_t F,
                         const float* d_fm_logit, const float* sum_x, const float* x, int64_t ld_x, float* out_rows,
                         float* out_lin, float* bias_sum, dr_stream_t stream);
/* DCN cross layer forward (dr_cross_fwd's math, keras/models/ranking/dcn.py:81-88) on pre-split weights: wt_planes = W^T as
 * planes [3][Dm][ld_planes] (dr_bf3_split with transpose = 1).  x0, x, out, prod_out share leading dimension ld. */
int dr_bf3_cross_fwd(const float* x0, const float* x, int64_t ld, const void* wt_planes, int64_t plane_stride,
                     int64_t ld_planes, const float* b, float diag_scale, int64_t M, int32_t Dm, float* out,
                     float* prod_out, dr_stream_t stream);
/* dr_bf3_wgrad: dstW[f, n] += scale * sum_r x[r, f] dy[r, n];  dstb[n] += scale * sum_r dy[r, n] (dstb may be NULL) -- the wgrad of
 * a wide layer on its fp32 activations as they are (x [R, F], dy [R, N] row-major): x goes from HBM straight into registers
 * (lane index along f), dy is split once per 256 x-columns into a two-stage LDS image; bf16x3 product mode; split over r into
 * `workspace` (dr_bf3_wgrad_workspace_bytes) with a fixed-order reduce: deterministic. */
/* dr_bf3_emb_linear_fwd: K3 and the first Dense layer in ONE launch -- the register-split GEMM gathers its activation operand
 * straight from the embedding tables: k-tile kt of example m is dims 32 (kt & 1) .. + 31 of row row_base[f] + ids[m, f], f = kt / 2
 * (single-valued fields, D == 64, at most 32 dense features, no field longer than field_rows_max <= 2^24 rows -- the kernel
 * addresses a field as one buffer with 32-bit offsets; anything else returns DR_ESHAPE and the caller uses dr_emb_pool_fwd +
 * dr_bf3_linear_nt).
 * Replaces, together: the F DenseFeatures lookups + tf.stack / tf.concat + the first-order Dense(1) + FM.call
 * (keras/models/ranking/fm.py:23-37,47-64, deepfm.py:36-45) AND deepfm.py:30-34's first Dense(u, relu).
 *   in : ids [M, F] (-1 = missing), table [R, 64] (R < 2^31), lin_w [R] / lin_bias [1] (may be NULL), dense_pad [M, 32] = the
 *        K - 64 F dense features of every example, zero-padded to 32 (NULL iff K == 64 F), W^T planes [3][N][ld_planes]
 *        (columns [K, roundup(K, 32)) zero), bias [N]
 *   out: concat[:, 0 : 64 F) (for the backward kernels; the caller places the dense features in concat[:, 64 F : K) itself),
 *        sum_x [M, 64], fm_logit [M] (as dr_emb_pool_fwd), out [M, N] = act(x W + bias), x = [embeddings, dense features];
 *        lin_vals_t [F, M] field-major (may be NULL): the first-order weight of every slot as it was read, lin_vals_t[f * M + m] =
 *        lin_w[row_base[f] + ids[m, f]] (undefined for a missing id; ignored when lin_w == NULL).  Handed to dr_emb_pool_bwd_sorted
 *        as `lin_old_t`, it turns the first-order update of a row that is unique in the batch into ONE write. */
int dr_bf3_emb_linear_fwd(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                          const float* table, int32_t D, const float* lin_w, const float* lin_bias, const float* dense_pad, float* concat,
                          int64_t ld_concat, int32_t K, const void* wt_planes, int64_t plane_stride, int64_t ld_planes, int32_t N,
                          const float* bias, int32_t act, float* sum_x, float* fm_logit, float* out, int64_t ld_out,
                          float* lin_vals_t, dr_stream_t stream);
int64_t dr_bf3_wgrad_workspace_bytes(int64_t R, int32_t F, int32_t N);
int dr_bf3_wgrad(const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t R, int32_t F, int32_t N,
                 float scale, float* dstW, int64_t ld_w, float* dstb, void* workspace, int64_t workspace_bytes,
                 dr_stream_t stream);
/* dr_bf3_wgrad for the FIRST tower layer, x = concat(field embeddings, dense features) gathered from the tables instead of read from
 * a buffer (D = 64; F = in_dim in [64 nf, 64 nf + 32]): ids_t [nf][R] int32 field-major ids (dr_ids_transpose_i32, -1 = missing),
 * dense_pad [R, 32] zero-padded dense features (NULL iff F == 64 nf).  Same workspace as dr_bf3_wgrad(R, F, N).  Every field
 * must have fewer than 2^24 - 1 rows (ids index a 4 GB raw buffer per field; -1 falls outside it and reads as zero).
 * Autodiff of the first Dense of keras/models/ranking/deepfm.py:30-34 w.r.t. its kernel, with deepfm.py:44-45's concat never built.
 * In two halves like dr_linear_bwd_narrow: parts = 1 the split-K GEMM into the workspace, 2 the fixed-order reduce that applies it to
 * dstW / dstb, 3 = both; any other value is DR_EINVAL. */
int dr_bf3_wgrad_emb(const int32_t* ids_t, int64_t R, int32_t nf, const int64_t* row_base, const float* table, int32_t D,
                     const float* dense_pad, const float* dy, int64_t ld_dy, int32_t F, int32_t N, float scale, float* dstW,
                     int64_t ld_w, float* dstb, void* workspace, int64_t workspace_bytes, int32_t parts, dr_stream_t stream);
int64_t dr_bf3_gemm_tn_workspace_bytes(int64_t R, int32_t F, int32_t N);
int dr_bf3_gemm_tn(const void* x_planes, int64_t x_plane_stride, int64_t x_ld, const void* y_planes,
                   int64_t y_plane_stride, int64_t y_ld, int64_t R, int32_t F, int32_t N, float scale, float* dst,
                   int64_t ld_dst, const float* y_colsum, float* dstb, void* workspace, int64_t workspace_bytes,
                   dr_stream_t stream);

/* ---- "f16x2" operand mode of the first tower layer's three GEMMs (round 4) ---------------------------------------------------------
 * The same products as dr_bf3_emb_linear_fwd / dr_bf3_linear_nt / dr_bf3_wgrad(_emb) (keras/models/ranking/deepfm.py:30-34 of the
 * reference and its autodiff; fp32 in, fp32 accumulate, fp32 out) with every operand value carried as TWO fp16 terms of x * s (22
 * significant bits) and a product formed from THREE matrix instructions instead of the bf16x3 mode's six.  s is a power of two per
 * TENSOR, derived inside the kernels from the tensor's `amax record`: one uint32 in device memory holding max |x| as float bits (or an
 * upper bound of it).  Records are written by dr_h2_amax or maintained by the tensor's producer (dr_emb_pool_bwd_sorted and
 * dr_emb_pool_bwd_sorted_adam keep the table's as a running maximum); a record that is too SMALL by a factor of 4 or more
 * saturates values instead of producing inf (still wrong: keep it an upper bound).  Accuracy: tests/test_gpu_h2_gemm.py.
 * Errors as the bf3 calls, plus DR_EINVAL for a missing record. */
int dr_h2_amax(const float* src, int64_t ld, int64_t R, int32_t C, uint32_t* amax, int32_t reset, dr_stream_t stream);
/* two fp16 planes of src * s(amax), laid out like dr_bf3_split's three (same arguments) */
int dr_h2_split(const float* src, int64_t ld_src, int64_t R, int32_t C, void* planes, int64_t plane_stride, int64_t ld_planes,
                int64_t row_offset, int64_t col_offset, int32_t transpose, const uint32_t* amax, dr_stream_t stream);
/* A weight's record and BOTH of its plane images in two launches (round 5): what dr_h2_amax(reset = 1) + dr_h2_split +
 * dr_h2_split(transpose = 1) produce -- same record, same planes -- without the 4-byte memset and the atomic pass (four small launches on
 * the serial chain between a wgrad and the next forward).  W [K, N] with row stride ldw; w_planes [2][K][w_ld], wt_planes [2][N][wt_ld];
 * parts: 256 uint32 of scratch. */
int dr_h2_refresh_weight(const float* W, int64_t ldw, int64_t K, int32_t N, void* w_planes, int64_t w_plane_stride, int64_t w_ld,
                         void* wt_planes, int64_t wt_plane_stride, int64_t wt_ld, uint32_t* amax, uint32_t* parts, dr_stream_t stream);
int dr_h2_linear_nt(const float* A, int64_t lda, const uint32_t* a_amax, const void* b_planes, int64_t b_plane_stride, int64_t b_ld,
                    const uint32_t* b_amax, int64_t M, int32_t N, int32_t K, const float* bias, int32_t act, const float* mask,
                    int64_t ld_mask, int32_t accumulate, float* C, int64_t ldc, uint32_t* c_amax, dr_stream_t stream);
/* c_amax / out_amax (may be NULL): reset, then raised to max |value stored into C / out| -- the record of the NEXT GEMM's operand */
/* Round 6 -- the first-layer dgrad of the DeepFM tower with K4's unique-row pass as its epilogue (csrc/h2_occ.hip; D = 64, single-valued
 * fields, SGD):  dx[m, 64 f + d] = sum_k dy[m][k] W[64 f + d][k] is the gradient row of slot (m, f).  For every slot whose table row no other
 * slot of the batch shares (unique_flags [M, F] of dr_emb_sort_slots; ids_t [F, M] int32 from dr_ids_transpose_i32, -1 = missing) the
 * kernel applies K4's update on the spot --  g = dx + d_fm_logit[m] (sum_x[m] - x), table[row] = x + scale g with x the row as it stands,
 * lin_w[row] = lin_old_t[f, m] + scale d_fm_logit[m]  -- operation for operation what dr_emb_pool_bwd_sorted does with the stored
 * gradient (bit-identical tables); the other slots' dx goes to d_concat [M, ld_dconcat] for the duplicate pass.  Follow with
 * dr_emb_pool_bwd_sorted(parts | 8) on the same stream (grad = d_concat): rows shared by several slots, hot rows, first-order
 * bias.  The tables must not be read by anything that needs their pre-step value after this call (run the first-layer wgrad that
 * gathers x BEFORE it).  w_planes: two fp16 planes [2][>= 64 F rows][w_ld] of the layer's kernel (dr_h2_split / dr_h2_refresh_weight's
 * `w`), w_ld >= roundup(K, 32); lin_w / lin_old_t both NULL or both given; table_amax (may be NULL): the table's running record, raised
 * to every value written.  Autodiff of keras/models/ranking/deepfm.py:30-34,44-45 and fm.py:23-37 w.r.t. the embedding tables. */
int dr_h2_dgrad_emb_sgd(const float* dy, int64_t ld_dy, const uint32_t* dy_amax, const void* w_planes, int64_t w_plane_stride,
                        int64_t w_ld, const uint32_t* w_amax, int64_t M, int32_t F, int32_t K, const int32_t* ids_t,
                        const uint8_t* unique_flags, const int64_t* row_base, float* table, float* lin_w, const float* lin_old_t,
                        const float* sum_x, const float* d_fm_logit, float scale, float* d_concat, int64_t ld_dconcat,
                        uint32_t* table_amax, dr_stream_t stream);
int dr_h2_cross_fwd(const float* x0, const float* x, int64_t ld, const uint32_t* x_amax, const void* wt_planes, int64_t plane_stride,
                    int64_t ld_planes, const uint32_t* w_amax, const float* b, float diag_scale, int64_t M, int32_t Dm, float* out,
                    float* prod_out, uint32_t* out_amax, dr_stream_t stream);
/* dense_amax: the record of dense_pad, required iff K > 64 F; lin_vals_t may be NULL */
int dr_h2_emb_linear_fwd(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max, const float* table,
                         int32_t D, const uint32_t* table_amax, const float* lin_w, const float* lin_bias, const float* dense_pad,
                         const uint32_t* dense_amax, float* concat, int64_t ld_concat, int32_t K, const void* wt_planes,
                         int64_t plane_stride, int64_t ld_planes, const uint32_t* w_amax, int32_t N, const float* bias, int32_t act,
                         float* sum_x, float* fm_logit, float* out, int64_t ld_out, float* lin_vals_t, dr_stream_t stream);
/* dr_h2_emb_linear_fwd followed by dr_tower_tail_fused (extra_logit = fm_logit, n_total = M) on its output h0, as ONE kernel plus the
 * tail's reduce: the tail runs as the forward GEMM's epilogue, on the accumulators.  `out` (h0) may be NULL: it is then never written.
 * prob, d_logit, d_h (may be NULL), dx = d h0 [M, N] and the record dx_amax (may be NULL; parts == 3: stored by the reduce, parts == 1:
 * reset in front of the kernel and raised by it, parts == 2: ignored) are the bits the two calls give; dst_* += scale * gradient and loss_out are the same fixed-order fp32 sums, grouped by this kernel's blocks (one per 256
 * rows).  parts: 1 = the kernel, 2 = the reduce (dr_tower_tail_fused's), 3 = both.
 * Domain: N == 256, H <= 32, M a positive multiple of 32, and dr_h2_emb_linear_fwd's (D == 64, K <= 64 F + 32, field_rows_max <= 2^24);
 * outside it: DR_ESHAPE, nothing launched. */
int64_t dr_h2_emb_linear_tail_fwd_workspace_bytes(int64_t M);
int dr_h2_emb_linear_tail_fwd(const int64_t* ids, int64_t M, int32_t F, const int64_t* row_base, int64_t field_rows_max,
                              const float* table, int32_t D, const uint32_t* table_amax, const float* lin_w, const float* lin_bias,
                              const float* dense_pad, const uint32_t* dense_amax, float* concat, int64_t ld_concat, int32_t K,
                              const void* wt_planes, int64_t plane_stride, int64_t ld_planes, const uint32_t* w_amax, int32_t N,
                              const float* bias, int32_t act, float* sum_x, float* fm_logit, float* out, int64_t ld_out,
                              float* lin_vals_t, const float* W1, int64_t ld_w1, const float* b1, int32_t H, const float* w2,
                              int64_t ld_w2, const float* b2, const float* labels, int32_t loss_mode, float scale, float* dst_w1,
                              int64_t ld_dst_w1, float* dst_b1, float* dst_w2, int64_t ld_dst_w2, float* dst_b2, float* prob,
                              float* d_logit, float* d_h, int64_t ld_dh, float* dx, int64_t ld_dx, float* loss_out, void* workspace,
                              int64_t workspace_bytes, int32_t parts, uint32_t* dx_amax, dr_stream_t stream);
int dr_h2_wgrad(const float* x, int64_t ld_x, const uint32_t* x_amax, const float* dy, int64_t ld_dy, const uint32_t* dy_amax, int64_t R,
                int32_t F, int32_t N, float scale, float* dstW, int64_t ld_w, float* dstb, void* workspace, int64_t workspace_bytes,
                dr_stream_t stream);
int dr_h2_wgrad_emb(const int32_t* ids_t, int64_t R, int32_t nf, const int64_t* row_base, const float* table, int32_t D,
                    const uint32_t* table_amax, const float* dense_pad, const uint32_t* dense_amax, const float* dy, int64_t ld_dy,
                    const uint32_t* dy_amax, int32_t F, int32_t N, float scale, float* dstW, int64_t ld_w, float* dstb, void* workspace,
                    int64_t workspace_bytes, int32_t parts, dr_stream_t stream);
/* dr_emb_pool_bwd_dups_apply = dr_emb_pool_bwd_sorted(parts = 1 | 8 or 3 | 8) whose first launch carries extra "rider" blocks behind the
 * duplicate pass's own: ordinary independent blocks (no launch, stream, event or grid-wide wait of their own) that run part 2 of the
 * wgrad (wg_R, wg_F, wg_N) whose part 1 left its product in wg_workspace earlier on this stream: dstW += wg_scale * sum of the
 * partials, dstb likewise (may be NULL), bit for bit.  wg_h2 != 0: the product came from an f16x2 call (dr_h2_wgrad_emb / dr_h2_wgrad);
 * the scales are taken from the amax words that call saved in the workspace, never from the live records.  DR_EINVAL for a null or
 * short wg_workspace before anything is launched. */
int dr_emb_pool_bwd_dups_apply(const int64_t* ids, const int64_t* row_base, const int64_t* sorted_rows, const int32_t* sorted_slots,
                               const uint8_t* unique_flags, const int32_t* dup_heads, const int32_t* dup_count, int64_t B, int32_t F,
                               int32_t D, int64_t num_rows, const float* grad, int64_t ld_grad, const float* sum_x,
                               const float* d_fm_logit, float scale, float* dst_table, float* dst_lin, float* dst_bias, float* x_sorted,
                               const float* lin_old_t, int32_t parts, uint32_t* table_amax, void* wg_workspace,
                               int64_t wg_workspace_bytes, int64_t wg_R, int32_t wg_F, int32_t wg_N, int32_t wg_h2, float wg_scale,
                               float* dstW, int64_t ld_w, float* dstb, dr_stream_t stream);
/* dr_emb_pool_bwd_dups_apply with the f16x2 plane refresh of the weight it steps riding along, without a launch or a stream of its own:
 * the riders of part 1 also store max |dstW value written| in amax_parts (one uint32 per rider, <= 1024, plain stores); part 2 -- the hot
 * rows' launch -- carries rider blocks that reduce the words of that launch, store the record w_amax and write both plane images of dstW
 * [wg_F, wg_N] (w_planes [2][wg_F][w_ld], wt_planes [2][wg_N][wt_ld]): what dr_h2_refresh_weight(dstW, ...) behind the call gives, bit for
 * bit.  Stream order makes dstW and the words final for part 2: no hand-off inside a launch.  parts: 9, 10 (part 2 alone, behind a call
 * with 9 on the same stream) or 11; part 2 is launched for its riders even when no hot row exists.  w_planes == NULL: no refresh (parts 9
 * or 11), dr_emb_pool_bwd_dups_apply itself.  amax_parts: 1024 uint32 of scratch. */
int dr_emb_pool_bwd_dups_apply_refresh(const int64_t* ids, const int64_t* row_base, const int64_t* sorted_rows,
                                       const int32_t* sorted_slots, const uint8_t* unique_flags, const int32_t* dup_heads,
                                       const int32_t* dup_count, int64_t B, int32_t F, int32_t D, int64_t num_rows, const float* grad,
                                       int64_t ld_grad, const float* sum_x, const float* d_fm_logit, float scale, float* dst_table,
                                       float* dst_lin, float* dst_bias, float* x_sorted, const float* lin_old_t, int32_t parts,
                                       uint32_t* table_amax, void* wg_workspace, int64_t wg_workspace_bytes, int64_t wg_R, int32_t wg_F,
                                       int32_t wg_N, int32_t wg_h2, float wg_scale, float* dstW, int64_t ld_w, float* dstb,
                                       void* w_planes, int64_t w_plane_stride, int64_t w_ld, void* wt_planes, int64_t wt_plane_stride,
                                       int64_t wt_ld, uint32_t* w_amax, uint32_t* amax_parts, dr_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * CIN  Compressed Interaction Network layer of xDeepFM (keras/models/ranking/xdeepfm.py:71-96):
 *   out[b, f, d] = act( sum_{i,j} W[i * Hk + j, f] * x0[b, i, d] * x[b, j, d] + bias[f] )
 * x0 [B, H0, D], x [B, Hk, D], W [H0 * Hk, Fm] (the conv1d kernel [1, H0 * Hk, Fm] of :55-61), out [B, Fm, D], all fp32
 * contiguous.  act: 0 none, 1 relu, 2 sigmoid (the layer's default), 3 tanh.  One MFMA GEMM whose left operand (the
 * outer product :80-86) is formed on the fly from LDS.  DR_ESHAPE when (H0 + Hk) * 65 floats exceed the 160 KB LDS.
 * dr_cin_bwd: autodiff of the above -- d_x0, d_x, dW [H0 * Hk, Fm], dbias [Fm] (may be NULL) from d_out and the saved out.
 * ---------------------------------------------------------------------------------------- */
int dr_cin_fwd(const float* x0, const float* x, int64_t B, int32_t H0, int32_t Hk, int32_t D, const float* W,
               int32_t Fm, const float* bias, int32_t act, float* out, dr_stream_t stream);
int dr_cin_bwd(const float* x0, const float* x, int64_t B, int32_t H0, int32_t Hk, int32_t D, const float* W,
               int32_t Fm, int32_t act, const float* out, const float* d_out, float* d_x0, float* d_x, float* dW,
               float* dbias, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CIN with its sum pooling, for stacks (xDeepFM's CINNetwork), csrc/cin_pool.hip.  Same tensors and act codes as above.
 *   dr_cin_pool_fwd   out [B, Fm, D] as dr_cin_fwd and pooled[b, f] = sum_d out[b, f, d] ([B, Fm]) in one launch.  A block owns whole
 *                     examples, so pooled is summed in a fixed order (no atomics) and no example's result depends on its neighbours.
 *                     out or pooled may be NULL (then it is not written); both NULL is DR_EINVAL.
 *                     DR_ESHAPE when (H0 + Hk + 64) * 65 floats exceed the 160 KB LDS.
 *   dr_cin_pool_bwd   with g = (d_out + d_pooled[:, :, None]) * act'(out): d_x0 [B, H0, D], d_x [B, Hk, D], dW [H0 * Hk, Fm] and
 *                     dbias [Fm] (may be NULL), all three products on the fp32-input MFMA; bit-reproducible (no float atomics).
 *                     d_out or d_pooled may be NULL (contributes zero; both NULL is DR_EINVAL); out may be NULL only for act 0.
 *                     accumulate_x0 != 0: the gradient is ADDED to what d_x0 holds (every layer of a stack feeds the same x0).
 *                     workspace: 16-byte aligned, at least dr_cin_pool_bwd_workspace_bytes(B, H0, Hk, D, Fm) bytes
 *                       = 4 * (H0 * ceil(Hk / 32) * ceil(Fm / 8) * 256  [W packed for the MFMA's A operand]
 *                              + chunks * (H0 * Hk * Fm + Fm))          [per-chunk partials of dW and dbias, added in chunk order]
 *                     where the B * D rows are split into `chunks` <= 64 runs of whole 64-row tiles.
 *                     DR_ESHAPE when (8 * ceil(Fm / 8) + 3 * H0 + 32 * ceil(Hk / 32)) * 65 floats exceed the 160 KB LDS.
 *   Both: DR_EINVAL for a NULL required pointer, a negative or zero size, act outside 0..3 or a short workspace; B == 0 is DR_OK and
 *   launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_cin_pool_fwd(const float* x0, const float* x, int64_t B, int32_t H0, int32_t Hk, int32_t D, const float* W, int32_t Fm,
                    const float* bias, int32_t act, float* out, float* pooled, dr_stream_t stream);
int64_t dr_cin_pool_bwd_workspace_bytes(int64_t B, int32_t H0, int32_t Hk, int32_t D, int32_t Fm);
int dr_cin_pool_bwd(const float* x0, const float* x, int64_t B, int32_t H0, int32_t Hk, int32_t D, const float* W, int32_t Fm,
                    int32_t act, const float* out, const float* d_out, const float* d_pooled, float* d_x0, int32_t accumulate_x0,
                    float* d_x, float* dW, float* dbias, void* ws, int64_t ws_bytes, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DLRM's pairwise dot interaction (Naumov et al. 2019; the reference's README lists DLRM among the models it plans and ships no code
 * for it), csrc/dot_interact.hip.  Per example, T [N, D] = the row dense[b] (when dense != NULL) followed by the F rows of
 * emb[b] ([F * D], field-major: the slab's concat, read in place); N = F + (dense != NULL), c0 = dense != NULL ? D : 0.
 *   dr_dot_interact_fwd   out[b, 0:c0] = dense[b];  the row-major lower triangle of T T^T after it:
 *                           self_interaction 0: out[b, c0 + i (i - 1) / 2 + j] = <t_i, t_j>, 0 <= j <  i < N   (P = N (N - 1) / 2)
 *                           self_interaction 1: out[b, c0 + i (i + 1) / 2 + j] = <t_i, t_j>, 0 <= j <= i < N   (P = N (N + 1) / 2)
 *                         and zeros in columns [c0 + P, ld_out); nothing is written beyond ld_out.
 *   dr_dot_interact_bwd   with G the lower-triangular matrix of d_out's triangle and S = G + G^T (the diagonal doubled):
 *                         dT = S T, dT_0 += d_out[b, 0:D];  d_dense [B, D] = dT_0, d_emb [B, F * D] = the other rows.  Reads the first
 *                         c0 + P columns of d_out only; overwrites D columns of d_dense and F * D columns of d_emb, nothing else.
 *   Products on the fp32-input MFMA (an fmaf chain in a fixed order); one wave owns one example: no atomics, bit-reproducible, an
 *   example's bits do not depend on its batch; the [B, N, N] matrix is never written.  One launch each, no workspace.
 *   Domain: D % 4 == 0, 4 <= D <= 256, 2 <= N <= 64, self_interaction 0 or 1, every ld a multiple of 4 and at least the width it covers
 *   (ld_dense, ld_ddense >= D; ld_emb, ld_demb >= F * D; ld_out, ld_dout >= c0 + P), dense, emb, d_dense and d_emb 16-byte aligned,
 *   d_dense given exactly when dense is.  Anything else is DR_EINVAL.  B == 0 is DR_OK and launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_dot_interact_fwd(const float* dense, int64_t ld_dense, const float* emb, int64_t ld_emb, int64_t B, int32_t F, int32_t D,
                        int32_t self_interaction, float* out, int64_t ld_out, dr_stream_t stream);
int dr_dot_interact_bwd(const float* dense, int64_t ld_dense, const float* emb, int64_t ld_emb, const float* d_out, int64_t ld_dout,
                        int64_t B, int32_t F, int32_t D, int32_t self_interaction, float* d_dense, int64_t ld_ddense, float* d_emb,
                        int64_t ld_demb, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * AFM's attention pooling over field pairs (Xiao et al., IJCAI 2017; the reference's README lists AFM among its ranking models and
 * ships no code for it), csrc/afm_pool.hip.  All fp32.  emb[b] holds the F rows e_0 .. e_{F-1} of example b ([F * D], field-major: the
 * slab's concat, read in place at the pitch ld_emb); W [D, A], b [A], h [A] dense.  Pairs are numbered q = i (i - 1) / 2 + j for
 * 0 <= j < i < F (the order of dr_dot_interact_fwd without the diagonal), P = F (F - 1) / 2.
 *   dr_afm_pool_fwd   p_q = e_i * e_j [D];  z_q = p_q W + b [A];  s_q = sum_a max(z_qa, 0) h_a;  a = softmax over q of s;
 *                     out[b, 0:D] = sum_q a_q p_q;  lse[b] = log sum_q exp(s_q);  attn[b, q] = a_q when attn != NULL (ld_attn >= P).
 *                     One launch; a wave owns an example, the softmax is online over tiles of 16 pairs; p, z and s are never written
 *                     (s passes through attn when that is given).  Writes D columns of out and P of attn, nothing else.
 *   dr_afm_pool_bwd   from g = d_out [B, D], with out and lse of the forward (z is recomputed):
 *                       ds_q = a_q (<g, p_q> - <g, out>);  dz_q = ds_q h * [z_q > 0]  (the derivative of max(z, 0) at 0 is 0)
 *                       dh = sum_b sum_q ds_q max(z_q, 0);  db = sum_b sum_q dz_q;  dW = sum_b sum_q p_q^T dz_q
 *                       dp_q = a_q g + dz_q W^T;  d_emb[b, i] = sum_{j != i} dp_(ij) * e_j     (F * D columns of d_emb are overwritten)
 *                     dW [D, A], db [A], dh [A] are overwritten.  Two launches: the main kernel and the sum of its per-block partials.
 *                     workspace: 16-byte aligned, at least dr_afm_pool_bwd_workspace_bytes(B, F, D, A) bytes
 *                       = 4 * blocks * (D * A + 2 * A),  blocks = min(ceil(B / waves), 512)
 *                     [one partial of dW, db and dh per block, added in block order], with `waves` as below.  It does not grow with
 *                     B * P.  dr_afm_pool_bwd_workspace_bytes returns DR_EINVAL / DR_ESHAPE (negative) outside the domain.
 *   The three products (z, dz W^T, p^T dz) run on the fp32-input MFMA; every sum has one owner and a fixed order: no float atomics in
 *   memory or LDS, results bit-identical from run to run, and out, lse, attn and d_emb of an example do not depend on its batch.
 *   Domain: D % 4 == 0, 4 <= D <= 256, 1 <= A <= 128, 2 <= F <= 64, ld_emb, ld_demb >= F * D, ld_out, ld_dout >= D, all four multiples of
 *   4, emb, out, d_out, d_emb and the workspace 16-byte aligned; anything else, a NULL required pointer or a short workspace is DR_EINVAL.
 *   NARROWER THAN D <= 256 AND A <= 128 TOGETHER: with DT = ceil(D / 16) and AT = ceil(A / 16), each rounded up to a power of two,
 *     DT * AT <= 32    (a wave keeps dW in 4 DT AT accumulator registers per lane; D 256 goes with A <= 32, D 128 with A <= 64,
 *                       D <= 64 with A <= 128), and
 *     16 DT (16 AT + 4) + 32 AT + 16 ceil(P / 16) + waves * (2 F (16 DT + 4) + 16 DT + 16 (16 AT + 4) + 16 (16 DT + 4)) <= 40000
 *                      floats of LDS for waves = 4, else 2, else 1 (the first that fits is the block's number of waves),
 *   else DR_ESHAPE, from all three entry points alike.  B == 0 is DR_OK and launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_afm_pool_fwd(const float* emb, int64_t ld_emb, const float* W, const float* b, const float* h, int64_t B, int32_t F, int32_t D,
                    int32_t A, float* out, int64_t ld_out, float* lse, float* attn, int64_t ld_attn, dr_stream_t stream);
int64_t dr_afm_pool_bwd_workspace_bytes(int64_t B, int32_t F, int32_t D, int32_t A);
int dr_afm_pool_bwd(const float* emb, int64_t ld_emb, const float* W, const float* b, const float* h, const float* out, int64_t ld_out,
                    const float* lse, const float* d_out, int64_t ld_dout, int64_t B, int32_t F, int32_t D, int32_t A, float* d_emb,
                    int64_t ld_demb, float* dW, float* db, float* dh, void* ws, int64_t ws_bytes, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DIEN's recurrences (Zhou et al., AAAI 2019; the reference's README lists DIEN after DIN and ships no code for it), csrc/dien.hip.
 * All fp32.  xp [B, T, 3H] holds the input-side pre-activations x_t W + b (the dense path's product over all B * T rows), gate columns
 * [u | r | c]; row (b, t) starts at xp + (b * T + t) * ld_xp, and hs, d_hs, d_xp are addressed the same way with their own ld.
 * U [H, 3H], h0 / h_last / d_h_last / d_h0 [B, H], att / d_att / a / d_a [B, T] and q / d_q [B, H] are dense.  lengths [B] int32,
 * 0 <= len <= T (values outside are clamped); NULL = all T.  h0 NULL = zeros.  att NULL = a plain GRU, else AUGRU.
 *   dr_gru_seq_fwd    for t < len[b]:  g = h_{t-1} U;  u = sigmoid(xp_u + g_u);  r = sigmoid(xp_r + g_r);  c = tanh(xp_c + r * g_c);
 *                       u' = att[b, t] u  (u' = u without att);  h_t = (1 - u') h_{t-1} + u' c;  hs[b, t] = h_t
 *                     for t >= len[b]: h_t = h_{t-1}, hs[b, t] = 0, and xp[b, t], att[b, t] are not read (NaN there reaches nothing).
 *                     h_last[b] = h_{len - 1} (h0, or zeros, when len == 0).  Keras's / PyTorch's update gate is z = 1 - u.
 *                     One launch: a block owns 16 examples and runs the time loop; its waves hold their column slices of U in
 *                     registers for all T steps, h crosses between waves through a 16 x H LDS tile with one barrier per step.
 *   dr_gru_seq_bwd    from d_hs [B, T, H] and d_h_last [B, H] (either may be NULL = zeros; d_hs at masked steps is ignored), with the
 *                     forward's hs; t runs downward and g, u, r, c are recomputed:
 *                       dh += d_hs[b, t];  dc = dh u';  du' = dh (c - h_{t-1});  dh_prev = dh (1 - u');  d_att[b, t] = sum_j du'_j u_j
 *                       du = att du';  dpc = dc (1 - c^2);  dpu = du u (1 - u);  dpr = dpc g_c r (1 - r)
 *                       d_xp[b, t] = [dpu | dpr | dpc];  dg = [dpu | dpr | dpc r];  dh_prev += dg U^T;  dU += h_{t-1}^T dg
 *                     d_xp (3H columns per row), dU [H, 3H], d_h0 and d_att are overwritten; d_h0 and d_att may be NULL.  d_xp and
 *                     d_att are exactly 0 at masked steps; for len == 0, d_h0[b] = d_h_last[b].
 *                     workspace: 16-byte aligned, at least dr_gru_seq_bwd_workspace_bytes(B, T, H) bytes
 *                       = 4 * B * (T + 1) * 3H  +  max(dr_linear_bwd_dw_workspace_bytes(B * T, H, 3H),
 *                                                      dr_linear_bwd_dw_workspace_bytes(B, H, 3H)) rounded up to 16
 *                     [dg of every step: the rows t = 0 first, then the rows t >= 1 shifted by one with a zero last row, so that row
 *                     (b, s) pairs with hs[b, s]; dU is then dr_linear_bwd_dw(hs, dg) plus dr_linear_bwd_dw(h0, dg rows 0) with that
 *                     call's deterministic reduce, in the GEMM mode of dr_set_gemm_mode].  0 for B == 0; DR_EINVAL / DR_ESHAPE
 *                     (negative) outside the domain.
 *   dr_seq_attn_fwd   a[b, t] = softmax over t < len[b] of <hs[b, t], q[b]>; 0 for t >= len[b] (a whole row of zeros when len == 0);
 *                     masked rows of hs are not read.  One wave per example.
 *   dr_seq_attn_bwd   ds_t = a_t (d_a_t - sum_t' a_t' d_a_t');  d_hs[b, t] = ds_t q[b] (H columns per row, 0 at masked steps);
 *                     d_q[b] = sum_t ds_t hs[b, t].  Both overwritten.  No workspace.
 *   The recurrent products run on the fp32-input MFMA (v_mfma_f32_16x16x4_f32); every sum has one owner and a fixed order: no float
 *   atomics in memory or LDS, results bit-identical from run to run, and hs, h_last, d_xp, d_h0, d_att, a, d_hs, d_q of an example do
 *   not depend on its batch.  Nothing of size B * T * 3H is written except d_xp and dg.
 *   Domain (all five alike): H % 4 == 0, 4 <= H <= 128, T >= 1, B >= 0, B * T <= 2^40; every ld a multiple of 4 and at least the width
 *   it covers (3H for xp and d_xp, H for hs and d_hs); xp, hs, d_hs, d_xp, h0, q and the workspace 16-byte aligned (the other
 *   arrays need only their 4 bytes).  H > 128 or B * T > 2^40 is DR_ESHAPE; anything else, a NULL required pointer or a short workspace is
 *   DR_EINVAL.  B == 0 is DR_OK and launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_gru_seq_fwd(const float* xp, int64_t ld_xp, const float* U, const float* h0, const int32_t* lengths, const float* att, int64_t B,
                   int32_t T, int32_t H, float* hs, int64_t ld_hs, float* h_last, dr_stream_t stream);
int64_t dr_gru_seq_bwd_workspace_bytes(int64_t B, int32_t T, int32_t H);
int dr_gru_seq_bwd(const float* xp, int64_t ld_xp, const float* U, const float* h0, const int32_t* lengths, const float* att,
                   const float* hs, int64_t ld_hs, int64_t B, int32_t T, int32_t H, const float* d_hs, int64_t ld_dhs,
                   const float* d_h_last, float* d_xp, int64_t ld_dxp, float* dU, float* d_h0, float* d_att, void* ws, int64_t ws_bytes,
                   dr_stream_t stream);
int dr_seq_attn_fwd(const float* hs, int64_t ld_hs, const float* q, const int32_t* lengths, int64_t B, int32_t T, int32_t H, float* a,
                    dr_stream_t stream);
int dr_seq_attn_bwd(const float* hs, int64_t ld_hs, const float* q, const int32_t* lengths, const float* a, const float* d_a, int64_t B,
                    int32_t T, int32_t H, float* d_hs, int64_t ld_dhs, float* d_q, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * FFM's field-aware interaction (Juan et al., RecSys 2016; the reference's README lists FFM among its ranking models and ships no code
 * for it), csrc/ffm.hip.  All fp32.  The table row of a feature of field i is F * k wide: block j of it, row[j * k : (j + 1) * k], is
 * that feature's factor towards field j.  Example b therefore owns A [F, F, k], A[i, j, :] = block j of field i's row.
 *   inter[b]            = sum_{i = 1 .. F-1} sum_{j < i} sum_c A[i, j, c] * A[j, i, c]
 *   d_rows[b, i, j, :]  = d_inter[b] * A[j, i, :] for j != i (one fp32 multiply per element, no sum);  d_rows[b, i, i, :] = +0.0
 *   The diagonal blocks A[i, i, :] take no part and are never read (NaN there reaches nothing).
 *   dr_ffm_fwd / dr_ffm_bwd          rows [B, F * F * k] at the pitch ld_rows: the slab's concat over columns of dimension F * k, read
 *                                    in place (multi-valued fields, or a caller that already holds the rows).  d_rows at the pitch ld_d:
 *                                    F * F * k columns are overwritten, nothing beyond them.
 *   dr_ffm_gather_fwd / _gather_bwd  single-valued fields, ids [B, F]: row i of example b is table + (row_base[i] + ids[b, i]) * F * k,
 *                                    read straight from the table and never written anywhere.  An id < 0 is a row of zeros (as K3).
 *                                    first_order[b] = lin_bias[0] + sum_f lin_w[row_base[f] + ids[b, f]], added in field order (missing
 *                                    ids skipped), is written when first_order and lin_w are both given; lin_bias NULL counts as 0.
 *                                    lin_w, lin_bias and first_order may be NULL.  d_rows [B, F * F * k] is what dr_emb_pool_bwd takes
 *                                    as d_concat (with D = F * k) to update or differentiate the table.
 *   A group of lanes (a wave from F = 12 up) owns an example and adds its products in an order that depends on (F, k) alone: no atomics,
 *   no workspace, no LDS; results are bit-identical from run to run and an example's bits depend neither on its batch nor on its place
 *   in it.  The gather entry points run the same arithmetic in the same order as the rows entry points: on K3's concat of single-valued
 *   fields inter and d_rows agree bit for bit.  One launch each.
 *   Domain: k % 4 == 0, 4 <= k <= 128, 2 <= F <= 64, F * k <= 256, ld_rows and ld_d multiples of 4 and >= F * F * k, rows, d_rows and
 *   table 16-byte aligned; anything else or a NULL required pointer is DR_EINVAL.  B == 0 is DR_OK and launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_ffm_fwd(const float* rows, int64_t ld_rows, int64_t B, int32_t F, int32_t k, float* inter, dr_stream_t stream);
int dr_ffm_bwd(const float* rows, int64_t ld_rows, const float* d_inter, int64_t B, int32_t F, int32_t k, float* d_rows, int64_t ld_d,
               dr_stream_t stream);
int dr_ffm_gather_fwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table, int32_t k,
                      const float* lin_w, const float* lin_bias, float* inter, float* first_order, dr_stream_t stream);
int dr_ffm_gather_bwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table, int32_t k,
                      const float* d_inter, float* d_rows, int64_t ld_d, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * NFM's Bi-Interaction pooling (He & Chua, SIGIR 2017; the reference's README lists NFM among its ranking models and ships no code for
 * it), csrc/bi_interaction.hip.  All fp32.  e_f = field f's row (D floats), s = sum_f e_f, q = sum_f e_f * e_f (elementwise):
 *   out[b, :]        = 0.5 * (s * s - q)             the vector K3 sums over d into fm_logit and never writes
 *   d_rows[b, f, :]  = d_out[b, :] * (s - e_f)       s is recomputed in the backward; nothing is saved between the two
 *   dr_bi_interact_fwd / _bwd                rows [B, F * D] at the pitch ld_rows: the slab's concat, read in place (multi-valued
 *                                            fields that K3 has pooled, or a caller that already holds the rows).  out [B, D] at the
 *                                            pitch ld_out, d_out at ld_do, d_rows [B, F * D] at ld_d: exactly D (F * D) columns are
 *                                            written, nothing beyond them.
 *   dr_bi_interact_gather_fwd / _gather_bwd  single-valued fields, ids [B, F]: row f of example b is table + (row_base[f] +
 *                                            ids[b, f]) * D, read straight from the table and never written anywhere.  An id < 0 is a
 *                                            row of zeros and is never dereferenced.  first_order[b] = lin_bias[0] + sum_f
 *                                            lin_w[row_base[f] + ids[b, f]], added in field order (missing ids skipped), is written
 *                                            when first_order and lin_w are both given; lin_bias NULL counts as 0.  lin_w, lin_bias
 *                                            and first_order may be NULL.  d_rows [B, F * D] is what dr_emb_pool_bwd takes as
 *                                            d_concat; for a missing slot the formula with e = 0 is written, K4 never applies it.
 *   A group of D / 4 lanes owns an example, lane l the float4 at column 4 l of s and q; the fields are added in ascending order, so
 *   the order is a function of (F, D) alone: no atomics, no workspace, no LDS, no cross-lane arithmetic.  Results are bit-identical
 *   from run to run and an example's bits depend neither on its batch nor on its place in it.  The gather entry points run the same
 *   arithmetic in the same order as the rows entry points: on K3's concat of single-valued fields out and d_rows agree bit for bit.
 *   s * s and q are rounded separately before the difference: F = 1 gives exactly +0.0.  One launch each.
 *   Domain: D % 4 == 0 and 4 <= D <= 256 (else DR_ESHAPE); 1 <= F <= 1024, every ld a multiple of 4 and >= its width, rows, table,
 *   out, d_out and d_rows 16-byte aligned, required pointers non-NULL (else DR_EINVAL).  B == 0 is DR_OK and launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_bi_interact_fwd(const float* rows, int64_t ld_rows, int64_t B, int32_t F, int32_t D, float* out, int64_t ld_out,
                       dr_stream_t stream);
int dr_bi_interact_bwd(const float* rows, int64_t ld_rows, const float* d_out, int64_t ld_do, int64_t B, int32_t F, int32_t D,
                       float* d_rows, int64_t ld_d, dr_stream_t stream);
int dr_bi_interact_gather_fwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table, int32_t D,
                              const float* lin_w, const float* lin_bias, float* out, int64_t ld_out, float* first_order,
                              dr_stream_t stream);
int dr_bi_interact_gather_bwd(const int64_t* ids, int64_t B, int32_t F, const int64_t* row_base, const float* table, int32_t D,
                              const float* d_out, int64_t ld_do, float* d_rows, int64_t ld_d, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * LS-PLM, the large-scale piece-wise linear model (Gai et al., Alibaba 2017; listed in the reference's README, no code there),
 * csrc/lsplm.hip.  All fp32.  A table row is W = 2 m floats: the first m are the gate u, the last m the expert w.
 *   z[b, :]  = bias[:] + sum_f mean over the valid ids of field f's bag of table[row_base[f] + id, :]
 *              K3's pooling (ids [B, C], col_start [F + 1], or col_start NULL and C == F for single-valued fields; ids < 0 are
 *              dropped, an empty bag adds nothing), so dr_emb_pool_bwd with D = W is its exact transpose.
 *   pi = softmax(z[:m]) with the max subtracted;  sg_i = sigmoid(z[m + i]);  sn_i = sigmoid(-z[m + i])
 *   p = sum_i pi_i sg_i;   q = sum_i pi_i sn_i  (1 - p, computed without the subtraction: sg and sn share one exponential)
 *   dr_lsplm_fwd       z (optional, [B, W] at ld_z), p [B], q [B].
 *   dr_lsplm_bwd       from the stored z and d_p [B]: d_z[b] = d_p[b] * [pi_i (sg_i - p) ; pi_i sg_i sn_i] ([B, W] at ld_dz) and d_rows
 *                      [B, F * W] at ld_d = F copies of d_z[b], bit for bit: dr_emb_pool_bwd's d_concat (K4 divides by the bag count
 *                      itself).  Either of d_z, d_rows may be NULL, not both.
 *   dr_lsplm_loss_fwd  the one-pass training form: p, q, loss[b] = -wt_b (y log p + (1 - y) log q) (loss may be NULL), and d_z / d_rows
 *                      = the gradient of row_scale * loss[b], i.e. dr_lsplm_bwd's with d_p = (row_scale * wt_b) * c, c = -y / p +
 *                      (1 - y) / q.  A term whose coefficient y or 1 - y is exactly 0 is not evaluated (no 0 * inf); inside the log
 *                      and the quotient p and q are floored at 1e-30.  sample_weight NULL: wt = 1.  p, q, d_z and d_rows carry the
 *                      same bits as dr_lsplm_fwd followed by dr_lsplm_bwd on that d_p.
 *   dr_lsplm_bias_grad d_bias[c] = sum_b d_z[b, c] (overwritten), rows summed in ascending order inside at most 256 chunks and the
 *                      chunks in order (dr_sum_partials.h): no float atomics, bit-identical from run to run.  workspace: at least
 *                      dr_lsplm_bias_grad_workspace_bytes(B, m) bytes.  B == 0 writes +0.0.
 *   A power-of-two group of at least m / 2 lanes owns an example; lane l holds the columns 2 l, 2 l + 1 of the gate and of the expert.
 *   The m-way max and sums are fixed-order xor butterflies inside the group.  No LDS, no atomics; fields in ascending order, a bag in
 *   column order: bit-identical from run to run, and an example's bits depend neither on its batch nor on its place in it.
 *   Domain: m even and 2 <= m <= 128 (else DR_ESHAPE); 1 <= F <= 1024, C >= F (C == F without col_start), every ld a multiple of 4 and
 *   >= its width, table, bias, z, d_z and d_rows 16-byte aligned, required pointers non-NULL (else DR_EINVAL).  B == 0 is DR_OK and
 *   launches nothing (dr_lsplm_bias_grad excepted).
 * ---------------------------------------------------------------------------------------- */
int dr_lsplm_fwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start, const int64_t* row_base,
                 const float* table, int32_t m, const float* bias, float* z, int64_t ld_z, float* p, float* q, dr_stream_t stream);
int dr_lsplm_bwd(const float* z, int64_t ld_z, const float* d_p, int64_t B, int32_t F, int32_t m, float* d_z, int64_t ld_dz,
                 float* d_rows, int64_t ld_d, dr_stream_t stream);
int dr_lsplm_loss_fwd(const int64_t* ids, int64_t B, int32_t F, int32_t C, const int32_t* col_start, const int64_t* row_base,
                      const float* table, int32_t m, const float* bias, const float* labels, const float* sample_weight,
                      float row_scale, float* p, float* q, float* loss, float* d_z, int64_t ld_dz, float* d_rows, int64_t ld_d,
                      dr_stream_t stream);
int64_t dr_lsplm_bias_grad_workspace_bytes(int64_t B, int32_t m);
int dr_lsplm_bias_grad(const float* d_z, int64_t ld_dz, int64_t B, int32_t m, float* d_bias, void* workspace,
                       int64_t workspace_bytes, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Skip-gram with negative sampling (Mikolov et al., NIPS 2013): the training step of Word2Vec, Item2Vec and DeepWalk, which the
 * reference's README lists and ships no code for; csrc/sgns.hip.  All fp32.  in_table [R_in, D] and out_table [R_out, D] dense.
 * Example b: c = centers[b], o_0 = contexts[b], o_1 .. o_K = negatives[b, :] ([B, K] dense int64), u = in_table[c], v_j = out_table[o_j],
 * z_j = 1 for j = 0 and 0 otherwise, w_b = sample_weight[b] (1 when sample_weight is NULL).
 *   s_j    = <u, v_j>
 *   loss_b = w_b * sum_j softplus((1 - 2 z_j) s_j),   softplus(x) = max(x, 0) + log1p(exp(-|x|))
 *   g_j    = w_b * (sigmoid(s_j) - z_j)
 *   Skipped: the whole example when c < 0 or o_0 < 0; a negative with o_j < 0; with flags & DR_SGNS_SKIP_EQUAL a negative with
 *   o_j == o_0 (the rule of word2vec.c).  A skipped slot has s_j = g_j = 0, adds nothing to loss_b (a skipped example's is 0) and its id
 *   is never turned into an address that is read: any int64 may stand there.
 *   dr_sgns_fwd   writes loss_rows [B], coeff [B, 1 + K] (the g_j) and, unless NULL, scores [B, 1 + K] (the s_j), all dense.  With
 *                 d_center and d_ctx given (both or neither) the same pass also writes the gradient rows of row_scale * loss_b:
 *                   c_j = row_scale * g_j;  d_ctx[b, j, :] = c_j * u  (+0.0 for a skipped slot);  d_center[b, :] = sum_j c_j * v_j,
 *                 j ascending, one fused multiply-add per term.  d_center [B, D] at the pitch ld_dc, d_ctx [B, (1 + K) * D] at the
 *                 pitch ld_dx (D resp. (1 + K) * D columns are overwritten, nothing beyond them; both pitches are ignored without
 *                 the buffers).  This is the training path: every row is read once.
 *   dr_sgns_bwd   the same two buffers from coeff and a per-example d_loss [B]: c_j = d_loss[b] * g_j, the rows re-gathered, the same
 *                 operations in the same order -- with d_loss[b] == row_scale both entry points write the same bits.
 *   d_center with ids [B, 1] and d_ctx with ids [B, 1 + K] are what the K4 entry points (atomic or sorted form) take as d_concat to
 *   update or differentiate in_table and out_table; a skipped slot with an id >= 0 adds its row of zeros.
 *   A group of D / 4 lanes, rounded up to a power of two, owns an example; u stays in registers, four rows v_j are in flight per
 *   lane.  No atomics, no LDS, no workspace, one launch: results are bit-identical from run to run and an example's bits depend
 *   neither on its batch nor on its place in it.
 *   Domain: D % 4 == 0, 4 <= D <= 256, 0 <= K <= 63 (negatives may be NULL when K == 0), flags 0 or DR_SGNS_SKIP_EQUAL, both tables and
 *   both gradient buffers 16-byte aligned, ld_dc and ld_dx multiples of 4 and >= the width they cover; anything else or a NULL
 *   required pointer is DR_EINVAL.  B == 0 is DR_OK and launches nothing.
 * ---------------------------------------------------------------------------------------- */
#define DR_SGNS_SKIP_EQUAL 1
int dr_sgns_fwd(const float* in_table, const float* out_table, int32_t D, const int64_t* centers, const int64_t* contexts,
                const int64_t* negatives, int64_t B, int32_t K, const float* sample_weight, int32_t flags, float row_scale,
                float* loss_rows, float* coeff, float* scores, float* d_center, int64_t ld_dc, float* d_ctx, int64_t ld_dx,
                dr_stream_t stream);
int dr_sgns_bwd(const float* in_table, const float* out_table, int32_t D, const int64_t* centers, const int64_t* contexts,
                const int64_t* negatives, int64_t B, int32_t K, int32_t flags, const float* coeff, const float* d_loss, float* d_center,
                int64_t ld_dc, float* d_ctx, int64_t ld_dx, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The integer kernels around the skip-gram step, csrc/sampling.hip.  All are counter-based on the hash of dr_attn_fwd's dropout
 * (dr_mix32, spelled out there): an element is a function of (seed, position) alone, never of the launch.
 *   dr_alias_sample   n draws from a Vose alias table (prob [V] fp32, alias [V] int32 with entries in [0, V), 1 <= V < 2^31), the
 *                     negative sampler of word2vec over counts^0.75.  Element i, with e = offset + i:
 *                       h1 = dr_mix32(seed, 2 e);  h2 = dr_mix32(seed, 2 e + 1);  slot = (uint64(h1) * V) >> 32;
 *                       r = (h2 >> 8) * 2^-24  (exact in fp32);   out[i] = r < prob[slot] ? slot : alias[slot]
 *                     so that draws [0, n) and then [n, 2 n) with offset = n equal one call of 2 n.
 *   dr_random_walk    W uniform random walks of L nodes over a CSR graph (row_ptr int64 [n_rows + 1], col int32, as dr_csr_spmm takes
 *                     them): walks [W, L] dense, walks[w, 0] = starts[w]; at step t >= 1 from v = walks[w, t - 1], with
 *                     deg = row_ptr[v + 1] - row_ptr[v]:  walks[w, t] = col[row_ptr[v] + ((uint64(dr_mix32(seed, w * L + t)) * deg) >> 32)].
 *                     v < 0, v >= n_rows or deg == 0 ends the walk: that step and every later one is -1.  One lane per walk.
 *   dr_random_walk_weighted   the same walk over integer edge weights: cum [nnz] int64 holds the inclusive prefix sums of the weights
 *                     (>= 0) over the whole col array.  From v, with lo = row_ptr[v], hi = row_ptr[v + 1]:
 *                       base = lo > 0 ? cum[lo - 1] : 0;  total = cum[hi - 1] - base;
 *                       t = (uint64(dr_mix32(seed, w * L + t_step)) * uint64(total)) >> 32;
 *                       walks[w, t_step] = col[e], e the smallest index in [lo, hi) with cum[e] - base > t  (binary search)
 *                     so an edge is taken for exactly weight(e) of the total values of t and a zero-weight edge never.  hi == lo or
 *                     total == 0 ends the walk as deg == 0 does.  The caller guarantees total < 2^32 for every row.  With all
 *                     weights 1 the walks are dr_random_walk's bit for bit.  col and cum may both be NULL for a graph without edges.
 *   n == 0 / W == 0 is DR_OK and launches nothing; V outside its range, L < 1, a negative size or a NULL required pointer is DR_EINVAL.
 * ---------------------------------------------------------------------------------------- */
int dr_alias_sample(const float* prob, const int32_t* alias, int64_t V, int64_t n, uint64_t seed, uint64_t offset, int64_t* out,
                    dr_stream_t stream);
int dr_random_walk(const int64_t* row_ptr, const int32_t* col, int64_t n_rows, const int64_t* starts, int64_t W, int32_t L,
                   uint64_t seed, int64_t* walks, dr_stream_t stream);
int dr_random_walk_weighted(const int64_t* row_ptr, const int32_t* col, const int64_t* cum, int64_t n_rows, const int64_t* starts,
                            int64_t W, int32_t L, uint64_t seed, int64_t* walks, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Skip-gram with side information: EGES (Wang et al., KDD 2018) and, with one field and two positives, Airbnb's listing embeddings
 * (Grbovic & Cheng, KDD 2018), which the reference's README lists and ships no code for; csrc/eges.hip.  All fp32.
 * side_table [R, D] dense; row_base [S] int64 on the device, the first row of field s (as the slab's); side_ids [B, S] int64: field s of
 * example b is the row row_base[s] + side_ids[b, s], an id < 0 means the field is missing ("present" otherwise).  att [R_att, ld_att]
 * (ld_att >= S) with att_ids [B] holds the example's attention logits; att == NULL or att_ids[b] < 0: all logits are 0, which with
 * missing fields is the paper's cold-start rule, the average of the side embeddings that are there.  out_table [R_out, D] dense;
 * contexts [B, P] (positives) and negatives [B, K] dense int64; w_b = sample_weight[b] (1 when NULL).
 *   a_s = att[att_ids[b], s] (or 0);  m = max over present s of a_s;  e_s = expf(a_s - m);  Z = sum_present e_s
 *   alpha_s = e_s / Z (0 for a missing field);   u = sum_present alpha_s w_s,  w_s the field's table row
 *   slots j = 0 .. P + K - 1: o_j from contexts then negatives, v_j = out_table[o_j], z_j = 1 for j < P
 *   s_j, loss_b, g_j exactly as documented for dr_sgns_fwd;   c_j = row_scale g_j  (d_loss[b] g_j in dr_eges_bwd)
 *   d_u = sum_j c_j v_j;   d_ctx[b, j, :] = c_j u;   d_side[b, s, :] = alpha_s d_u   (+0.0 for a missing field)
 *   q_s = <d_u, w_s>;  r = sum_present alpha_s q_s;  d_att[b, s] = alpha_s (q_s - r)
 *                      (+0.0 for a missing field, for the columns S .. ld_da - 1, and when the logits were taken as 0)
 *   Sums run in ascending index order, one fused multiply-add per term added (the first term of u is the rounded product).
 *   Skipped: the whole example when no field is present or contexts[b, 0] < 0; a slot whose id is < 0; with flags & DR_SGNS_SKIP_EQUAL
 *   a negative slot whose id equals any non-negative positive of the example.  A skipped slot or example has s = g = 0, rows of +0.0
 *   (a skipped example's alpha row too) and no term anywhere; the id of a skipped slot or a missing field, and every id of a skipped
 *   example, is never turned into an address that is read.
 *   dr_eges_fwd    writes loss_rows [B], coeff [B, P + K], alpha [B, S] and, unless NULL, scores [B, P + K], all dense.  With the three
 *                  gradient buffers given (all or none) the same pass writes d_side [B, S * D] at the pitch ld_ds, d_att [B, ld_da]
 *                  (dense; ld_da a multiple of 4 with S <= ld_da <= 16, S rounded up, so that K4 takes it as a D = ld_da row with ids
 *                  [B, 1]) and d_ctx [B, (P + K) * D] at the pitch ld_dx, for c_j = row_scale g_j.  Nothing beyond the widths named is
 *                  written; the pitches are ignored without the buffers.
 *   dr_eges_bwd    the same three buffers from coeff, alpha and a per-example d_loss [B], the rows gathered again, the same operations
 *                  in the same order: with d_loss[b] == row_scale both entry points write the same bits.  att is only tested against
 *                  NULL here (with att_ids it says whether the logits were taken as 0).
 *   dr_eges_embed  the aggregation alone: out [n, D] = u at the pitch ld_out; an example with no present field gets a row of +0.0.
 *                  What an index over all items, cold ones (no id row) included, is built from.
 *   d_side with ids side_ids and row_base, d_att with ids att_ids as [B, 1], d_ctx with ids [contexts | negatives] are what the K4
 *   entry points take as d_concat.  With S = 1, P = 1 and att == NULL, loss_rows, coeff, scores, d_side and d_ctx are dr_sgns_fwd's
 *   loss_rows, coeff, scores, d_center and d_ctx bit for bit (the slot arithmetic is one set of device functions, csrc/sgns_common.h).
 *   A group of D / 4 lanes, rounded up to a power of two, owns an example; u and d_u stay in registers, four rows are in flight per
 *   lane, the S rows w_s are read a second time once d_u is complete.  No atomics, no LDS, no workspace, one launch: results are
 *   bit-identical from run to run and an example's bits depend neither on its batch nor on its place in it.
 *   Domain: D % 4 == 0, 4 <= D <= 256, 1 <= S <= 16, 1 <= P <= 4, K >= 0, P + K <= 64 (negatives may be NULL when K == 0), flags 0 or
 *   DR_SGNS_SKIP_EQUAL, att_ids given whenever att is, both tables, the gradient buffers and out 16-byte aligned, ld_ds, ld_dx and
 *   ld_out multiples of 4 and >= the width they cover; anything else or a NULL required pointer is DR_EINVAL.  B == 0 / n == 0 is DR_OK
 *   and launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_eges_fwd(const float* side_table, int32_t D, const int64_t* row_base, const int64_t* side_ids, int32_t S, const float* att,
                int64_t ld_att, const int64_t* att_ids, const float* out_table, const int64_t* contexts, int32_t P,
                const int64_t* negatives, int32_t K, int64_t B, const float* sample_weight, int32_t flags, float row_scale,
                float* loss_rows, float* coeff, float* alpha, float* scores, float* d_side, int64_t ld_ds, float* d_att, int64_t ld_da,
                float* d_ctx, int64_t ld_dx, dr_stream_t stream);
int dr_eges_bwd(const float* side_table, int32_t D, const int64_t* row_base, const int64_t* side_ids, int32_t S, const float* att,
                const int64_t* att_ids, const float* out_table, const int64_t* contexts, int32_t P, const int64_t* negatives, int32_t K,
                int64_t B, int32_t flags, const float* coeff, const float* alpha, const float* d_loss, float* d_side, int64_t ld_ds,
                float* d_att, int64_t ld_da, float* d_ctx, int64_t ld_dx, dr_stream_t stream);
int dr_eges_embed(const float* side_table, int32_t D, const int64_t* row_base, const int64_t* side_ids, int32_t S, const float* att,
                  int64_t ld_att, const int64_t* att_ids, int64_t n, float* out, int64_t ld_out, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * PNN's outer-product layer (Qu et al., ICDM 2016; the reference's README lists PNN among its ranking models and ships no code for
 * it), csrc/pnn_outer.hip.  All fp32.  emb[b] holds the F rows of example b ([F * D], field-major: the slab's concat, read in place at
 * the pitch ld_emb); W [D * D, N] row-major at the pitch ld_w, row d * D + e multiplies u_d u_e (the full square, not a triangle).
 *   dr_pnn_outer_fwd   u[b, d] = sum_i emb[b, i * D + d], i ascending ([B, D] at ld_u; the backward reads it instead of emb);
 *                      out[b, n] = sum_{d,e} u[b,d] u[b,e] W[d * D + e, n], plus addend[b, n] when addend != NULL.
 *                      Writes D columns of u and N columns of out, nothing else.  F == 1: u = emb.  Two launches (u, then the GEMM
 *                      M = B, K = D^2 whose left operand is formed in LDS from the row tile's u, one multiply per lane).
 *   dr_pnn_outer_bwd   from g = d_out [B, N] (the addend's gradient is g itself and needs no kernel):
 *                        dW[d * D + e, n] = sum_b u[b,d] u[b,e] g[b,n]                      (N columns of every row are overwritten)
 *                        S[b,d,e] = sum_n g[b,n] W[d * D + e, n];  du[b,d] = sum_e (S[b,d,e] + S[b,e,d]) u[b,e]
 *                        d_emb[b, i * D + d] = du[b,d] for every field i; accumulate 1: added to what d_emb holds, 0: overwrites
 *                      (S + S^T is one product with W[(d,e)] + W[(e,d)], added as the tile is staged).  Three launches.
 *                      workspace: 16-byte aligned, at least dr_pnn_outer_bwd_workspace_bytes(B, F, D, N) bytes
 *                        = 4 * parts * D * D * 4 ceil(N / 4),  per = 128 * max(1, ceil(B / 8192)),  parts = max(1, ceil(B / per)) <= 64
 *                      [dW of each run of `per` examples, added in run order].  It does not grow with B beyond 64 copies of dW.
 *                      dr_pnn_outer_bwd_workspace_bytes returns DR_EINVAL / DR_ESHAPE (negative) outside the domain.
 *   All products run on the fp32-input MFMA (v_mfma_f32_32x32x2_f32).  No tensor of B * D^2 or B * N * D elements is written in either
 *   direction.  Every sum has one owner and a fixed order: no float atomics in memory or LDS, results bit-identical from run to run,
 *   and u, out and d_emb of an example do not depend on its batch.
 *   Every row of W, addend and d_out, the last one too, must be readable up to 4 ceil(N / 4) floats (the pitch covers that); what the
 *   padding holds, NaN included, reaches nothing.
 *   Domain: D % 4 == 0, 4 <= D <= 128, 1 <= N <= 4096, 1 <= F <= 64, accumulate 0 or 1; every ld a multiple of 4 and at least the width
 *   it covers (ld_emb, ld_demb >= F * D; ld_u >= D; ld_w, ld_add, ld_out, ld_dout, ld_dw >= N); every pointer 16-byte aligned.
 *   Anything else, a NULL required pointer (addend may be NULL) or a short workspace is DR_EINVAL.  B > 2^31 is DR_ESHAPE from all
 *   three entry points alike.  B == 0 is DR_OK and launches nothing.
 * ---------------------------------------------------------------------------------------- */
int dr_pnn_outer_fwd(const float* emb, int64_t ld_emb, const float* W, int64_t ld_w, const float* addend, int64_t ld_add, int64_t B,
                     int32_t F, int32_t D, int32_t N, float* u, int64_t ld_u, float* out, int64_t ld_out, dr_stream_t stream);
int64_t dr_pnn_outer_bwd_workspace_bytes(int64_t B, int32_t F, int32_t D, int32_t N);
int dr_pnn_outer_bwd(const float* u, int64_t ld_u, const float* W, int64_t ld_w, const float* d_out, int64_t ld_dout, int64_t B,
                     int32_t F, int32_t D, int32_t N, float* d_emb, int64_t ld_demb, int32_t accumulate, float* dW, int64_t ld_dw,
                     void* ws, int64_t ws_bytes, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DIN ActivationUnit input (keras/models/ranking/din.py:59-67): out[b, :] = concat(x[b], y[b], interacter(x, y)[b])
 * mode 0: no interacter (2 D columns), 1: x - y (keras Subtract, the reference test's interacter), 2: x * y (Multiply).
 * The two Dense layers that follow (:69-70) are dr_linear_fwd / dr_linear_bwd_*.
 * ---------------------------------------------------------------------------------------- */
int dr_din_concat_fwd(const float* x, const float* y, int64_t B, int32_t D, int32_t mode, float* out, int64_t ld_out,
                      dr_stream_t stream);
int dr_din_concat_bwd(const float* x, const float* y, int64_t B, int32_t D, int32_t mode, const float* d_out,
                      int64_t ld_dout, float* d_x, float* d_y, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Element-wise pieces around the GEMM path (deep_recommenders_amd/csrc/elementwise.hip):
 * dr_act_fwd / _bwd   a Dense activation other than ReLU (keras/models/ranking/deepfm.py:30-34 `dnn_activation`,
 *                     estimator/models/feature_interaction/dnn.py:9-14): act 1 relu, 2 sigmoid, 3 tanh, in place on the linear
 *                     layer's output [M, N] (leading dimension ld); backward dy *= act'(y) through the saved output.
 * dr_dropout_fwd/_bwd tf.nn.dropout(x, rate) of estimator/.../dnn.py:26-27 (always on there): keep iff hash(seed, index) >=
 *                     rate * 2^32, kept elements * 1 / (1 - rate); mask [M * N] bytes saved for the backward.
 * dr_reduce_sum       out[0] (+)= alpha * sum x (squared = 0) / alpha * sum x^2 (squared = 1: the L2 term of a Keras
 *                     kernel_regularizer / bias_regularizer, dcn.py:27-30,39-45); fixed-order two-stage reduction;
 *                     workspace: 1024 floats.
 * ---------------------------------------------------------------------------------------- */
int dr_act_fwd(float* x, int64_t M, int32_t N, int64_t ld, int32_t act, dr_stream_t stream);
int dr_act_bwd(const float* y, int64_t ld_y, float* dy, int64_t ld_dy, int64_t M, int32_t N, int32_t act,
               dr_stream_t stream);
int dr_dropout_fwd(const float* x, int64_t ld_x, int64_t M, int32_t N, float rate, uint64_t seed, float* y,
                   int64_t ld_y, uint8_t* mask, dr_stream_t stream);
int dr_dropout_bwd(const float* dy, int64_t ld_dy, const uint8_t* mask, int64_t M, int32_t N, float rate, float* dx,
                   int64_t ld_dx, dr_stream_t stream);
int dr_reduce_sum(const float* x, int64_t n, int32_t squared, float alpha, int32_t accumulate, float* out,
                  float* workspace, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Multi-task learning (estimator/models/multi_task_learning/{mixture_of_experts,esmm}.py, examples/train_mmoe_on_synthetic_estimator.py)
 *
 * Grouped dense layers: G independent problems of one shape (M, K, N) in ONE launch -- MMoE's expert layers after the first
 * and the task towers (mixture_of_experts.py:60-67,79-88), ESMM's two towers (esmm.py:35-51).  Group g reads x at
 * x + g*x_gs (row pitch ld_x), W at W + g*w_gs, b at b + g*b_gs and writes y at y + g*y_gs (row pitch ld_y); dy / dx / relu_src /
 * dW / db likewise.  Same contract as dr_linear_fwd / _bwd_dx / _bwd_dw (relu in the fwd epilogue, relu' folded into dx through
 * relu_src; dw into a zeroed buffer with scale = 1 or into the parameter with scale = -lr).  With a workspace of
 * dr_linear_bwd_dw_grouped_workspace_bytes() the weight AND bias gradients are combined in a fixed order (deterministic; each
 * group's dW equals dr_linear_bwd_dw's with a workspace bit for bit); without one, fp32 atomics.  Every GEMM mode
 * (dr_set_gemm_mode) applies.  G > 65535 returns DR_ESHAPE (the caller falls back to per-group dr_linear_* calls).
 * ---------------------------------------------------------------------------------------- */
int dr_linear_fwd_grouped(const float* x, int64_t ld_x, int64_t x_gs, const float* W, int64_t ld_w, int64_t w_gs, const float* b,
                          int64_t b_gs, int64_t M, int32_t K, int32_t N, int32_t G, int32_t act, float* y, int64_t ld_y, int64_t y_gs,
                          dr_stream_t stream);
int dr_linear_bwd_dx_grouped(const float* dy, int64_t ld_dy, int64_t dy_gs, const float* W, int64_t ld_w, int64_t w_gs, int64_t M,
                             int32_t K, int32_t N, int32_t G, const float* relu_src, int64_t ld_relu_src, int64_t rs_gs,
                             int32_t accumulate, float* dx, int64_t ld_dx, int64_t dx_gs, dr_stream_t stream);
int64_t dr_linear_bwd_dw_grouped_workspace_bytes(int64_t M, int32_t K, int32_t N, int32_t G);
int dr_linear_bwd_dw_grouped(const float* x, int64_t ld_x, int64_t x_gs, const float* dy, int64_t ld_dy, int64_t dy_gs, int64_t M,
                             int32_t K, int32_t N, int32_t G, float scale, float* dstW, int64_t ld_w, int64_t w_gs, float* dstb,
                             int64_t b_gs, float* workspace, int64_t workspace_bytes, dr_stream_t stream);

/* MMoE gate softmax + expert mixture (mixture_of_experts.py:71-77).  h [B, E*U] (expert e in columns e*U ..), logits [B, T*E]:
 *   fwd  p[b,t,:] = softmax(logits[b, t*E : (t+1)*E]) (maximum subtracted), out[b, t*U+u] = sum_e p[b,t,e] h[b, e*U+u] (ascending e);
 *        p [B, T*E] is saved for the backward.
 *   bwd  d_h[b, e*U+u] = sum_t p[b,t,e] d_out[b, t*U+u] (ascending t);
 *        d_l[b,t,e] = p[b,t,e] (<d_out_t, h_e> - sum_e' p[b,t,e'] <d_out_t, h_e'>).
 * One 64-lane wave per row, no atomics (deterministic).  Domain 1 <= E <= 64, 1 <= T <= 16, U >= 1; otherwise DR_ESHAPE. */
int dr_mmoe_gate_mix_fwd(const float* h, int64_t ld_h, const float* logits, int64_t ld_l, int64_t B, int32_t E, int32_t T, int32_t U,
                         float* p, int64_t ld_p, float* out, int64_t ld_out, dr_stream_t stream);
int dr_mmoe_gate_mix_bwd(const float* h, int64_t ld_h, const float* p, int64_t ld_p, const float* d_out, int64_t ld_do, int64_t B,
                         int32_t E, int32_t T, int32_t U, float* d_h, int64_t ld_dh, float* d_l, int64_t ld_dl, dr_stream_t stream);

/* T mean-squared-error losses in one call (tf.losses.mean_squared_error, SUM_BY_NONZERO_WEIGHTS with unit weights;
 * examples/train_mmoe_on_synthetic_estimator.py:39-40): pred [B, T] and labels [B, T] row-major with pitches,
 * loss[t] = mean_b (pred - y)^2, d_pred = 2 (pred - y) / B (may be NULL).  Fixed-order two-stage reduction. */
int64_t dr_mse_workspace_bytes(int32_t T);
int dr_mse_fwd_bwd(const float* pred, int64_t ld_pred, const float* labels, int64_t ld_labels, int64_t B, int32_t T, float* loss,
                   float* d_pred, int64_t ld_dpred, float* workspace, int64_t workspace_bytes, dr_stream_t stream);

/* ESMM head (esmm.py:33-55): logits [B, 2] = (cvr, ctr) -> p_cvr, p_ctr, p_ctcvr = p_ctr * p_cvr, each [B].  The backward takes
 * any subset of the three output gradients (NULL = zero) and writes both logit gradients.  Finite for any finite logit. */
int dr_esmm_head_fwd(const float* logits, int64_t ld_logits, int64_t B, float* p_cvr, float* p_ctr, float* p_ctcvr, dr_stream_t stream);
int dr_esmm_head_bwd(const float* p_cvr, const float* p_ctr, const float* d_cvr, const float* d_ctr, const float* d_ctcvr, int64_t B,
                     float* d_logits, int64_t ld_dlogits, dr_stream_t stream);

/* dr_adam_step on a [rows, cols] block with a pitch per operand: the column slice of a concatenated parameter that one TF variable
 * is (MMoE's gates); same per-element arithmetic as dr_adam_step. */
int dr_adam_step_2d(float* param, int64_t ld_p, const float* grad, int64_t ld_g, float* m, float* v, int64_t ld_mv, int64_t rows,
                    int32_t cols, float lr_t, float beta1, float beta2, float eps, float grad_scale, dr_stream_t stream);

/* tf.feature_column.input_layer's column assembly: out[m][j] = map[j] >= 0 ? a[m][map[j]] : b[m][-map[j] - 1]  (numeric block and
 * pooled embeddings interleaved by column name); also its backward (the pooled embeddings' gradient out of d_input). */
int dr_gather_cols(const float* a, int64_t lda, const float* b, int64_t ldb, const int32_t* map, int64_t M, int32_t N, float* out,
                   int64_t ldo, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Graph convolution (keras/models/retrieval/gcn.py:44-55, examples/train_gcn_on_cora_keras.py; csrc/graph.hip)
 *
 * CSR of A [n_rows, n_cols]: row_ptr int64 [n_rows + 1] (row_ptr[n_rows] == nnz), col int32 [nnz], val fp32 [nnz].  Dense operands
 * are fp32 row-major with a row pitch that is a multiple of 4 floats and a 16-byte aligned base (DR_EINVAL otherwise).
 *   dr_csr_spmm        out[r, :D] = (sum_k val[k] X[col[k], :D]) * (relu_src[r] > 0) (+ out[r] if accumulate), k over row r in
 *                      ascending order (tf.sparse.sparse_dense_matmul, gcn.py:45-46); relu_src may be NULL.  Rows with more than
 *                      DR_CSR_LONG_ROW entries are cut into fixed chunks whose partial sums are added in chunk order: no atomics,
 *                      every call bit-identical.  Needs the plan of the same CSR (dr_csr_plan; may be NULL when
 *                      dr_csr_spmm_workspace_bytes(nnz, D) == 0) and a workspace of that many bytes.  64-bit addressing.
 *   dr_csr_plan        the long rows and their chunks, once per graph: plan >= dr_csr_plan_bytes(nnz) bytes, workspace >=
 *                      dr_csr_plan_workspace_bytes(n_rows) bytes.
 *   dr_csr_transpose   the CSR of A^T (t_row_ptr [n_cols + 1], t_col / t_val [nnz]) on the device, source rows ascending inside every
 *                      column (a stable radix sort by column): the backward dX = A^T dAgg is dr_csr_spmm on it.  n_rows, n_cols < 2^31.
 *   dr_softmax_rows_fwd / _bwd   y = softmax(x) per row (maximum subtracted); dx = y * (dy - sum_c y dy).  One wave per row.
 *   dr_cce_prob_rows   tf.keras.losses.categorical_crossentropy on probabilities: q = clip(p / sum_c p, 1e-7, 1 - 1e-7),
 *                      row_loss[r] = w_r * -sum_c y log q, grad (may be NULL) = d row_loss / d p.  sample_weight may be NULL.
 * ---------------------------------------------------------------------------------------- */
int64_t dr_csr_plan_bytes(int64_t nnz);
int64_t dr_csr_plan_workspace_bytes(int64_t n_rows);
int dr_csr_plan(const int64_t* row_ptr, int64_t n_rows, int64_t nnz, int64_t* plan, int64_t plan_bytes, void* workspace,
                int64_t workspace_bytes, dr_stream_t stream);
int64_t dr_csr_spmm_workspace_bytes(int64_t nnz, int32_t D);
int dr_csr_spmm(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows, int64_t nnz, const float* X, int64_t ld_x,
                int32_t D, const float* relu_src, int64_t ld_relu_src, int32_t accumulate, float* out, int64_t ld_out,
                const int64_t* plan, float* workspace, int64_t workspace_bytes, dr_stream_t stream);
int64_t dr_csr_transpose_workspace_bytes(int64_t nnz, int64_t n_cols);
int dr_csr_transpose(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_rows, int64_t n_cols, int64_t nnz,
                     int64_t* t_row_ptr, int32_t* t_col, float* t_val, void* workspace, int64_t workspace_bytes, dr_stream_t stream);
int dr_softmax_rows_fwd(const float* x, int64_t ld_x, int64_t B, int32_t C, float* y, int64_t ld_y, dr_stream_t stream);
int dr_softmax_rows_bwd(const float* y, int64_t ld_y, const float* dy, int64_t ld_dy, int64_t B, int32_t C, float* dx, int64_t ld_dx,
                        dr_stream_t stream);
int dr_cce_prob_rows(const float* p, int64_t ld_p, const float* labels, int64_t ld_labels, int64_t B, int32_t C,
                     const float* sample_weight, float* row_loss, float* grad, int64_t ld_grad, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sampled graph blocks: GraphSAGE (Hamilton et al., NeurIPS 2017) and PinSage (Ying et al., KDD 2018), which the reference's README
 * lists and ships no code for; csrc/neighbor_sample.hip.  Integer kernels (one fp32 division per edge in dr_block_csr), counter-based
 * on dr_mix32 (spelled out at dr_attn_fwd): an output is a function of (seed, inputs) alone, never of the launch, the grid or the run.
 * The graph is a CSR as dr_csr_spmm takes it (row_ptr int64 [n_rows + 1], col int32).  Node lists are int64 with -1 for "none".
 *   dr_neighbor_sample   nbr [n, fanout] int64, cnt [n] int32.  For i < n: v = nodes[i]; v < 0 or v >= n_rows: cnt[i] = 0, the row of
 *                     nbr is all -1 and nothing is dereferenced.  Otherwise lo = row_ptr[v], hi = row_ptr[v + 1], deg = hi - lo.
 *                       deg <= fanout: nbr[i, :] = col[lo .. hi) in CSR order, then -1; cnt[i] = deg.
 *                       deg >  fanout: edge e in [lo, hi) has the key (uint64(dr_mix32(seed, e)) << 32) | uint64(e - lo); the fanout
 *                                      edges with the smallest keys are taken (the keys are distinct: the set is unique) and col[e] of
 *                                      them is written in ascending e; cnt[i] = fanout.
 *                     Uniform without replacement under a uniform hash; the sample of v does not depend on where v sits in nodes.
 *                     1 <= fanout <= 64.  Rows of up to DR_SAMPLE_LONG_ROW (512) edges are selected by one wave, longer ones by a
 *                     whole block (a radix select on the hash): the same result either way.  col may be NULL for a graph without edges.
 *   dr_walk_neighbors PinSage's importance neighbours.  walks [n, R, L] int64 is dr_random_walk's output for every node repeated R
 *                     times as start (walks[i, r, 0] is the node).  For start i: every id in walks[i, :, 1:] that is >= 0 and differs
 *                     from walks[i, 0, 0] is a visit; the distinct visited ids are ordered by (visits descending, id ascending) and the
 *                     first T of them are written to nbr [n, T] int64 with weight [n, T] fp32 = visits (a small integer, exact); the
 *                     rest of both rows is -1 and 0; cnt[i] = the number kept.  R (L - 1) <= 1024, 1 <= T <= 64, R >= 1, L >= 1.
 *   dr_frontier_build the next layer's node list.  dst [n_dst] int64: valid ids (>= 0) form a prefix, -1 a suffix of padding.
 *                     nbr [m] int64, -1 = none.  id_bound > 0 is the caller's promise that every id is < id_bound (the number of graph
 *                     nodes: it sets the number of sort passes; an id >= id_bound in nbr is treated as none); id_bound <= 0: any id
 *                     < 2^63 - 1.  Outputs: counts [2] int64 on the device, src [n_dst + m] int64, local [m] int32.
 *                       counts[0] = the number of valid dst entries; src[0 .. counts[0]) = that prefix verbatim;
 *                       src[counts[0] .. counts[1]) = the distinct ids of nbr that occur nowhere in dst, in ascending id order;
 *                       src[counts[1] ..) = -1;  local[j] = the index in src of nbr[j] -- for an id that dst holds several times, the
 *                       lowest such index -- and -1 where nbr[j] is none.
 *                     No host reads: src is a valid `nodes` / `dst` of the next layer.  n_dst + m < 2^31.  workspace >=
 *                     dr_frontier_workspace_bytes(n_dst, m) bytes.  m == 0 with n_dst > 0 still writes src and counts.
 *   dr_block_csr      the CSR of one block.  cnt [n_dst] int32 (clamped to [0, fanout]), local [n_dst, fanout] int32, weight
 *                     [n_dst, fanout] fp32 or NULL (all 1).  n_valid: a device pointer to the number of valid rows (dr_frontier_build's
 *                     counts[0] of the layer whose src these rows are), or NULL for n_dst.  len(r) = cnt[r] + add_self for r < *n_valid,
 *                     0 beyond; row_ptr [n_dst + 1] int64 = the exclusive scan of len.  Row r holds, with add_self, first (r, weight 1),
 *                     then (local[r, k], w_k) for k < cnt[r] in that order, w_k = weight[r, k] or 1;  S = the fp32 sum of the row's
 *                     weights taken in that order starting from 0 (with add_self: from the self weight 1);  val = w / S, one fp32
 *                     division per entry.  col / val need room for n_dst (fanout + add_self) entries.  add_self is 0 or 1;
 *                     1 <= fanout <= 64; workspace >= dr_block_csr_workspace_bytes(n_dst) bytes.
 *   A size of 0 (n, or n_dst + m, or n_dst) is DR_OK and launches nothing; a negative size, a NULL required pointer, a parameter outside
 *   its range or a workspace that is too small is DR_EINVAL.
 * ---------------------------------------------------------------------------------------- */
int dr_neighbor_sample(const int64_t* row_ptr, const int32_t* col, int64_t n_rows, const int64_t* nodes, int64_t n, int32_t fanout,
                       uint64_t seed, int64_t* nbr, int32_t* cnt, dr_stream_t stream);
int dr_walk_neighbors(const int64_t* walks, int64_t n, int32_t R, int32_t L, int32_t T, int64_t* nbr, float* weight, int32_t* cnt,
                      dr_stream_t stream);
int64_t dr_frontier_workspace_bytes(int64_t n_dst, int64_t m);
int dr_frontier_build(const int64_t* dst, int64_t n_dst, const int64_t* nbr, int64_t m, int64_t id_bound, int64_t* src, int64_t* counts,
                      int32_t* local, void* workspace, int64_t workspace_bytes, dr_stream_t stream);
int64_t dr_block_csr_workspace_bytes(int64_t n_dst);
int dr_block_csr(const int32_t* cnt, const int32_t* local, const float* weight, int64_t n_dst, int32_t fanout, int32_t add_self,
                 const int64_t* n_valid, int64_t* row_ptr, int32_t* col, float* val, void* workspace, int64_t workspace_bytes,
                 dr_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * Transformer package (keras/models/nlp/ of the reference), csrc/attention.hip.
 *
 *   dr_attn_fwd   ScaledDotProductAttention of every (batch, head) (multi_head_attention.py:60-86 inside :122-149).  q [B, Lq, H*dh],
 *                 k, v [B, Lk, H*dh] fp32 with row pitches ld_* >= H*dh; head h is the column block [h*dh, (h+1)*dh) -- the
 *                 reference's split / concat copies do not exist.  s = (q . k) / sqrt(dh); key_mask (may be NULL) [B, Lk] bytes,
 *                 1 = padded: s += -2^32 (the fp32 value of -2^32 + 1; an fp32 add, so it saturates only for |s| < 128..256);
 *                 future != 0 (needs Lq == Lk): entries with key > query are REPLACED by -2^32.  p = softmax_k(s) -- a row whose
 *                 scores are all equal is uniform over all Lk keys.  Dropout: element (b, h, i, j) is kept iff
 *                 dr_mix32(seed, ((b*H + h)*Lq + i)*Lk + j) >= (uint32)min(4294967040, rate * 2^32)   [always when rate == 0], with
 *                   dr_mix32(seed, idx): z = idx * 0x9E3779B97F4A7C15 + seed; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                                        z = (z ^ z >> 27) * 0x94D049BB133111EB; return (z ^ z >> 31) >> 32      (64-bit wrap-around)
 *                 and kept probabilities are scaled by 1 / (1 - rate).  out [B, Lq, H*dh] = p_dropped . v.
 *                 stats [B*H*Lq, 2] = (row maximum, sum of exp(s - maximum)) for the backward.  1 <= dh <= 128, any Lq, Lk >= 1.
 *                 Products are fp32-input MFMA (exact fp32 products).  DR_ESHAPE: dh > 128, future with Lq != Lk; DR_EINVAL: rate
 *                 outside [0, 1), a pitch below H*dh, a NULL tensor.
 *   dr_attn_bwd   dq, dk, dv (same strided layout) from d_out; p is recomputed from q, k and stats, the dropout mask from the hash.
 *                 The gradient passes through the additive padding mask and stops at entries the future mask replaced.
 *                 delta: workspace of B*H*Lq floats (sum_j p_ij dp_ij, summed from the recomputed p and dp in a pass of its own).
 *                 Bit-reproducible: no atomics, no inter-block waits.
 *   dr_add_layernorm_fwd / _bwd   y = gamma * (s - mean) / sqrt(var + eps) + beta over the last axis, s = a + b (b may be NULL),
 *                 population variance (transformer.py:109-113 after the residual adds of :212-219).  stats [M, 2] = (mean,
 *                 1 / sqrt(var + eps)).  The backward writes d_s (the gradient of both addends), d_gamma and d_beta (overwritten;
 *                 fixed-order column reduction through a workspace of dr_add_layernorm_bwd_workspace_bytes(M, D) bytes).
 *   dr_token_embedding_fwd   out[n, :] = dropout(table[ids[n], :] * sqrt(D) + pos[n % L, :]) for n < N = B*L (transformer.py:195-204);
 *                 pos [L, D] may be NULL; dropout as above on the element index n*D + c.  An id outside [0, V) reads as a zero row.
 *   dr_token_embedding_bwd   d_table[v, :] += sqrt(D) * sum over the positions n with ids[n] == v, ascending, of the kept
 *                 d_out[n, :] / (1 - rate).  sorted_ids / order: the ids sorted ascending by a STABLE sort and the permutation that
 *                 sorts them (int64 [N]); every table row has one owner block: a fixed order, no atomics.
 * ---------------------------------------------------------------------------------------- */
int dr_attn_fwd(const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v, const uint8_t* key_mask,
                int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t dh, int32_t future, float rate, uint64_t seed, float* out,
                int64_t ld_o, float* stats, dr_stream_t stream);
int dr_attn_bwd(const float* q, int64_t ld_q, const float* k, int64_t ld_k, const float* v, int64_t ld_v, const uint8_t* key_mask,
                const float* d_out, int64_t ld_do, const float* stats, int32_t B, int32_t H,
                int32_t Lq, int32_t Lk, int32_t dh, int32_t future, float rate, uint64_t seed, float* dq, int64_t ld_dq,
                float* dk, int64_t ld_dk, float* dv, int64_t ld_dv, float* delta, dr_stream_t stream);
int dr_add_layernorm_fwd(const float* a, int64_t ld_a, const float* b, int64_t ld_b, const float* gamma, const float* beta,
                         int64_t M, int32_t D, float eps, float* y, int64_t ld_y, float* stats, dr_stream_t stream);
int64_t dr_add_layernorm_bwd_workspace_bytes(int64_t M, int32_t D);
int dr_add_layernorm_bwd(const float* a, int64_t ld_a, const float* b, int64_t ld_b, const float* gamma, const float* stats,
                         const float* dy, int64_t ld_dy, int64_t M, int32_t D, float* d_s, int64_t ld_ds, float* d_gamma,
                         float* d_beta, float* workspace, int64_t workspace_bytes, dr_stream_t stream);
int dr_token_embedding_fwd(const int64_t* ids, int64_t N, int32_t L, const float* table, int64_t V, int32_t D, const float* pos,
                           float rate, uint64_t seed, float* out, int64_t ld_out, dr_stream_t stream);
int dr_token_embedding_bwd(const int64_t* sorted_ids, const int64_t* order, int64_t N, int64_t V, int32_t D, const float* d_out,
                           int64_t ld_do, float rate, uint64_t seed, float* d_table, dr_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * DIN (keras/models/ranking/din.py of the reference), csrc/din.hip.
 *
 *   dr_dice_fwd   Dice (din.py:88-130) over the rows of x [M, N] fp32 (row pitch ld_x), alpha [N] = Keras PReLU's parameter:
 *                   m = mean_j x_j;  s = sqrt(mean_j (x_j - m)^2);  r = 1 / sqrt(s + eps)     (the reference's second square root)
 *                   p_j = sigmoid((x_j - m) r);  pre_j = max(x_j, 0) - alpha_j max(-x_j, 0);  y_j = pre_j > 0 ? p_j pre_j : (1 - p_j) pre_j
 *                 Any M >= 0 and N >= 1 (DR_ESHAPE otherwise).
 *   dr_dice_bwd   dx [M, N] and dalpha [N] (overwritten) from dy:
 *                   dpre_j = dy_j (pre_j > 0 ? p_j : 1 - p_j);   c_j = dy_j pre_j (pre_j > 0 ? 1 : -1) p_j (1 - p_j)
 *                   dx_i = dpre_i (x_i > 0 ? 1 : x_i < 0 ? alpha_i : 0) + r (c_i - mean_j c_j)
 *                          - 0.5 r^3 (sum_j c_j (x_j - m)) (x_i - m) / (N s)            [this term is ZERO where s == 0]
 *                   dalpha_j = sum over rows of dpre_j min(x_j, 0)
 *                 s == 0 (a constant row, always for N == 1): TensorFlow's gradient is NaN there; this returns the finite rest.
 *                 dalpha is reduced in a fixed order in two stages through a workspace of dr_dice_bwd_workspace_bytes(M, N) bytes
 *                 (no float atomics: bit-reproducible).
 *   dr_din_pool_fwd   score[b, t] = mask[b, t] ? Dense(1)(act(concat([q_b, k_bt, inter(q_b, k_bt)]) W + b)) : 0   (scores [B, T], dense)
 *                     out[b, :]   = sum over the valid t of score[b, t] keys[b, t, :]                               (no softmax)
 *                 query [B, D] (pitch ld_q), keys [B, T, D] with key (b, t) at keys + (b T + t) ld_k (ld_k % 4 == 0, 16-byte aligned),
 *                 mask [B, T] bytes, nonzero = valid, NULL = all valid.  W [(2 or 3) D, U] dense row-major in the concat's order
 *                 [q | k | inter]; mode 0: no interacter (W is [2D, U]), 1: q - k, 2: q * k.  b [U], b_out [1] may be NULL (no bias);
 *                 w_out [U].  act 0 linear, 1 relu, 2 sigmoid, 3 tanh, 4 Dice over the U hidden units with alpha [U] and eps.
 *                 Masked keys are never read.  One launch, fp32-input MFMA products, nothing of size B T except scores is written.
 *                 Domain: D % 4 == 0, 4 <= D <= 128, 1 <= U <= 128, T >= 1, B >= 0 -- DR_ESHAPE outside it.
 *   dr_din_pool_bwd   d_query [B, D], d_keys [B, T, D] (exactly 0 at masked keys), dW, db, d_w_out, d_b_out, dalpha (all overwritten;
 *                 db / d_b_out / dalpha may be NULL when the forward had none) from d_out [B, D] (pitch ld_do % 4 == 0) and d_scores
 *                 [B, T] dense (may be NULL).  The hidden layer is recomputed; the workspace (dr_din_pool_bwd_workspace_bytes) holds its
 *                 gradient [B T, U] and the fixed-order partial sums of the parameter gradients.  Bit-reproducible.
 * ---------------------------------------------------------------------------------------- */
int dr_dice_fwd(const float* x, int64_t ld_x, const float* alpha, int64_t M, int32_t N, float eps, float* y, int64_t ld_y,
                dr_stream_t stream);
int64_t dr_dice_bwd_workspace_bytes(int64_t M, int32_t N);
int dr_dice_bwd(const float* x, int64_t ld_x, const float* alpha, const float* dy, int64_t ld_dy, int64_t M, int32_t N, float eps,
                float* dx, int64_t ld_dx, float* dalpha, void* workspace, int64_t workspace_bytes, dr_stream_t stream);
int dr_din_pool_fwd(const float* query, int64_t ld_q, const float* keys, int64_t ld_k, const uint8_t* mask, const float* W,
                    const float* b, const float* w_out, const float* b_out, const float* alpha, int64_t B, int32_t T, int32_t D,
                    int32_t U, int32_t mode, int32_t act, float eps, float* out, int64_t ld_out, float* scores, dr_stream_t stream);
int64_t dr_din_pool_bwd_workspace_bytes(int64_t B, int32_t T, int32_t D, int32_t U);
int dr_din_pool_bwd(const float* query, int64_t ld_q, const float* keys, int64_t ld_k, const uint8_t* mask, const float* W,
                    const float* b, const float* w_out, const float* b_out, const float* alpha, const float* d_out, int64_t ld_do,
                    const float* d_scores, int64_t B, int32_t T, int32_t D, int32_t U, int32_t mode, int32_t act, float eps,
                    float* d_query, int64_t ld_dq, float* d_keys, int64_t ld_dk, float* dW, float* db, float* d_w_out,
                    float* d_b_out, float* dalpha, void* workspace, int64_t workspace_bytes, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Streaming evaluation metrics (deep_recommenders_amd/csrc/metrics.hip): the confusion counters of tf.metrics.auc
 * (examples/train_fm_on_movielens_estimator.py:47, train_fnn_..:48, train_deepfm_..:48, train_wdl_..:61) and of
 * tf.keras.metrics.AUC / Precision / Recall
 * (examples/train_deepfm_on_movielens_keras.py:45-47), kept on the device as one histogram.
 *
 * bucket(p) = the number of t in 0 .. T-1 with p > thresholds[t], every comparison in fp32 against the array passed (device memory,
 * ASCENDING, T floats), as TensorFlow compares.  A NaN compares false everywhere: bucket 0.  Predictions outside [0, 1] fall into
 * the end buckets a threshold array that brackets [0, 1] gives them; nothing on the device asserts the range.
 * hist[(labels[i] != 0) * (T + 1) + bucket(pred[i])] += weights[i] (1 when weights is NULL) for i < n; hist is [2][T + 1] fp64 and is
 * ACCUMULATED INTO (zero it to reset).  tp[t] = sum_{b > t} hist[1][b], fp[t] = sum_{b > t} hist[0][b], fn = sum hist[1] - tp,
 * tn = sum hist[0] - fp.  from_logits != 0: pred holds logits and bucket(sigmoid(pred[i])) is taken, with dr_sigmoid_fwd's arithmetic
 * (the state equals, bit for bit, an update with that kernel's output).
 * Without weights the per-block partial counts are integers combined in a fixed order: the state is exact up to 2^53 and
 * bit-identical from run to run.  With weights the sums are fp64 end to end (the order of the adds inside a block is not fixed).
 * Two launches on `stream`, no host synchronisation.  workspace: dr_confusion_hist_workspace_bytes(n, T) bytes (0 for arguments
 * the update refuses), contents unspecified before and after.
 * n == 0: nothing is done, DR_OK.  T < 1, n < 0 or (n > 0) a NULL pred / labels / thresholds / hist / workspace: DR_EINVAL.
 * T > 4096 (the supported maximum: the histogram and the thresholds live in LDS) or n > 2^40: DR_ESHAPE.
 * ---------------------------------------------------------------------------------------- */
int64_t dr_confusion_hist_workspace_bytes(int64_t n, int32_t num_thresholds);
int dr_confusion_hist_update(const float* pred, const float* labels, const float* weights, int64_t n, const float* thresholds,
                             int32_t T, int32_t from_logits, double* hist, void* workspace, dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Sampled softmax (csrc/sampled_softmax.hip): the training loss of YoutubeNet (Covington et al., RecSys 2016), which the reference's
 * README lists and ships no code for.  The arithmetic is TensorFlow's tf.nn.sampled_softmax_loss (_compute_sampled_logits + softmax
 * cross-entropy) with num_true = 1 and NO per-class bias (the paper's softmax has none; TensorFlow's users pass zeros).  All fp32.
 *   u [B, D] at the row pitch ld_u; table [V, D] dense, read in place by id (no [S, D] copy); labels int64 [B]; sampled int64 [S], shared
 *   by the whole batch; log_q_true [B], log_q_sampled [S], sample_weight [B] (w_i; each may be NULL: 0, 0, 1).
 *     t_i     = u_i . table[labels_i] - log_q_true_i
 *     s_ij    = u_i . table[sampled_j] - log_q_sampled_j
 *     keep_ij = sampled_j >= 0 and not (remove_accidental_hits and sampled_j == labels_i)
 *     lse_i   = log(exp(t_i) + sum_{j kept} exp(s_ij))
 *     loss_i  = w_i (lse_i - t_i)
 *   TensorFlow adds -FLT_MAX to an accidental hit, whose exp is 0 in fp32 beside the finite true logit: leaving the entry out is the
 *   same arithmetic.  An accidental hit masks one (i, j) entry; the column's row is still read by the other examples.
 *   A row with labels_i < 0 is padding: u_i is replaced by zeros on load (a NaN in it reaches no output), true_logit, row_lse and
 *   row_loss are 0 and so are its gradient rows.  A sampled id < 0 leaves its column out of every row and its d_sampled row is 0.  No
 *   id < 0 is turned into an address.  Labels and sampled ids must be < V: this is NOT checked on the device.
 *   dr_sampled_softmax_fwd   writes true_logit [B] (t_i), row_lse [B], row_loss [B] and, unless NULL, scores [B, S] dense (s_ij, -inf at
 *                            left-out entries; a padding row's are those of u_i = 0) -- for tests and diagnosis, never for training.
 *                            Without it nothing of size B * S is written: online softmax over 64-column tiles.
 *   dr_sampled_softmax_bwd   from the saved true_logit and row_lse, the gradients of row_scale * sum_i loss_i, the scores recomputed:
 *                              g_i = row_scale w_i (exp(t_i - lse_i) - 1),  G_ij = row_scale w_i exp(s_ij - lse_i)  (0 where left out)
 *                              d_u [B, D] at the pitch ld_du  = g_i table[labels_i] + sum_j G_ij table[sampled_j]
 *                              d_true [B, D] dense            = g_i u_i            what K4 takes as d_concat for ids labels [B, 1]
 *                              d_sampled [S, D] dense         = sum_i G_ij u_i     what K4 takes as d_concat for ids sampled [S, 1]
 *                            Two sweeps: a row-owning one (d_u, d_true) over all column tiles, a column-owning one (d_sampled) over a
 *                            chunk of the batch, the chunk partials added in chunk order.  Four products for the two of the
 *                            mathematics; no float atomics, no B * S tensor, bit-identical from run to run.
 *   Every product is v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), the true logit included: a sampled id equal to
 *   the label scores the bits of the true logit.  The columns are cut into dr_sampled_softmax_col_groups' segments -- a function of S
 *   alone: min(DR_SAMPLED_SOFTMAX_MAX_GROUPS, ceil(S / DR_SAMPLED_SOFTMAX_COL_GROUP)), evened out over whole tiles -- every segment
 *   starts from fresh accumulators and the segments are combined in ascending order, whether one block walks them all (more than
 *   DR_SAMPLED_SOFTMAX_SPLIT_TILES row tiles) or each has a block of its own: true_logit, row_lse, row_loss, d_u and d_true of a row
 *   depend on that row and `sampled` alone, not on B or the other rows.  dr_sampled_softmax_col_groups returns the number of blocks per
 *   row tile (1 or the segment count), dr_sampled_softmax_row_chunks the number of d_sampled partials (<= DR_SAMPLED_SOFTMAX_MAX_CHUNKS,
 *   at least DR_SAMPLED_SOFTMAX_ROW_CHUNK rows each): pure functions of (B, S, D), no device query.
 *   workspace: 16-byte aligned, dr_sampled_softmax_workspace_bytes(B, S, D) bytes (the same for both entry points): the (max, sum)
 *   pairs, the d_u partials of the split form and the d_sampled partials; nothing that grows like B * S.
 *   Domain: D % 4 == 0, 4 <= D <= 256, 1 <= S < 2^31, 1 <= V < 2^31, B >= 0; u, table, d_u, d_true, d_sampled 16-byte aligned, ld_u and
 *   ld_du multiples of 4 and >= D.  Anything else or a NULL required pointer is DR_ESHAPE / DR_EINVAL before a launch (the three
 *   sizing functions return the negative status).  B == 0 is DR_OK with nothing written.
 * ---------------------------------------------------------------------------------------- */
#define DR_SAMPLED_SOFTMAX_TILE 64
#define DR_SAMPLED_SOFTMAX_COL_GROUP 128
#define DR_SAMPLED_SOFTMAX_MAX_GROUPS 8
#define DR_SAMPLED_SOFTMAX_SPLIT_TILES 128
#define DR_SAMPLED_SOFTMAX_ROW_CHUNK 128
#define DR_SAMPLED_SOFTMAX_MAX_CHUNKS 64
int64_t dr_sampled_softmax_workspace_bytes(int64_t B, int64_t S, int32_t D);
int32_t dr_sampled_softmax_col_groups(int64_t B, int64_t S, int32_t D);
int32_t dr_sampled_softmax_row_chunks(int64_t B, int64_t S, int32_t D);
int dr_sampled_softmax_fwd(const float* u, int64_t ld_u, const float* table, int64_t V, int32_t D, const int64_t* labels, int64_t B,
                           const int64_t* sampled, int64_t S, const float* log_q_true, const float* log_q_sampled,
                           const float* sample_weight, int32_t remove_accidental_hits, float* true_logit, float* row_lse,
                           float* row_loss, float* scores, void* workspace, int64_t workspace_bytes, dr_stream_t stream);
int dr_sampled_softmax_bwd(const float* u, int64_t ld_u, const float* table, int64_t V, int32_t D, const int64_t* labels, int64_t B,
                           const int64_t* sampled, int64_t S, const float* log_q_sampled, const float* sample_weight,
                           int32_t remove_accidental_hits, float row_scale, const float* true_logit, const float* row_lse, float* d_u,
                           int64_t ld_du, float* d_true, float* d_sampled, void* workspace, int64_t workspace_bytes,
                           dr_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Margin ranking loss with hard-negative mining (csrc/margin_rank.hip): the training loss of EBR (Huang et al., "Embedding-based
 * Retrieval in Facebook Search", KDD 2020), which the reference's README lists and ships no code for -- a triplet loss over cosine
 * similarities against a negative matrix that the whole batch shares ("in-batch": the positives of the other rows), optionally
 * restricted to each row's num_hard hardest negatives (the paper's online hard-negative mining).  A sibling of the sampled softmax
 * above: the same tiles (csrc/dr_score_tile.h), no [B, S] tensor, scores recomputed in the backward.  All fp32.
 *   q [B, D] at the pitch ld_q; pos [B, D] at ld_p; neg [S, D] at ld_n (it may be the buffer of pos with S == B); pos_ids int64 [B],
 *   neg_ids int64 [S], sample_weight [B] (w_i), each may be NULL.  metric 0 (dot): x^ = x.  metric 1 (cosine): x^ = x r_x,
 *   r_x = (max(sum x^2, eps))^(-1/2) -- tf.math.l2_normalize with its epsilon (1e-12).
 *     t_i     = q^_i . p^_i                    s_ij = q^_i . n^_j
 *     valid_i = pos_ids == NULL or pos_ids_i >= 0
 *     keep_ij = valid_i and not (in_batch and j == i) and (neg_ids == NULL or neg_ids_j >= 0)
 *               and not (both id arrays given and neg_ids_j == pos_ids_i)
 *     N(i)    = all kept j (num_hard == 0) | the num_hard kept j of largest s_ij, ties to the smaller j (fewer if fewer are kept)
 *     h_ij    = margin - t_i + s_ij            loss_i = w_i sum_{j in N(i)} max(0, h_ij)       (h_ij == 0 is inactive)
 *   A padding row (valid_i false) has q_i replaced by zeros on load (a NaN in it reaches nothing; its pos row is not read for t_i);
 *   pos_score, row_loss, row_active and its d_q / d_pos rows are 0, its hard_idx -1.  A negative with id < 0 is never read and its
 *   d_neg row is 0.  No id is turned into an address: the ids are only compared.
 *   dr_margin_rank_fwd   writes pos_score [B] (t_i), row_loss [B], row_active int32 [B] (the number of j in N(i) with h_ij > 0), with
 *                        num_hard > 0 hard_idx int32 [B, num_hard] (falling score, -1 padded) and, unless NULL, scores [B, S] dense
 *                        (s_ij, -inf where not kept) -- for tests and diagnosis.  Without it nothing of size B * S is written.
 *   dr_margin_rank_bwd   from the forward's pos_score and hard_idx, the scores recomputed, the gradients of row_scale * sum_i loss_i
 *                        with respect to the RAW rows (the normalisation is differentiated inside):
 *                          a_ij = row_scale w_i [j in N(i) and h_ij > 0]    c_i = sum_j a_ij    e_i = sum_j a_ij s_ij    f_j = sum_i a_ij s_ij
 *                          d_q [B, D] at ld_dq = r_qi [ sum_j a_ij n^_j - c_i p^_i - pi_qi (e_i - c_i t_i) q^_i ]
 *                          d_pos [B, D] dense  = -c_i r_pi ( q^_i - pi_pi t_i p^_i )
 *                          d_neg [S, D] dense  = r_nj [ sum_i a_ij q^_i - pi_nj f_j n^_j ]
 *                        pi_x = 1 if sum x^2 >= eps else 0 (a zero row has cosine 0 with everything and gets the unprojected
 *                        gradient); metric dot is r = 1, pi = 0.  "j in N(i)" is "j is among hard_idx[i, :]" (num_hard compares, no
 *                        second selection).  All three are overwritten; in in-batch use the caller adds d_pos + d_neg.
 *   Every product is v_mfma_f32_16x16x4_f32 on the raw rows; the inverse norms (a prologue writes them to the workspace) multiply the
 *   score tile, (raw r_q) r_n, and the weights a_ij r_nj / a_ij r_qi of the second product.  Order of every sum: as the sampled
 *   softmax -- column segments that are a function of S alone (min(DR_MARGIN_RANK_MAX_GROUPS, ceil(S / DR_MARGIN_RANK_COL_GROUP)),
 *   evened out over whole tiles), fresh accumulators per segment, segments combined in ascending order whether one block walks them
 *   all (more than DR_MARGIN_RANK_SPLIT_TILES row tiles) or each has a block of its own; a row's pos_score, row_loss, row_active,
 *   hard_idx, d_q and d_pos depend on that row and the negatives alone, not on B or the other rows.  dr_margin_rank_col_segments returns
 *   the number of segments, dr_margin_rank_col_groups the number of blocks per row tile (1 or the segment count): pure functions of
 *   (B, S, D), no device query.  d_neg and f_j are summed over dr_margin_rank_row_chunks' chunks of the batch (<=
 *   DR_MARGIN_RANK_MAX_CHUNKS, at least DR_MARGIN_RANK_ROW_CHUNK rows each), the partials added in chunk order.  The top-k is a sorted (score, j) list per row,
 *   carried across the tiles of a segment and merged in segment order; its order is total, so the selected set does not depend on
 *   the segmentation.  The hinge terms of a row are summed in column order in both modes, so num_hard >= the number of kept columns
 *   gives the bits of num_hard == 0.  No float atomics, no waiting between workgroups; bit-identical from run to run.
 *   workspace: 16-byte aligned, dr_margin_rank_workspace_bytes(B, S, D, num_hard) bytes (the same for both entry points).
 *   Domain: D % 4 == 0, 4 <= D <= 256, 1 <= S < 2^31, B >= 0, 0 <= num_hard <= DR_MARGIN_RANK_MAX_HARD, metric 0 | 1, in_batch needs
 *   S == B; q, pos, neg, d_q, d_pos, d_neg, workspace 16-byte aligned, ld_q, ld_p, ld_n, ld_dq multiples of 4 and >= D.  Anything
 *   else or a NULL required pointer is DR_ESHAPE / DR_EINVAL before a launch (the three sizing functions return the negative status).
 *   B == 0 is DR_OK with nothing written.
 * ---------------------------------------------------------------------------------------- */
#define DR_MARGIN_RANK_TILE 64
#define DR_MARGIN_RANK_COL_GROUP 128
#define DR_MARGIN_RANK_MAX_GROUPS 8
#define DR_MARGIN_RANK_SPLIT_TILES 128
#define DR_MARGIN_RANK_ROW_CHUNK 128
#define DR_MARGIN_RANK_MAX_CHUNKS 64
#define DR_MARGIN_RANK_MAX_HARD 8
int64_t dr_margin_rank_workspace_bytes(int64_t B, int64_t S, int32_t D, int32_t num_hard);
int32_t dr_margin_rank_col_groups(int64_t B, int64_t S, int32_t D);
int32_t dr_margin_rank_col_segments(int64_t B, int64_t S, int32_t D);
int32_t dr_margin_rank_row_chunks(int64_t B, int64_t S, int32_t D);
int dr_margin_rank_fwd(const float* q, int64_t ld_q, const float* pos, int64_t ld_p, const float* neg, int64_t ld_n, int32_t D, int64_t B,
                       int64_t S, const int64_t* pos_ids, const int64_t* neg_ids, const float* sample_weight, float margin,
                       int32_t metric, int32_t in_batch, int32_t num_hard, float eps, float* pos_score, float* row_loss,
                       int32_t* row_active, int32_t* hard_idx, float* scores, void* workspace, int64_t workspace_bytes,
                       dr_stream_t stream);
int dr_margin_rank_bwd(const float* q, int64_t ld_q, const float* pos, int64_t ld_p, const float* neg, int64_t ld_n, int32_t D, int64_t B,
                       int64_t S, const int64_t* pos_ids, const int64_t* neg_ids, const float* sample_weight, float margin,
                       int32_t metric, int32_t in_batch, int32_t num_hard, float eps, float row_scale, const float* pos_score,
                       const int32_t* hard_idx, float* d_q, int64_t ld_dq, float* d_pos, float* d_neg, void* workspace,
                       int64_t workspace_bytes, dr_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * BERT (Devlin et al., NAACL 2019; the reference README's model list names it, its tree has no code for it), csrc/bert.hip.
 * All fp32, on the caller's stream, no host synchronisation, no float atomics: every result is bit-identical from run to run, and
 * a row's outputs do not depend on the batch around it (the column reductions d_gamma, d_beta, d_seg, d_pos and dr_colsum_add cut
 * their chunks by the row index and are fixed for a given shape).
 *
 *   dr_gelu_fwd   h = z * Phi(z) over z [M, N] (row pitches ld_z, ld_h >= N, any N >= 1), Phi(z) = erfc(-z / sqrt 2) / 2: the exact
 *                 GELU 0.5 z (1 + erf(z / sqrt 2)) without the cancellation of 1 + erf at negative z.  Saturated inputs give finite
 *                 values: gelu(-88) = -0.0, gelu(88) = 88.  h may not alias z where the backward still needs z.
 *   dr_gelu_bwd   in place on dy [M, N]: dy *= Phi(z) + z phi(z), phi(z) = exp(-z^2 / 2) / sqrt(2 pi), through the saved PRE-activation
 *                 z (GELU is not monotonic, so dr_act_bwd's "derivative from the output" does not exist for it).
 *   dr_bert_embed_fwd   s[n, :] = (tok[ids[n], :] + pos[n % L, :]) + seg[segment[n], :] for n < N = B*L, two fp32 additions in that
 *                 order; out[n, :] = dropout(gamma * (s - mean) * rstd + beta), mean and the POPULATION variance over the D columns,
 *                 rstd = 1 / sqrt(var + eps); dropout as dr_token_embedding_fwd: element n*D + c is kept iff dr_mix32(seed, n*D + c)
 *                 >= (uint32)min(4294967040, rate * 2^32) [always when rate == 0] and kept values are scaled by 1 / (1 - rate).
 *                 stats [N, 2] = (mean, rstd).  tok [V, D], pos [max_position, D], seg [T, D], gamma, beta [D], ids and segment int64
 *                 [N]; an id outside [0, V) or a segment outside [0, T) reads as a zero row and is never turned into an address.
 *                 Domain: D % 4 == 0, 4 <= D <= 1024, L <= max_position, N % L == 0, N < 2^31 (DR_ESHAPE otherwise); tables, gamma,
 *                 beta and out 16-byte aligned, ld_out % 4 == 0 and >= D, rate in [0, 1) (DR_EINVAL otherwise).
 *   dr_bert_embed_bwd   from d_out [N, D] (pitch ld_do), with s recomputed from the tables and the mask from the hash:
 *                 d_s [N, D] (dense) = rstd * (g gamma - mean_c(g gamma) - xhat mean_c(g gamma xhat)), g = the kept d_out / (1 - rate);
 *                 d_gamma [D] = sum_n g xhat and d_beta [D] = sum_n g, d_seg [T, D] = the sum of the d_s rows of each segment:
 *                 OVERWRITTEN, two-stage sums (128-row chunks in ascending row order, then the chunks in order);
 *                 d_pos [L, D] (the first L rows of the position table's gradient) = sum_b d_s[b*L + l, :]: OVERWRITTEN, two-stage
 *                 (16-sequence chunks);
 *                 d_tok [V, D] += the sum of d_s[n, :] over the positions with ids[n] == v in ascending n: one owner block per table
 *                 row fed by sorted_ids / order (the ids sorted by a STABLE sort and its permutation, as dr_token_embedding_bwd, whose
 *                 device code this shares).  workspace: dr_bert_embed_bwd_workspace_bytes(N, L, D, T) bytes, a function of the
 *                 shapes alone.
 *   dr_softmax_ce_ids   softmax cross-entropy over integer labels, IN PLACE: logits [M, C] (pitch ld >= C) are overwritten with the
 *                 gradient.  z = logits + bias (bias [C] or NULL), lse = log sum_j exp z_j (max-shifted), label = labels[r] (int64),
 *                 w = weight[r] (or 1), e = smoothing in [0, 1):
 *                   row_loss[r] = w ((1 - e) (lse - z_label) + e (lse - mean_j z_j))               (NOT divided by the denominator)
 *                   g[r, j]     = row_scale w / (denom ? denom[0] + denom_eps : 1) * (softmax_j - e / C - (1 - e) [j == label])
 *                 denom is a DEVICE scalar (no host read).  A row with label < 0 is padding: loss 0, its gradient row exact +0.0, its
 *                 logits never read (a NaN there reaches nothing).  label >= C breaks the contract (the row's result is unspecified;
 *                 it is not checked).  One block owns a row: up to dr_softmax_ce_ids_lds_cols() = DR_SOFTMAX_CE_IDS_LDS_COLS columns
 *                 the row is staged once in LDS, so the logits move once in and once out; a wider row is re-read from memory and
 *                 gives the same bits.  path: 0 chooses by C; 1 / 2 force the staged / the re-reading kernel (tests only; 1 with a
 *                 row too wide is DR_ESHAPE).  Rows are read as float4 when logits is 16-byte aligned and ld % 4 == 0.  Max and sums
 *                 are fixed-order reductions.
 *   dr_colsum_add       dst[j] += sum_r g[r, j] over g [M, C] (pitch ld), two-stage (32-row chunks, then the chunks in order): the
 *                 bias gradient of the above.  workspace: dr_colsum_add_workspace_bytes(M, C) bytes.
 *   dr_mlm_mask   BERT's dynamic masking, integer only and counter-based: a function of (seed, ids) alone.  Per row b of ids [B, L]:
 *                 position l is a candidate iff ids[b, l] >= num_special; n = 0 without candidates, else
 *                 min(P, max(1, (n_cand * prob_q16 + 32768) >> 16)), prob_q16 = round(prob * 65536) <= 65536.  Candidate l has the key
 *                 (uint64(dr_mix32(seed, b*L + l)) << 32) | l; the n smallest keys are chosen and written in ascending l:
 *                 positions int32 [B, P] = l, labels int64 [B, P] = the original id, both -1 beyond n.  out_ids = ids with the chosen
 *                 positions replaced by r = dr_mix32(seed + 1, b*L + l) % 10: r < 8 -> mask_id; r == 8 -> num_special +
 *                 dr_mix32(seed + 2, b*L + l) % (V - num_special); r == 9 -> unchanged.  One wave per row.  1 <= P <= 128,
 *                 V > num_special >= 0 (DR_EINVAL otherwise); 1 <= L <= 512 (L > 512: DR_ESHAPE).
 * ---------------------------------------------------------------------------------------- */
int dr_gelu_fwd(const float* z, int64_t ld_z, int64_t M, int32_t N, float* h, int64_t ld_h, dr_stream_t stream);
int dr_gelu_bwd(const float* z, int64_t ld_z, float* dy, int64_t ld_dy, int64_t M, int32_t N, dr_stream_t stream);
int dr_bert_embed_fwd(const int64_t* ids, const int64_t* segment, int64_t N, int32_t L, const float* tok, int64_t V, const float* pos,
                      int32_t max_position, const float* seg, int32_t T, const float* gamma, const float* beta, int32_t D, float eps,
                      float rate, uint64_t seed, float* out, int64_t ld_out, float* stats, dr_stream_t stream);
int64_t dr_bert_embed_bwd_workspace_bytes(int64_t N, int32_t L, int32_t D, int32_t T);
int dr_bert_embed_bwd(const int64_t* ids, const int64_t* segment, const int64_t* sorted_ids, const int64_t* order, int64_t N, int32_t L,
                      const float* tok, int64_t V, const float* pos, const float* seg, int32_t T, const float* gamma, const float* stats,
                      int32_t D, const float* d_out, int64_t ld_do, float rate, uint64_t seed, float* d_s, float* d_gamma, float* d_beta,
                      float* d_tok, float* d_pos, float* d_seg, float* workspace, int64_t workspace_bytes, dr_stream_t stream);
int dr_softmax_ce_ids(float* logits, int64_t ld, const float* bias, const int64_t* labels, const float* weight, int64_t M, int32_t C,
                      float smoothing, float row_scale, const float* denom, float denom_eps, float* row_loss, int32_t path,
                      dr_stream_t stream);
int32_t dr_softmax_ce_ids_lds_cols(void);
int64_t dr_colsum_add_workspace_bytes(int64_t M, int32_t C);
int dr_colsum_add(const float* g, int64_t ld, int64_t M, int32_t C, float* dst, float* workspace, int64_t workspace_bytes,
                  dr_stream_t stream);
int dr_mlm_mask(const int64_t* ids, int64_t B, int32_t L, int64_t V, int64_t num_special, int64_t mask_id, uint32_t prob_q16, int32_t P,
                uint64_t seed, int64_t* out_ids, int32_t* positions, int64_t* labels, dr_stream_t stream);

/* ----------------------------------------------------------------------------------------
 * IntentGC (Zhao et al., KDD 2019, arXiv:1907.12377; the reference README's model list names it, its tree has no code for it),
 * csrc/intent_conv.hip: IntentNet's vector-wise convolution over R neighbour types and L local filters.  All fp32, on the caller's
 * stream, no host synchronisation, no atomics: every result is bit-identical from run to run.
 *
 *   a_0 = h[v],  a_r = sum_k val[k] h[col[k]] over k in [row_ptr[v R + r - 1], row_ptr[v R + r])     (r = 1 .. R)
 *   p_i = sum_{r = 0 .. R} W[i, r] a_r,  g_i = relu(p_i),  s = sum_{i < L} theta_i g_i,  out[v] = act(s)
 *
 * The CSR (row_ptr int64 [n_dst R + 1], col int32, val fp32) is a typed block: virtual row v R + r - 1 holds the type-r neighbours of
 * destination v (layers.sample_typed_blocks; row-normalised, possibly empty) and the destinations are rows 0 .. n_dst - 1 of h.  W
 * [L, R + 1] and theta [L] are dense; a_r, p_i, g_i, s are D-vectors and W[i, r], theta_i scalars.  act: 0 linear, 1 relu.
 *
 *   dr_intent_conv_fwd  gathers a_1 .. a_R as dr_csr_spmm gathers a row (ascending k, the same bits on any row that kernel does not
 *                       split; here rows of ANY length are summed in ascending k, there is no split), applies the filters in registers
 *                       and writes out [n_dst, D] (pitch ld_out).  agg non-NULL: also stores a_1 .. a_R as [n_dst, R, D], dense.
 *   dr_intent_mix_fwd   the same body with a_r read from agg [n_dst, R, D] (pre-aggregated rows; adj.spmm's output over a whole
 *                       graph) and a_0 from h_self (pitch ld_h): the same out bits from the same a_r bits.
 *   dr_intent_conv_bwd  from h_self, agg, d_out (pitch ld_do) and optionally the forward's out (pitch ld_out; NULL: s is recomputed,
 *                       the same bits): d_self [n_dst, D] (pitch ld_ds) = d_a_0, d_agg [n_dst, R, D] = d_a_r (the caller scatters it
 *                       with the transposed block), d_W [L, R + 1] and d_theta [L], all OVERWRITTEN.
 *                         ds = d_out * act'(s),  d_theta_i = sum_{v, c} ds g_i,  dp_i = [p_i > 0] theta_i ds,
 *                         d_W[i, r] = sum_{v, c} dp_i a_r,  d_a_r = sum_i W[i, r] dp_i
 *                       d_W / d_theta are two-stage sums: per-block partials in the workspace (lanes by a fixed butterfly, destinations
 *                       in ascending order), then the blocks in order.  The grid is a function of (n_dst, D) alone.
 *                       workspace: dr_intent_conv_bwd_workspace_bytes(n_dst, D, R, L) bytes (-1 outside the domain).
 *   Order of every sum: p_i over ascending r, s and d_a_r over ascending i, each an fmaf chain from +0.
 *   Domain: D % 4 == 0, 4 <= D <= 256, 1 <= R <= 7, 1 <= L <= 16 (DR_ESHAPE otherwise); act in {0, 1}, pitches multiples of 4 and
 *   >= D, every matrix 16-byte aligned (DR_EINVAL otherwise).  Outside the domain nothing is launched; n_dst == 0 returns DR_OK and
 *   launches nothing (d_W and d_theta are then not written).
 * ---------------------------------------------------------------------------------------- */
int dr_intent_conv_fwd(const int64_t* row_ptr, const int32_t* col, const float* val, int64_t n_dst, int32_t R, const float* h,
                       int64_t ld_h, int32_t D, const float* W, const float* theta, int32_t L, int32_t act, float* out, int64_t ld_out,
                       float* agg, dr_stream_t stream);
int dr_intent_mix_fwd(const float* h_self, int64_t ld_h, const float* agg, int64_t n_dst, int32_t R, int32_t D, const float* W,
                      const float* theta, int32_t L, int32_t act, float* out, int64_t ld_out, dr_stream_t stream);
int64_t dr_intent_conv_bwd_workspace_bytes(int64_t n_dst, int32_t D, int32_t R, int32_t L);
int dr_intent_conv_bwd(const float* h_self, int64_t ld_h, const float* agg, const float* d_out, int64_t ld_do, const float* out,
                       int64_t ld_out, const float* W, const float* theta, int64_t n_dst, int32_t R, int32_t D, int32_t L, int32_t act,
                       float* d_self, int64_t ld_ds, float* d_agg, float* d_W, float* d_theta, void* workspace,
                       int64_t workspace_bytes, dr_stream_t stream);

/* dr_clock_stamp: dst[0] = the device's constant-rate wall clock (100 MHz ticks) when a one-thread kernel reaches the head of
 * `stream`.  Measurement plumbing with no reference counterpart: bench.py brackets the sharded step's cross-stream waits with two
 * stamps to report the EXPOSED part of the exchange (HIP timing events around a wait serialise the step). */
int dr_clock_stamp(uint64_t* dst, dr_stream_t stream);

/* Measurement plumbing: dst[0 .. bytes) = src[0 .. bytes) as a streaming copy of 16-byte vectors with nontemporal loads / stores
 * (bytes a multiple of 16, both pointers 16-byte aligned; DR_EINVAL otherwise).  bench.py times it over 1 GiB as the
 * `measured_copy_ceiling` beside the 8 TB/s spec peak: read + write bytes / time is what an HBM-bound kernel can reach on that box. */
int dr_copy_nt(const void* src, void* dst, int64_t bytes, dr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DR_HOTPATH_H */
