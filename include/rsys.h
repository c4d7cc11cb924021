/* rsys.h -- C ABI of the MI355X-native training hot path (librsys_hip.so).
 *
 * Drop-in boundary for the data-parallel training step of Fro116/RecommenderSystem
 * (reference files: notebooks/Training/transformer.model.py = "model.py",
 * notebooks/Training/transformer.py = "train.py").  The reference has no FFI of its
 * own; each entry point below names the reference
 * interface it replaces.  A Julia host binds these with `ccall`, a Python host with
 * ctypes (recommendersystem_amd/_lib.py); INTEGRATION.md shows both stubs.
 *
 * Conventions: every function returns 0 on success, <0 on error
 * (rsys_last_error gives the thread-local message).  Handles are opaque.  The caller
 * owns every host buffer; the library owns all device memory.  Calls on one handle
 * must be serialised by the caller; one handle set per GPU (one process per GPU as
 * in train.py:582-587).  No callbacks, no exceptions cross the boundary.
 */
#ifndef RSYS_H
#define RSYS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsys_model rsys_model;
typedef struct rsys_optimizer rsys_optimizer;
typedef struct rsys_comm rsys_comm;

/* RSYS_DTYPE_FP8: bf16 arithmetic with the transformer blocks' linears (q k v o w1 w3 w2: forward and input-gradient products) on
 * tensor-wise dynamically scaled fp8 operands -- the reference's pretraining arithmetic (transformer.py:671-676, torchao
 * "tensorwise": e4m3 inputs and weights, e5m2 output gradients); pretraining only, needs embed_dim % 128 == 0 >= 256,
 * (num_kv_heads * head_dim) % 128 == 0, num_heads / num_kv_heads <= 14 (the hidden width is padded to a multiple of 128 inside) */
enum { RSYS_DTYPE_FP32 = 0, RSYS_DTYPE_BF16 = 1, RSYS_DTYPE_FP8 = 2 };

/* mirrors the config dict of train.py:535-560 (+ finetune keys of :520-524) */
typedef struct rsys_config {
  int32_t num_layers, num_heads, num_kv_heads, embed_dim, intermediate_dim;
  int32_t max_sequence_length;          /* S interactions per row -> 2S tokens; a multiple of 4, S <= 2048 (rows of up to 4096 tokens) */
  int32_t vocab_0, vocab_1;             /* vocab_sizes["0_matchedid"], ["1_matchedid"] */
  int32_t vocab_status, vocab_gender, vocab_source;
  int32_t metadata_dim;                 /* metadata_emb_size */
  double min_ts, max_ts;
  float rating_mean, rating_std;
  float mask_rate;
  int32_t mask_topk;
  int32_t finetune;                     /* 0/1 */
  int32_t finetune_metric;              /* 0 = watch, 1 = rating */
  int32_t dtype;                        /* RSYS_DTYPE_* : arithmetic type of the dense contractions */
  int32_t max_rows;                     /* rows (of S interactions) per forward call = local batch size */
  float lora_dropout;                   /* finetune only: nn.Dropout(p) on the LoRA input (model.py:238); 0 disables */
  /* row-sharded item table (beyond the reference): world 0 = replicated table (the reference's scheme,
   * transformer.py:678-682); world >= 1: this rank owns table rows [rank*(V+1)/world, (rank+1)*(V+1)/world) of the item
   * embedding, the metadata table, the fused table and their Adam moments; rsys_model_set_shard_comm gives the communicator */
  int32_t table_shard_rank, table_shard_world;
  /* row-sharded table only: > 0 replaces the full soft-max of the watch heads by a sampled one -- per step and medium every
   * rank draws this many of its local classes (stratified uniform) and the partition function is estimated by importance
   * weighting (log-Q correction), the target class always included.  0 = full soft-max (the reference, model.py:514-519). */
  int32_t sampled_negatives;
} rsys_config;

/* the batch record of train.py:75-98 / transformer.jl:79-142: 27 parallel arrays of
 * rows*S interactions.  Index of label/weight/position: medium*3 + {0 watch,1 rating,2 status}. */
typedef struct rsys_batch {
  int32_t rows;
  const int32_t *userid, *token_mask_ids, *gender, *source, *matchedid, *status;
  const double* time;
  const float *rating, *progress;
  const float* label[6];
  const float* weight[6];
  const int32_t* position[6];
  const uint8_t* watch_mask;   /* optional (parity mode): replaces the random draw of model.py:437-440 */
  const uint8_t* rating_mask;  /* optional, with watch_mask */
  const int32_t* rope_input_pos; /* optional (inference, model.py:470-476) */
} rsys_batch;

const char* rsys_version(void);
size_t rsys_last_error(char* buf, size_t n);
int32_t rsys_device_count(int32_t* n);
int32_t rsys_device_synchronize(void);

/* RecommenderModel(config) -- model.py:346-377.  Parameters are zero until set or
 * rsys_model_init_random (init_weights, model.py:5-12) is called. */
int32_t rsys_model_create(const rsys_config* cfg, int32_t device, rsys_model** out);
int32_t rsys_model_destroy(rsys_model* m);
int32_t rsys_model_init_random(rsys_model* m, uint64_t seed);
/* load_pretrained_embeddings -- model.py:379-389; table is (V, M) row-major f32 */
int32_t rsys_model_load_metadata(rsys_model* m, const float* table, int64_t V, int64_t M);
/* synthetic frozen table generated on the device: N(0,1)/sqrt(M) */
int32_t rsys_model_random_metadata(rsys_model* m, uint64_t seed);
/* RoPE tables precompute_freqs_cis -- model.py:173-179; (n_pos, head_dim/2) f32 each */
int32_t rsys_model_set_rope(rsys_model* m, const float* cos, const float* sin, int64_t n_pos);

/* state_dict interchange -- names are the reference's state_dict keys */
int32_t rsys_param_count(rsys_model* m, int32_t* n);
int32_t rsys_param_info(rsys_model* m, int32_t i, char* name, size_t name_cap, int64_t shape[2], int32_t* ndim,
                        int32_t* trainable);
int32_t rsys_param_get(rsys_model* m, const char* name, float* out, int64_t n);
int32_t rsys_param_set(rsys_model* m, const char* name, const float* in, int64_t n);
int32_t rsys_grad_get(rsys_model* m, const char* name, float* out, int64_t n);
int32_t rsys_zero_grad(rsys_model* m);

/* to_device -- train.py:178-184: copies the batch into device-resident buffers */
int32_t rsys_batch_upload(rsys_model* m, const rsys_batch* b);
/* The reference's loader overlap (DataLoader workers + non_blocking to_device, train.py:162-165,178-184): rsys_batch_prefetch checks
 * and packs the NEXT batch on the calling thread and copies it on a stream of its own while the current step still runs on the
 * device (a second staging buffer / device blob); rsys_batch_swap then makes it the resident batch -- enqueue the step's forward /
 * backward / optimizer first, prefetch, read the step's losses, swap.  The host arrays may be freed when prefetch returns.
 * Replicated item table only (the row-sharded table builds its row-exchange plan inside rsys_batch_upload). */
/* rows of the resident batch (0: none), whichever call made it resident */
int32_t rsys_batch_rows(rsys_model* m, int32_t* rows_out);
int32_t rsys_batch_prefetch(rsys_model* m, const rsys_batch* b);
int32_t rsys_batch_swap(rsys_model* m);
/* Inference on trimmed rows (beyond the reference, whose server always runs rows of max_sequence_length).  A serving row
 * holds one user: its live events are a prefix, everything behind them is padding with userid 0 (Finetune/embed.py:86-123).  The mask's
 * first predicate is userid[q] == userid[kv] (transformer.model.py:479-480), so no live token attends padding, and every other operator
 * of the trunk is token-local: dropping the padding columns is exact.
 * rsys_batch_upload_trimmed is rsys_batch_upload for such rows: the arrays keep the caller's row stride S = max_sequence_length, only
 *   columns [0, row_len) of each row are read, checked, packed and copied; the resident batch then has rows of row_len interactions
 *   (2 row_len tokens) and every forward over it launches its kernels for rows * 2 row_len tokens.  row_len % 4 == 0 and
 *   4 <= row_len <= S; row_len == S is rsys_batch_upload, with everything that call requires.  Every column >= row_len of every row must have userid == 0: checked on the host
 *   before anything is written, as the index paths are (RSYS_ERR_ARG: the resident batch and its row length stay as they were).  rope_input_pos
 *   (may be NULL: the column) is a position, bounded by the RoPE tables as in rsys_batch_upload, not by row_len: the candidate rows of the
 *   ranking cache sit at position n_hist, whatever their length.  The label, weight, position and mask arrays are not read and may be NULL.  fp32 and bf16 models with a replicated table; an fp8 model
 *   (its tensor-wise amax sees every token) and a row-sharded table return RSYS_ERR_ARG.
 * On a trimmed batch: rsys_infer returns [rows][2 row_len][D] (n is checked against that); rsys_infer_select[_adapters] keep the caller's
 *   token geometry r * 2S + t, a t >= 2 row_len is RSYS_ERR_ARG; rsys_rank_cache_store takes n_hist <= row_len and
 *   rsys_rank_cache_candidates n_cand <= row_len -- the slot layout does not change, so a slot stored from a trimmed row serves candidate
 *   rows of any length and the reverse; rsys_forward_backward, rsys_adapter_forward_backward and every pass that reads targets return
 *   RSYS_ERR_STATE ("a trimmed batch is inference-only") and touch nothing.  The next rsys_batch_upload / _swap restores the full rows.
 * rsys_batch_row_length: interactions per row of the resident batch: S after an ordinary upload, 0 without a batch.
 * rsys_serving_trim_set (default 0; read by rsys_render_request and rsys_render_request_full only): every forward of those pipelines
 *   runs at row_len = min(S, 32 ceil(longest live row of that forward / 32)) -- whole 64-token attention tiles.  Waves, chunks, slots
 *   and outputs are unchanged; with the switch off every launch is what it was.
 * rsys_serving_pack_set (default 0; read by rsys_render_request and rsys_render_request_full only): the retrieval stage of
 *   those pipelines runs several users per row.  A user's live columns (through its query token) become a segment that starts at a
 *   column that is a multiple of 32 and lies inside one row; users are placed first-fit in decreasing length, ties in user order, and
 *   a forward is max_rows such rows at row_len = min(S, 32 ceil(its fullest row / 32)), whatever rsys_serving_trim_set says.  Each
 *   segment runs with the adapter slot of its own medium (one slot per 64-token tile).  A retrieval row must hold one user (one userid
 *   beside 0: RSYS_ERR_ARG otherwise).  Q and everything after it is in user order as before: pages, totals, ranking waves, store
 *   rows, slots and chunks are unchanged; "forward_rows" reports the packed forwards as (0, rows, row_len).
 * rsys_serving_pack_ranking_set (default 0; read by rsys_render_request_full only): the K/V-cache store rows of that pipeline
 *   hold several users.  A store wave is up to rc_slots users with a history (the model's reserve, rsys_rank_cache_reserve; at least
 *   max_rows), slot = the user's place in the wave.  Its histories become segments that start at a column that is a multiple of 32, placed
 *   first-fit in decreasing length, ties in user order, rows in the order they were opened, forwards of max_rows rows at row_len =
 *   min(S, 32 ceil(fullest row / 32)) -- if that takes fewer forwards than one history per row at that row's trim length, or as many
 *   forwards and fewer tokens; otherwise one history per row, at column 0.  The rows are cut on the device from the kept history rows
 *   and stored as rsys_rank_cache_store_packed stores them, without a host wait.  Candidate forwards, the empty-history rows, chunking,
 *   pages and totals are unchanged; "forward_rows" reports the packed store forwards as (1, rows, row_len).
 * rsys_serving_compact_top_set (default 0): inference passes run the last layer only where its outputs are read.  Read by
 *   every inference pass over the resident batch: rsys_infer_select[_adapters | _tiles], the render pipelines' retrieval and ranking
 *   forwards, and the four rsys_rank_cache_* passes.  A pass that reports n selected tokens with n <= the compact buffers' rows and
 *   2 n <= the batch's tokens runs the last layer's output projection, MLP and the final norm on those n rows only (token order is kept);
 *   when also n <= rows * ceil(2 row_len / 64) and the rows are not candidate rows, that layer's attention runs for the selected queries
 *   only.  A store pass (rsys_rank_cache_store[_packed]) ends after its last K | V copy; the slots hold the same bits.  Needs the
 *   compact buffers (an fp32 / bf16 model with a replicated table and at most 2^19 tokens per batch): otherwise, and for rsys_infer
 *   without a selection, the pass runs dense as before.  Values agree with the dense pass to rounding (the order of two sums changes), not
 *   bit for bit.  rsys_trunk_output_get after such a pass computes the dense output on demand.  With the switch off every launch is what
 *   it was.  on = 2 / 3 are measurement values (tools/bench_compact_top.py): as 1, with the attention rule forced to "never" / "always". */
int32_t rsys_batch_upload_trimmed(rsys_model* m, const rsys_batch* b, int32_t row_len);
int32_t rsys_batch_row_length(rsys_model* m, int32_t* row_len_out);
int32_t rsys_serving_pack_set(rsys_model* m, int32_t on);
int32_t rsys_serving_pack_get(rsys_model* m, int32_t* on_out);
int32_t rsys_serving_pack_ranking_set(rsys_model* m, int32_t on);
int32_t rsys_serving_pack_ranking_get(rsys_model* m, int32_t* on_out);
int32_t rsys_serving_compact_top_set(rsys_model* m, int32_t on);
int32_t rsys_serving_compact_top_get(rsys_model* m, int32_t* on_out);
int32_t rsys_serving_trim_set(rsys_model* m, int32_t on);
int32_t rsys_serving_trim_get(rsys_model* m, int32_t* on_out);
/* device-side synthetic batch (bench): fills the resident batch from a counter RNG */

/* model(d, evaluate) + loss.backward() -- model.py:493-529, train.py:259-272.
 * task_w[4] in the order (0,watch),(0,rating),(1,watch),(1,rating); the gradient of
 * sum_i task_w[i]*loss_i*grad_scale is ACCUMULATED into the gradient buffer (skipped
 * when evaluate != 0).  mask_seed/step drive the Philox mask draw when the batch
 * carries no explicit masks.  Asynchronous: results are read with rsys_losses_get. */
int32_t rsys_forward_backward(rsys_model* m, int32_t evaluate, const float task_w[4], float grad_scale,
                              uint64_t mask_seed, uint64_t step);
/* losses_out[12]: per task 3 slots (train: [loss,0,0]; evaluate rating tasks: 3 moments of model.py:395-401);
 * weight_sums_out[4]: d[name.weight].sum() after masking (train.py:261).  Synchronises. */
int32_t rsys_losses_get(rsys_model* m, float losses_out[12], float weight_sums_out[4]);
/* The same without a host wait per step (transformer.py:245-262 adds the losses into device tensors and reads them at the end of the
 * epoch, :279-283): rsys_losses_push parks the finished step's sums on the device (stream-ordered, at most 1024 steps),
 * rsys_losses_drain synchronises once and writes every parked step in order: losses_out[n][12], weight_sums_out[n][4] as
 * rsys_losses_get would have returned them; *n_out = n <= cap. */
int32_t rsys_losses_push(rsys_model* m);
int32_t rsys_losses_drain(rsys_model* m, float* losses_out, float* weight_sums_out, int32_t cap, int32_t* n_out);
/* number of positive-weight positions selected per task in the last forward (they bound the head GEMMs) */
int32_t rsys_head_rows_get(rsys_model* m, int32_t out[4]);
/* ItemEmbedding.forward over all items (model.py:139-145), the table Finetune/register.py:27-33 exports as the watch-head
 * weights of the serving registry: out [V][embed_dim] f32, V = vocab_0 + vocab_1 (manga rows first) */
int32_t rsys_item_table(rsys_model* m, float* out, int64_t n);
/* Retrieval candidates for a batch of query embeddings (Finetune/embed.jl:86-90 + the scoring, masking and sort of
 * Inference/render.jl:240-333), on the model's fused item table of `medium` (the tied watch head, model.py:148-170).
 * Ids are medium-local, in [0, V_m) (V_m = vocab_0 or vocab_1).  z_q[i] = F_m[i] . u_q accumulated in fp32 on operands of the model's
 * compute dtype (bf16 mode: the query rounded to bf16, the bf16 table copy); lse_q = log sum_{i < V_m} exp z_q[i] over every item;
 * score_g[i] = prior_g[i] + sum over the queries q of group g, in query order, of (z_q[i] - lse_q).  Excluded from group g: the ids of
 * its exclusion list (duplicates allowed) and ids whose score is -inf or NaN; -0.0 ranks as +0.0.  Output per group: the min(k,
 * admissible) best ids by descending score, ties by ascending id (render.jl's stable sortperm(p, rev=true) without the -Inf entries),
 * counts_out[g] = that number, the slots after it id -1 and score -inf.  1 <= n_queries <= 4096, 1 <= k <= min(V_m, 8192), every group
 * needs a query, replicated table only.  Works without an uploaded batch (rebuilds the fused table when stale) and changes no model
 * state; synchronous, bitwise reproducible; the device workspace grows on demand and is freed with the model. */
int32_t rsys_retrieve_topk(rsys_model* m, int32_t medium,
                           const float* queries, int64_t n_queries,          /* [n_queries][embed_dim] f32, host */
                           const int32_t* group, int32_t n_groups,           /* [n_queries] in [0, n_groups), or NULL: group = query */
                           const float* prior,                               /* [n_groups][V_m] f32 added to the score, or NULL */
                           const int64_t* excl_offsets, const int32_t* excl_ids, /* CSR over groups of medium-local ids, or both NULL */
                           int32_t k, int32_t* ids_out, float* scores_out,   /* [n_groups][k] each */
                           int32_t* counts_out);                             /* [n_groups] */
/* Finetune evaluation (Finetune/regress.jl:193-266): per query q the rank and log-probability of one target item t_q, on the scores of
 * rsys_retrieve_topk.  s_i = z_q[i] - lse_q in fp32, bit for bit the score rsys_retrieve_topk gives item i for a one-query group
 * without prior (lse_q over every item of the medium, exclusions included).  logp_out[q] = s_{t_q}, read before any exclusion.
 * Admissible: not in q's exclusion list (duplicates allowed) and s_i neither NaN nor -inf; -0.0 equals +0.0.
 * rank_out[q] = 1 + #{i admissible : s_i > s_t} + #{i admissible, i < t : s_i == s_t}, the 1-based position of t in Julia's
 * partialsortperm(logp, rev=true) (ties by ascending id) and in rsys_retrieve_topk's order; 0 when t itself is not admissible.
 * 1 <= n_queries <= 4096, replicated table only.  Works without an uploaded batch (rebuilds the fused table when stale) and changes no
 * model state; synchronous, bitwise reproducible; the device workspace grows on demand and is freed with the model.  ARG errors: a
 * target or exclusion id outside [0, V_m), malformed offsets, a bad medium. */
int32_t rsys_retrieve_target_rank(rsys_model* m, int32_t medium,
                                  const float* queries, int64_t n_queries,          /* [n_queries][embed_dim] f32, host */
                                  const int32_t* targets,                           /* [n_queries] medium-local, in [0, V_m) */
                                  const int64_t* excl_offsets, const int32_t* excl_ids, /* CSR over queries of medium-local ids, or both NULL */
                                  int32_t* rank_out, float* logp_out);              /* [n_queries] each */
/* The serving tables of rsys_retrieve_request (Inference/render.jl:240-331, `retrieval(state)`), held on the device by the model, freed with
 * it, not part of checkpoints; loading them changes nothing else (the fused item table stays valid).  Every setter replaces the table;
 * a NULL array clears it.
 * Relations of medium m: kind 0 = "{m}.dependencies" (V_m x V_m), 1 = "{m}.recaps" (V_m x V_m), 2 = "{m}.adaptations" (V_m x V_{1-m}),
 * as 0-based CSC in Julia's column order (colptr[n_cols + 1] with colptr[0] = 0, non-decreasing; rowval in [0, n_rows)).  Stored
 * values must be finite and >= 0 (else an ARG error); explicitly stored zeros are dropped, so "product != 0" is reachability along the
 * stored pattern. */
int32_t rsys_retrieve_relations_set(rsys_model* m, int32_t medium, int32_t kind, int64_t n_rows, int64_t n_cols,
                                    const int64_t* colptr, const int32_t* rowval, const float* nzval);
/* item similarity of medium m: emb = "embeddings.{m}" ([V_m][dim] f32: Julia's dim x V_m), crossproject = "crossproject.{m}" (dim x dim,
 * column-major as Julia holds it, maps medium m into medium 1 - m; NULL: not loaded).  dim a multiple of 4 in [4, 2048].
 * emb == NULL clears both. */
int32_t rsys_retrieve_similarity_set(rsys_model* m, int32_t medium, int64_t dim, const float* emb, const float* crossproject);
/* released items of medium m: mask[V_m], nonzero = released (render.jl's `keys(get_media_info(m))`); NULL: every item released */
int32_t rsys_retrieve_released_set(rsys_model* m, int32_t medium, const uint8_t* mask);
/* Query weights of the NEXT request (the reference's roadmap: "inference: allow weighting different queries"): a finite f32
 * weight per user and per selected item of the request's states, in the call's user order and in the order of sel_ids.  One call instead of
 * a weighted twin of each of the six request entry points.  The arrays are copied on the host and held by the model until the next call of
 * rsys_retrieve_request, rsys_retrieve_window, rsys_rank_request, rsys_render_request, rsys_render_request_full or rsys_render_items, which
 * consumes them: they are cleared when that call returns, on success and on error alike.  No other entry point (rsys_retrieve_topk included)
 * reads or clears them.  (NULL, 0) for a kind = unweighted for that kind; (NULL, 0, NULL, 0) clears both; a call replaces what was held.
 * The consuming call checks the counts before anything else -- n_users against its n_queries / n_users, n_sel against
 * sel_offsets[n_groups] (0 without sel_offsets) -- and a mismatch is RSYS_ERR_ARG with outputs untouched.  rsys_rank_request takes no
 * selected-item weights and rsys_render_items no user weights (RSYS_ERR_ARG); rsys_rank_request with r_in reads no weights but consumes
 * them.  A weight that is NaN or infinite: RSYS_ERR_ARG, and nothing is held.
 * Semantics: weights scale score terms only, every operation rounded in fp32 on its own (no fused multiply-add), so a float32 restatement
 * is bit-exact --
 *   selected sum   s_g = s_g + w_a * x_a in list order (x_a = E_m[id] or crossproject.{am} E_am[id]); the prior E_m^T s_g as without weights
 *   retrieval      score = score + w_q * (z_q[i] - lse_q) in query order
 *   ranking        score = score + w_u * (lp_u + r_u) in user order, lp_u and r_u as rsys_rank_request forms them
 * A weight of +0.0 or -0.0 skips the term: the running sum keeps its bits, so 0 * -inf never makes a NaN.  Negative weights are allowed
 * ("less like B"; a thumbs-down).  With every weight 1.0 each result equals the unweighted call's bit for bit; without pending weights of a
 * kind the unweighted kernels run.  Masks and flags ignore the weights: a user vetoes its watched items, adaptations, recaps, missing
 * dependencies and sequels whatever its weight, a selected item of the request's medium is masked whatever its weight, the related flags
 * read every user's list; totals change only where a score becomes NaN or -inf.  Inside rsys_render_request / _full the same weights reach
 * the retrieval stage and the ranking stage of every wave (packed, trimmed and compact-topped alike: those change which forwards run, not
 * the score kernels); no forward is skipped for a zero-weight user. */
int32_t rsys_query_weights_set(rsys_model* m, const float* user_w, int64_t n_users,   /* [n_users], or NULL with 0 */
                               const float* sel_w, int64_t n_sel);                    /* [n_sel], or NULL with 0 */
/* out = (n_users, n_sel) of the weights the model holds for the next request, 0 = none of that kind */
int32_t rsys_query_weights_pending(rsys_model* m, int64_t out[2]);
/* Text queries of the NEXT request (the reference's roadmap: "Natural language queries" beside "Multiquery recs"): n_texts
 * query embeddings x [n_texts][Q] (host f32) of the search handle `search` (rsys_search_*, features set, on the model's device, its V_m the
 * model's for `medium`), each for one group of the consuming call and with a finite weight (w == NULL: 1.0 each).  The call scores them on
 * the search handle's stream, with one wait -- P = x Wenc as rsys_search_topk forms it, then one streaming pass over E_m per tile of up
 * to 8 texts (text_scores_kernel; 4 texts above D = 2048, 2 above 4096: the tile's fp32 rows stay within 64 KiB of LDS), z_t[i] = (P_t . E_m[i]) * exp(logit_scale) for i < V_m in fp32, and lse_t = log sum_i exp(z_t[i]) by
 * the launches of rsys_op_lse -- into a buffer the model owns, and the model holds rows, lse, groups and weights of that medium until the
 * next call of rsys_retrieve_request, rsys_retrieve_window, rsys_rank_request, rsys_render_request, rsys_render_request_full or
 * rsys_render_items, which consumes the sets of BOTH media: they are gone when that call returns, on success and on error alike.  No other
 * entry point (rsys_retrieve_topk and rsys_search_* included) reads or clears them.  One set per medium; a call replaces that medium's
 * set, n_texts == 0 clears it (the other arguments are then not read); 1 <= n_texts <= min(64, the handle's max_batch).
 * RSYS_ERR_ARG, with nothing held for that medium afterwards: a null handle, a handle on another device, a V_m that is not the model's,
 * features never set, null x or group, a non-finite x or w; a medium that is not 0 or 1 (nothing changes).
 * The consuming call checks, before anything else, every text's group against its n_groups, and in the page pipelines against
 * group_medium (a text of medium m belongs to a group of medium m); a call on one medium refuses a set of the other.  Each is RSYS_ERR_ARG
 * with outputs untouched.
 * Semantics, every operation rounded in fp32 on its own (weighted_add: no fused multiply-add), a weight of +-0.0 skips its term --
 *   retrieval   after the prior and before the masks: score_g[i] = score_g[i] + w_t * (z_t[i] - lse_t) over the group's texts in text
 *               order, then the users' terms exactly as without texts.  A group without users (rsys_retrieve_window, rsys_render_items)
 *               is scored by prior + texts.  Texts carry no masks and no flags.
 *   ranking     r[c] = +0.0, then r[c] = r[c] + w_t * (z_t[id_c] - lse_t) in text order (rank_text_kernel), then the users' terms onto it;
 *               no coefficient and no rating term apply to a text.  With r_in the texts are consumed and not read.  rsys_render_items
 *               keeps r = +0.0: its retrieval order already carries the texts.
 * The page pipelines hand each medium's set to that medium's retrieval and ranking stages, groups renumbered as the stages number them. */
int32_t rsys_query_texts_set(rsys_model* m, void* search, int32_t medium,
                             const float* x, int64_t n_texts,      /* [n_texts][Q] f32, host */
                             const int32_t* group,                 /* [n_texts], group of the consuming call */
                             const float* w);                      /* [n_texts] or NULL = 1.0 */
/* out[m] = the texts the model holds for medium m for the next request, 0 = none */
int32_t rsys_query_texts_pending(rsys_model* m, int64_t out[2]);
/* A whole render.jl `retrieval(state)` per group of queries, on the tables above: score_g = p_g + the rsys_retrieve_topk score, where
 * p_g = E_m^T s_g, s_g = sum over the group's selected items in list order of E_m[id] (same medium) or crossproject.{am} E_am[id] (fp32
 * throughout; 0 without selected items).  Masked for group g (render.jl:255-331): item 0; the group's selected items of medium m; items
 * not released; and for any user of the group, with its list reduced to the last status per (medium, id): W_m = ids of medium m whose
 * status is not 3 / 5, W_o = the same of medium 1 - m, C_m = status >= 7, K_m = status 6 / 2 / 1 -- item i if i in W_m, or
 * (Adapt W_o)[i] != 0 and (Dep W_m)[i] == 0, or (Recap W_m)[i] != 0, or Dep row i is non-empty and (Dep C_m)[i] == 0, or (Dep K_m)[i] != 0.
 * Output, limits and guarantees as rsys_retrieve_topk.  The three relation tables of `medium` must be loaded; selected items need the
 * similarity table of their medium (and its crossproject when it is not `medium`) and that of `medium`.  ARG errors: missing tables,
 * ids out of range for their medium, malformed offsets. */
int32_t rsys_retrieve_request(rsys_model* m, int32_t medium,
                              const float* queries, int64_t n_queries,        /* [n_queries][embed_dim] f32 */
                              const int32_t* group, int32_t n_groups,         /* [n_queries] in [0, n_groups), or NULL: group = query */
                              const int64_t* hist_offsets,                    /* [n_queries + 1] CSR over queries, or NULL (no lists) */
                              const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status, /* list items in list order */
                              const int64_t* sel_offsets,                     /* [n_groups + 1] CSR over groups, or NULL (none selected) */
                              const int32_t* sel_medium, const int32_t* sel_ids,
                              int32_t k, int32_t* ids_out, float* scores_out, /* [n_groups][k] each */
                              int32_t* counts_out);                           /* [n_groups] */
/* rsys_retrieve_request for any rank range: per group the items whose rank in the request's ordering (descending score, ties by ascending
 * id, -0.0 as +0.0, NaN and -inf inadmissible) lies in [win_start[g], win_start[g] + win_len[g]), 1 <= win_len <= 1024, and the exact
 * number of admissible items -- what render.jl:450-463 needs for `total` and for a page at any offset.  The arguments of
 * rsys_retrieve_request with k replaced by the windows.  A group may have no queries, and n_queries may be 0 with queries == NULL: 1 <=
 * n_groups <= 4096, not bounded by n_queries.  A group without queries (render.jl:243-252, a state without users) is scored by the prior
 * p_g alone, in the same fp32 arithmetic (+0.0 everywhere without selected items), under the item-0, selected-item and released masks; it
 * has no relation masks.  Groups with queries get bit for bit the scores of rsys_retrieve_request.
 * Output: ids_out / scores_out [n_groups][1024], best first, slots past counts_out[g] = clamp(total_g - win_start[g], 0, win_len[g]) hold
 * -1 / -inf; total_out[g] = the admissible items of group g.  Device candidate storage is n_groups x 1024 whatever win_start is.  Tables:
 * as rsys_retrieve_request, but the relation tables only when n_queries > 0, and neither the item table nor a forward when n_queries == 0.
 * Synchronous, bitwise reproducible, no side effects.  RSYS_ERR_ARG (outputs untouched): win_len outside [1, 1024], win_start < 0, and
 * whatever rsys_retrieve_request rejects. */
int32_t rsys_retrieve_window(rsys_model* m, int32_t medium,
                             const float* queries, int64_t n_queries,        /* [n_queries][embed_dim] f32, or NULL with n_queries == 0 */
                             const int32_t* group, int32_t n_groups,         /* [n_queries] in [0, n_groups), or NULL: group = query */
                             const int64_t* hist_offsets,                    /* [n_queries + 1] CSR over queries, or NULL (no lists) */
                             const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                             const int64_t* sel_offsets,                     /* [n_groups + 1] CSR over groups, or NULL (none selected) */
                             const int32_t* sel_medium, const int32_t* sel_ids,
                             const int64_t* win_start, const int32_t* win_len, /* [n_groups] each */
                             int32_t* ids_out, float* scores_out,            /* [n_groups][1024] each */
                             int32_t* counts_out, int32_t* total_out);       /* [n_groups] each */
/* A page for states without users in one device pipeline (Inference/compute.jl:490-514 `/add_item` + render.jl:437-474):
 * "pick a title, see similar titles".  Group g, media mixed: group_medium[g], pagination (offset[g] >= 0, 1 <= limit[g] <= 1024),
 * penalties[g][4] as rsys_rank_request, selected items as CSR over groups in the shape of rsys_retrieve_request (NULL: none).  Per group:
 * the window of render.jl:448-463 from the exact total (mitr = 1024 - 1024 % limit, start = offset / mitr * mitr, mitr ranks, clamped to
 * the total), rsys_retrieve_window without queries, then the reranking of rsys_rank_request on r = +0.0 (render.jl:354) without related
 * flags, partialk = the page's last index.  Candidates stay on the device; counts, pages and totals come back.
 * Output as rsys_render_request, except that total_out[g] is exact (the admissible items, not capped at 8192) and a page exists for every
 * offset below it; a page starting at or past the total is empty.  Needs the similarity table of every medium involved (and the
 * crossproject of the other medium when a selected item crosses media) and the related table; no relation tables, no item table, no
 * forward.  Any dtype.  Synchronous, bitwise reproducible; the resident batch, parameters, gradients and optimizer state are not touched.
 * RSYS_ERR_ARG (outputs untouched): a bad medium, limit outside [1, 1024], offset < 0, malformed offsets, ids out of range, missing
 * tables, ids_cap below the sum of the limits. */
int32_t rsys_render_items(rsys_model* m, int32_t n_groups,
                          const int32_t* group_medium, const int64_t* offset, const int32_t* limit,   /* [n_groups] each */
                          const float* penalties,                                  /* [n_groups][4] */
                          const int64_t* sel_offsets,                              /* [n_groups + 1] CSR over groups, or NULL (none selected) */
                          const int32_t* sel_medium, const int32_t* sel_ids,
                          int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out);
/* "{m}.related" of Inference/render.jl's reranking (the franchise relation, V_m x V_m) for rsys_rank_request: 0-based CSC in Julia's column
 * order, with the contract and validation of rsys_retrieve_relations_set (colptr[n + 1], colptr[0] = 0, non-decreasing; rowval in [0, n);
 * stored values finite and >= 0, else an ARG error; explicitly stored zeros are dropped).  n must be V_m.  NULL colptr clears the table.
 * Held on the device, freed with the model, not part of checkpoints. */
int32_t rsys_rank_related_set(rsys_model* m, int32_t medium, int64_t n, const int64_t* colptr, const int32_t* rowval, const float* nzval);
/* render.jl `ranking(state, idxs)` + `reranking!(state, idxs, r, partialk)` for n_groups requests of one medium.
 * Group g: candidates ids[cand_offsets[g] .. cand_offsets[g + 1]) (medium-local, distinct, 1 <= n_g <= 1024), partialk[g] >= 1 (min(partialk,
 * n_g) rounds), penalties[g][4] = (decay, mmr_penalty, same_series_penalty, related_penalty).  User u: queries[u] (its "{m}.retrieval"
 * embedding), group[u], r_masked (n_g values of its group's candidates, ragged in user order; n_r_masked = their sum), list items in
 * list order (CSR as rsys_retrieve_request; NULL: no lists).
 * Ranking score of candidate i, summed in user order as score = score + (lp_u + r_u): lp_u = z - lse_u + log(coef) with z, lse_u the fp32
 * scores of rsys_retrieve_topk (-inf where coef * exp(z - lse_u) is 0 in fp32, log(0) in the reference); coef = *retrieval_coef or 1;
 * r_u = c0 * rating_mean + c1 * r_masked with (c0, c1) = rating_coefs, or r_masked when rating_coefs is NULL.  r_in (n_total floats in
 * candidate order) replaces the score (queries and r_masked are then not read).
 * Reranking (every operation rounded in fp32, no contraction): per round score = ((r - mmr) - ss) - rel, best = the first position of the
 * maximum under Julia's isless (-inf < ... < -0.0 < +0.0 < ... < inf < NaN), r[best] = -inf (a position is picked again once fewer finite
 * scores than rounds remain); then ss = ss * decay, + same_series_penalty for every candidate that is a stored row of column ids[best] of
 * "{m}.related"; rel = rel * decay, + flag * related_penalty if flag[best]; mmr = max(mmr * decay, G[:, best] * mmr_penalty) with Julia's
 * max (NaN propagates, +0.0 over -0.0).  flag[i]: candidate i is a stored row of the column of any list entry of medium m, of any user of
 * the group, whose status is not 3 or 5 (every entry, not the last status per item).  G = E_c^T E_c over the candidates' rows of the
 * item-similarity table of m (rsys_retrieve_similarity_set), fp32 with a fixed summation order.
 * Output: ids_out[cand_offsets[g] + t] = the id picked in round t (slots t >= min(partialk, n_g): -1), or NULL (ranking only: no Gram, no
 * loop); r_out = the ranking scores before reranking (n_total floats in candidate order), or NULL.  ids_out needs the related and
 * similarity tables of `medium`.  1 <= n_users <= 4096, every group needs a user.  Synchronous, bitwise reproducible, changes no model
 * state; the device workspace grows on demand and is freed with the model. */
int32_t rsys_rank_request(rsys_model* m, int32_t medium, int32_t n_groups,
                          const int64_t* cand_offsets, const int32_t* cand_ids,   /* [n_groups + 1] CSR over groups, [n_total] */
                          const int32_t* partialk, const float* penalties,        /* [n_groups], [n_groups][4] */
                          const float* queries, int64_t n_users,                  /* [n_users][embed_dim] f32 */
                          const int32_t* group,                                   /* [n_users] in [0, n_groups), or NULL: group = user */
                          const float* r_masked, int64_t n_r_masked,              /* ragged over users */
                          const int64_t* hist_offsets,                            /* [n_users + 1] CSR over users, or NULL (no lists) */
                          const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                          const float* retrieval_coef, const float* rating_coefs, float rating_mean, /* [1] or NULL, [2] or NULL */
                          const float* r_in,                                      /* [n_total] or NULL */
                          int32_t* ids_out, float* r_out);                        /* [n_total] each, or NULL */
/* A page from raw histories in one device pipeline (Inference/compute.jl:512-531 + render.jl:437-474): for n_groups request
 * states of either medium -- the retrieval forward of their users, rsys_retrieve_request, the page window (render.jl:447-465, the ranked
 * slice clamped to the retrieved list), the ranking forward at the page's candidates, rsys_rank_request with partialk = the page's last
 * index.  User embeddings, retrieved ids and rating-head values stay on the device; only the per-group counts are read back in between.
 * Group g: group_medium[g], pagination (offset[g] >= 0, 1 <= limit[g] <= 1024), penalties[g][4] as rsys_rank_request.  User u (1 <= n_users
 * <= 4096, every group needs one): group[u]; row u of retrieval_rows, an inference batch of n_users rows of max_sequence_length
 * interactions laid out as rsys_batch_upload takes it (the ten inference arrays incl. rope_input_pos; targets and masks are not read),
 * whose query token is token retrieval_token[u] in [0, 2 S) of the row; row u of ranking_prefix, the same ten arrays with prefix_stride
 * columns per row, of which the first nh = user_desc[u][0] (<= S / 2) are the history part of the user's ranking rows; user_desc[u] =
 * (nh, userid, gender, source) and user_ts[u] = `time` of the candidate tokens.  The library assembles one ranking row per user and chunk of
 * at most S - S / 2 candidates on the device: prefix, then per candidate j matchedid = id (+ vocab_0 for medium 1), time = user_ts, status
 * -1, rating = progress = 0, rope_input_pos = nh, token_mask_ids = nh + j, and reads the rating head at its action token.  Both forwards
 * run in waves of at most max_rows rows, media mixed.  adapter_slots[4] = the bank slots of (0.retrieval, 0.ranking, 1.retrieval, 1.ranking),
 * each -1 for the base model, or NULL: every row runs the base model.  List items and selected items once, as CSR over users / groups in
 * the shapes of rsys_retrieve_request (either may be NULL).  coef_have[m] (NULL: 0): bit 0 = coefs[m][0] is medium m's retrieval
 * coefficient, bit 1 = coefs[m][1..2] are its rating coefficients and coefs[m][3] its rating mean (rsys_rank_request's).
 * Output: ids_out[ids_offsets[g] .. ids_offsets[g + 1]) = the page of group g (empty when it starts past the list), ids_offsets[n_groups
 * + 1]; total_out[g] = min(admissible items, 8192); ids_cap >= the sum of the limits.  fp32 and bf16 models with a replicated table; needs
 * the serving tables of both request calls.  Synchronous, bitwise reproducible.  Replaces the resident batch; reads and changes no
 * parameter, gradient or optimizer state.  RSYS_ERR_ARG (outputs untouched): a bad medium, a group without users, limit < 1, malformed
 * offsets, an incomplete adapter slot, an fp8 model, ids or index-path values out of range, missing tables. */
int32_t rsys_render_request(rsys_model* m, int32_t n_groups,
                            const int32_t* group_medium, const int64_t* offset, const int32_t* limit,  /* [n_groups] each */
                            const float* penalties,                                  /* [n_groups][4] */
                            int64_t n_users, const int32_t* group,                   /* [n_users] in [0, n_groups) */
                            const rsys_batch* retrieval_rows, const int32_t* retrieval_token,   /* rows = n_users; [n_users] */
                            const rsys_batch* ranking_prefix, int32_t prefix_stride, /* rows = n_users, prefix_stride columns per row */
                            const int32_t* user_desc, const double* user_ts,         /* [n_users][4], [n_users] */
                            const int32_t* adapter_slots,                            /* [4] or NULL */
                            const int64_t* hist_offsets,                             /* [n_users + 1] CSR over users, or NULL (no lists) */
                            const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                            const int64_t* sel_offsets,                              /* [n_groups + 1] CSR over groups, or NULL (none selected) */
                            const int32_t* sel_medium, const int32_t* sel_ids,
                            const int32_t* coef_have, const float* coefs,            /* [2] or NULL, [2][4] or NULL */
                            int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out);
/* rsys_render_request with the ranking forward on the reference's row (Finetune/embed.py:74-131, max_user_len - 1 = S - 1 events; DESIGN.md
 * 4w): every user is ranked on ALL the history its retrieval row holds, through the per-user K/V cache of rsys_rank_cache_*, instead of the
 * newest S / 2 - 1 events that fit beside a chunk of candidates.  The arguments of rsys_render_request without ranking_prefix and
 * prefix_stride; user_desc[u] = (n_hist, userid, gender, source) with n_hist in [0, S - 1]: columns [0, n_hist) of retrieval row u are the
 * user's history (positions 0 .. n_hist - 1, token_mask_ids 0; serve.render_pack writes retrieval_token[u] = 2 n_hist).  The rows' history
 * columns stay on the device while the retrieval waves upload them; no history column crosses the bus twice.  Per wave of at most max_rows
 * users with n_hist >= 1 one forward stores their histories (slot = the user's place in the wave), then their candidates run against the
 * slots in rows of at most S candidates (a user's candidates may span rows, rows of several users share a forward of at most max_rows rows):
 * candidate j of a row at column j with rope_input_pos = n_hist.  Users with n_hist = 0 run the assembled rows of rsys_render_request (nh =
 * 0, chunks of S - S / 2), in forwards of their own.  The cache is the model's reserve when it holds min(max_rows, users with a history)
 * slots, else max_rows slots are reserved (RSYS_ERR_STATE, outputs untouched, when they do not fit); the slots a call used hold its last
 * wave's histories afterwards, other slots are not touched.  Outputs, limits, errors and side effects as rsys_render_request. */
int32_t rsys_render_request_full(rsys_model* m, int32_t n_groups,
                                 const int32_t* group_medium, const int64_t* offset, const int32_t* limit,  /* [n_groups] each */
                                 const float* penalties,                                  /* [n_groups][4] */
                                 int64_t n_users, const int32_t* group,                   /* [n_users] in [0, n_groups) */
                                 const rsys_batch* retrieval_rows, const int32_t* retrieval_token,   /* rows = n_users; [n_users] */
                                 const int32_t* user_desc, const double* user_ts,         /* [n_users][4], [n_users] */
                                 const int32_t* adapter_slots,                            /* [4] or NULL */
                                 const int64_t* hist_offsets,                             /* [n_users + 1] CSR over users, or NULL (no lists) */
                                 const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                                 const int64_t* sel_offsets,                              /* [n_groups + 1] CSR over groups, or NULL (none selected) */
                                 const int32_t* sel_medium, const int32_t* sel_ids,
                                 const int32_t* coef_have, const float* coefs,            /* [2] or NULL, [2][4] or NULL */
                                 int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out);
/* ---- Item-similarity LambdaRank model (Training/item_similarity/pairwise_ltr.py, --features transformer / content).
 * A handle of its own, independent of rsys_model: an rsys_simmodel, passed as an opaque void*.  Trainable parameters by the reference's
 * state-dict names: "encoder.1.weight" [E][F] (weight decay 0.1) and "logit_scale" (scalar, log(1/0.07) at creation, no decay); the frozen
 * table f [V][F] ("transformer_embeddings.weight", F = 2048, or [transformer | content], F = 5120) goes through rsys_sim_features_set.
 * embed(ids) = normalize(W dropout_p(f[ids])), normalize(y) = y / max(|y|, 1e-12); score x = <embed(source), embed(target)> exp(logit_scale).
 * dtype RSYS_DTYPE_BF16 follows bf16 autocast: gathered features and W rounded to bf16, fp32 accumulation, the encoder output rounded to
 * bf16, normalisation, dot and scale in fp32; the weight gradient takes dY rounded to bf16 and is accumulated in fp32.  Every call is
 * bitwise reproducible (no float atomics in any sum a result depends on).  Calls on one handle are serialised by the caller. */
/* LTRModel(config) (pairwise_ltr.py:124-141): V items, F feature width (a multiple of 64), E = embed_dim (a multiple of 64), dtype
 * RSYS_DTYPE_FP32 or _BF16; 1 <= max_queries <= 4096 lists of 1 <= items_per_query <= 2048 slots per call; dropout in [0, 1) */
int32_t rsys_sim_create(int64_t V, int32_t F, int32_t E, int32_t dtype, int32_t max_queries, int32_t items_per_query, float dropout,
                        int32_t device, void** out);
int32_t rsys_sim_destroy(void* h);
/* state_dict access (load_pretrained_embeddings / load_state_dict): n must be the tensor's element count; unknown names are ARG errors */
int32_t rsys_sim_param_get(void* h, const char* name, float* out, int64_t n);
int32_t rsys_sim_param_set(void* h, const char* name, const float* in, int64_t n);
int32_t rsys_sim_grad_get(void* h, const char* name, float* out, int64_t n);
int32_t rsys_sim_zero_grad(void* h);   /* optimizer.zero_grad (train_epoch, pairwise_ltr.py:246) */
/* the frozen feature table [V][F] f32 (pairwise_ltr.py:146-155); V and F must be the handle's (a wrong F is an ARG error) */
int32_t rsys_sim_features_set(void* h, const float* features, int64_t V, int64_t F);
/* the same from a transformer model on the same device, without a host round trip: the rows of medium `medium` of its fp32 item table
 * (ItemEmbedding over all items, the table rsys_item_table returns; rebuilt first when stale).  The handle's V must be V_m and its F the
 * model's embed_dim ("transformer_embeddings.weight" of pairwise_ltr.py:146-155); replicated table only.  Synchronous. */
int32_t rsys_sim_features_from_model(void* h, rsys_model* m, int32_t medium);
/* model(batch) + loss.backward() (process_batch + lambdarank_loss, pairwise_ltr.py:175-190, 244-252): n_q lists of n slots, source[n_q],
 * target[n_q][n], relevance[n_q][n] and weight[n_q] (= sqrt(popularity)) as f32 (the reference holds them in fp64: relevances that differ
 * only beyond fp32 precision compare equal here).  order = 1-based rank of x descending, ties by slot; the loss is
 * sum_q w_q sum_{i,j: y_i > y_j} -logsigmoid(x_i - x_j) |(D_i - D_j)(y_i - y_j)| / sum_q w_q with D = 1 / log2(1 + order); the ranks
 * carry no gradient.  Training (evaluate == 0): every slot embeds its own copy of the source, each gathered row with its own dropout
 * mask (Philox keyed on (seed, step, row, column), launch_dropout's stream), and the gradient is ACCUMULATED.  evaluate != 0: no
 * dropout, no gradient.  *loss_out (may be NULL) = the batch loss.  Synchronous.  ARG errors: ids outside [0, V), n_q or n out of
 * range, non-finite or negative weights, a zero weight sum, features not set. */
int32_t rsys_sim_forward_backward(void* h, int32_t n_q, int32_t n, const int32_t* source, const int32_t* target, const float* relevance,
                                  const float* weight, int32_t evaluate, uint64_t seed, uint64_t step, float* loss_out);
/* LTRModel.ndcg in eval mode (pairwise_ltr.py:192-208): per list DCG = sum_r y_(r) / log2(r + 1) over the slots sorted by x descending
 * (ties by slot), IDCG the same over y sorted descending; out[0] = sum_q w_q nDCG_q, out[1] = sum_q w_q (fp64, query order) */
int32_t rsys_sim_ndcg(void* h, int32_t n_q, int32_t n, const int32_t* source, const int32_t* target, const float* relevance,
                      const float* weight, double out[2]);
/* clip_grad_norm_(clip) + GradScaler.step(AdamW) + zero_grad (pairwise_ltr.py:253-256, 263-275): AdamW beta 0.9 / 0.999, eps 1e-8, weight
 * decay 0.1 on encoder.1.weight and 0 on logit_scale, lr as given, the global-norm clip fused (clip <= 0: none).  A non-finite gradient
 * norm skips the update: parameters, moments and the step count stay as they were.  *norm_out = the norm before clipping, *skipped_out =
 * 1 when skipped (either may be NULL).  The gradient is cleared in both cases. */
int32_t rsys_sim_adamw_step(void* h, float lr, float clip, float* norm_out, int32_t* skipped_out);
int32_t rsys_sim_adamw_state_get(void* h, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step);
/* generate_embeddings (pairwise_ltr.py:450-472): embed every id in fp32 in both dtypes; out [V][E] (may be NULL).  train_mode != 0
 * applies dropout (the export train() takes right after train_epoch, the model still in train mode): row = id, RNG stream 0xffffffff.
 * The result is held on the device as the export rsys_sim_hard_negatives scores against. */
int32_t rsys_sim_embed_all(void* h, int32_t train_mode, uint64_t seed, float* out);
/* sets the held export [V][E] f32 directly (the reference's output.embeddings file) */
int32_t rsys_sim_export_set(void* h, const float* emb);
/* pairs.{m}.h5 "testmask" as bit rows: bits[V][ceil(V / 32)], bit (j & 31) of word j >> 5 of row i = testmask[i, j]; NULL clears */
int32_t rsys_sim_testmask_set(void* h, const int32_t* bits);
/* load_hard_negatives (pairwise_ltr.py:56-82) for n_src sources: w = bf16(bf16(E[i]) . bf16(E)^T) over the held export (fp32
 * accumulation, the output rounded to bf16); -inf for the source itself, for testmask[i, :] (split 0, training) or ~testmask[i, :]
 * (split 1, test), and for the source's positives pos_ids[pos_offsets[s] .. pos_offsets[s + 1]) (CSR over sources, or both NULL).
 * ids_out[s][n] = np.argsort(w, kind="stable")[-n:]: the n best ids in ascending (score, id) order, so a tie keeps the larger id and
 * lists tied ids ascending; when fewer than n ids are admissible, the admissible ones come last, preceded by the largest inadmissible
 * ids in ascending order.  1 <= n <= min(items_per_query, V).  ARG errors: ids out of range, malformed offsets, no testmask or export. */
int32_t rsys_sim_hard_negatives(void* h, int32_t split, int32_t n_src, const int32_t* sources, const int64_t* pos_offsets,
                                const int32_t* pos_ids, int32_t n, int32_t* ids_out);
/* The ranks pairwise_metrics.jl sorts the whole catalogue for (ndcg_at_k / recall_at_k, :72-123, over M = E' * E .* testmask, :172-174):
 * for n_src sources and their targets tgt_ids[tgt_offsets[s] .. tgt_offsets[s + 1]) (CSR over sources, tgt_offsets[0] == 0), ranks_out[j]
 * = the 1-based position of target j among ALL items i != source of the medium.  Over the held fp32 export (rsys_sim_embed_all /
 * rsys_sim_export_set) and the held test mask (rsys_sim_testmask_set):
 *   g[s][i] = the fp32 dot product of export rows s and i, fp32 accumulation in a fixed order (no bf16 anywhere);
 *   v[s][i] = g[s][i] where testmask[s][i] is set, else g[s][i] * 0.0f as an IEEE product (a masked zero keeps the sign of g, a
 *             non-finite g becomes NaN);
 *   order   = sortperm(v, rev = true): descending under isless (-inf < ... < -0.0 < +0.0 < ... < +inf < NaN, all NaNs equal), equal
 *             values by ascending id;
 *   rank(t) = 1 + #{i != s : v_i sorts above v_t} + #{i != s, i < t : v_i equal to v_t} for t != s, and 0 for t == s (not a candidate).
 * Sources may repeat, and so may the targets of a source (each gets its rank).  Any n_src >= 1 (chunks of 256 sources; the workspace
 * grows on demand and is freed with the handle).  Synchronous, bitwise reproducible, changes no model state.  ARG errors (nothing is
 * written): no export, no test mask, ids outside [0, V), malformed offsets, more than 2^31 - 1 targets. */
int32_t rsys_sim_pair_ranks(void* h, int32_t n_src, const int32_t* sources, const int64_t* tgt_offsets, const int32_t* tgt_ids,
                            int32_t* ranks_out);

/* ---- Search model (Training/search/train.py:76-130): text-query embeddings against the transformer's item table.  A handle
 * of its own per medium, independent of rsys_model: an rsys_searchmodel, passed as an opaque void*.  Trainable parameters by the
 * reference's state-dict names: "encoder.weight" Wenc [Q][D] (nn.Linear(D, Q, bias = False); weight decay) and "logit_scale" (scalar, 1.0
 * at creation, no decay); the frozen table E_m [V_m][D] (the rows of medium m of "retrieval_embeddings.weight") goes through
 * rsys_search_features_set.  The reference forms W = E Wenc^T and soft-maxes x W^T exp(logit_scale) over the columns of each medium; all
 * labels of a batch lie in the handle's medium, so the other medium's columns carry neither loss nor gradient, and the device computes
 * the factored form: P = x Wenc, logits = P E_m^T exp(logit_scale), loss = sum_i w_i (logsumexp_i - logit_i[y_i]) / sum w.
 * dtype RSYS_DTYPE_FP32: everything fp32.  RSYS_DTYPE_BF16: x, Wenc, E_m, P, G = w (softmax - onehot) and dP rounded to bf16 as MFMA
 * operands with fp32 accumulation; the scores, soft-max statistics, loss, d logit_scale, dWenc and the optimizer stay fp32.  These are
 * NOT bf16 autocast's rounding points (autocast rounds W and the logits, which the factored form never holds).  Every call is bitwise
 * reproducible (no float atomics in any sum a result depends on).  Calls on one handle are serialised by the caller. */
/* SearchModel(config, medium): V_m items (any count), D = the item table's width and Q = the query embedding's width (multiples of 64;
 * 2048 and 3072 in the reference), 1 <= max_batch <= 4096 rows per call */
int32_t rsys_search_create(int64_t V_m, int32_t D, int32_t Q, int32_t dtype, int32_t max_batch, int32_t device, void** out);
int32_t rsys_search_destroy(void* h);
/* state_dict access: n must be the tensor's element count; unknown names are ARG errors */
int32_t rsys_search_param_get(void* h, const char* name, float* out, int64_t n);
int32_t rsys_search_param_set(void* h, const char* name, const float* in, int64_t n);
int32_t rsys_search_grad_get(void* h, const char* name, float* out, int64_t n);
int32_t rsys_search_zero_grad(void* h);
/* the frozen table E_m [V_m][D] f32 from the host; V_m and D must be the handle's */
int32_t rsys_search_features_set(void* h, const float* features, int64_t V_m, int64_t D);
/* the same from a transformer model on the same device without a host round trip: the rows of medium `medium` of its fp32 item table
 * (as rsys_sim_features_from_model).  Synchronous. */
int32_t rsys_search_features_from_model(void* h, rsys_model* m, int32_t medium);
/* model(batch) + loss.backward() (train.py:113-130): x [B][Q] f32 query embeddings, labels [B] medium-local ids, weights [B] (=
 * sqrt(counts)).  *loss_out = sum_i w_i (lse_i - logit_i[y_i]) / sum w, *weight_sum_out = sum w (either may be NULL).  evaluate == 0:
 * the gradient is ACCUMULATED into .grad; evaluate != 0: forward only.  Synchronous.  ARG errors (the reference would return NaN or
 * fault): B outside [1, max_batch], a label outside [0, V_m), a negative or non-finite weight, a zero weight sum, features not set. */
int32_t rsys_search_forward_backward(void* h, const float* x, const int32_t* labels, const float* weights, int32_t B, int32_t evaluate,
                                     float* loss_out, float* weight_sum_out);
/* AdamW over the two parameters (train.py:181-192): betas and eps as given (torch's defaults 0.9, 0.999, 1e-8 in the reference),
 * weight_decay on encoder.weight and 0 on logit_scale; clears the moments and the step count */
int32_t rsys_search_adamw_create(void* h, float beta1, float beta2, float eps, float weight_decay);
/* clip_grad_norm_(clip) + GradScaler.step(AdamW) + zero_grad (train.py:170-174): the global-norm clip fused (clip <= 0: none).  A
 * non-finite gradient norm skips the update: parameters, moments and the step count stay as they were.  *norm_out = the norm before
 * clipping, *skipped_out = 1 when skipped (either may be NULL).  The gradient is cleared in both cases.  RSYS_ERR_STATE before
 * rsys_search_adamw_create. */
int32_t rsys_search_adamw_step(void* h, float lr, float clip, float* norm_out, int32_t* skipped_out);
int32_t rsys_search_adamw_state_get(void* h, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step);
int32_t rsys_search_adamw_state_set(void* h, const char* name, const float* exp_avg, const float* exp_avg_sq, int64_t n, int32_t step);
/* generate_embeddings (train.py:346-371): out [V_m][Q] = E_m Wenc^T ("search.{m}"), fp32 arithmetic in both dtypes.  "temperature" is
 * the raw logit_scale parameter (rsys_search_param_get), not its exponential. */
int32_t rsys_search_export(void* h, float* out);
/* Serving (beyond the reference, which has no serving code for this model; parity is against the numpy restatement only): for n_queries
 * query embeddings x [n_queries][Q], log_softmax over the medium's items of the factored logits (W is not needed), and per query the k
 * best items by descending log-probability, ties by ascending id: ids_out / logp_out [n_queries][k].  1 <= n_queries <= max_batch,
 * 1 <= k <= min(V_m, 8192); a non-finite x is an ARG error (checked on the host).  Changes no model state. */
int32_t rsys_search_topk(void* h, const float* x, int32_t n_queries, int32_t k, int32_t* ids_out, float* logp_out);

/* ---- Watch-order counts (Training/media_relations.jl get_watch_order, :174-197).  A handle of its own, passed as an opaque
 * void*: one row band [row0, row1) of the V x V int32 matrix W, W[a][b] = the number of users whose projected history has a before b
 * (the reference's watch_order[a+1, b+1]).  Counts are exact integer adds, so every result is bitwise reproducible and independent of
 * how the users are split into add calls.  A full band (0, V) is the normal case; a narrower one caps device memory. */
/* zeros(Int32, V, V) (:175) restricted to rows [row0, row1): 0 <= row0 <= row1 <= V.  RSYS_ERR_STATE when the band does not fit in free
 * device memory (the message names the bytes asked for) */
int32_t rsys_watch_order_create(int64_t V, int64_t row0, int64_t row1, int32_t device, void** out);
int32_t rsys_watch_order_destroy(void* h);
/* the loop of :184-193 over n_users projected histories (project_earliest, :156-172): items[offsets[u] .. offsets[u + 1]) in watch order,
 * distinct per user, in [0, V); adds 1 to W[h_i][h_j] for every i < j with h_i in the band.  offsets [n_users + 1] start at 0 and do not
 * decrease.  ARG errors (nothing is added): malformed offsets, an item outside [0, V), a user count past 2^31 - 1.  Synchronous. */
int32_t rsys_watch_order_add(void* h, int64_t n_users, const int64_t* offsets, const int32_t* items);
/* users with >= 1 item added so far (get_watch_order's num_users, :186-188) */
int32_t rsys_watch_order_users(void* h, int64_t* out);
/* dense rows [row0, row0 + n_rows) of W, within the band: out[n_rows][V] */
int32_t rsys_watch_order_rows_get(void* h, int64_t row0, int64_t n_rows, int32_t* out);
/* out[k] = W[a[k]][b[k]] (is_watched_before, :199-202; pairwise_dataset.jl:126-135); a[k] in the band, b[k] in [0, V), else ARG */
int32_t rsys_watch_order_gather(void* h, int64_t n, const int32_t* a, const int32_t* b, int32_t* out);
/* the band's non-zeros as CSR (rows band-local, columns ascending): indptr [row1 - row0 + 1] int64, indices / values [nnz].  *nnz is
 * always written; the arrays only when none is NULL and cap >= nnz (call once with NULL to size them).  The same matrix gives the same
 * bytes on every call. */
int32_t rsys_watch_order_csr(void* h, int64_t* indptr, int32_t* indices, int32_t* values, int64_t cap, int64_t* nnz);
/* zeros the band and the user count */
int32_t rsys_watch_order_clear(void* h);

/* on != 0: every float sum of the training step gets a fixed order (split-K partial tiles summed in split order, reductions through
 * per-workgroup partials instead of float atomics), so a step -- losses, gradients, updated parameters -- is bitwise reproducible
 * from run to run; costs a few percent of the step.  Replicated or row-sharded table, full or sampled soft-max.  (The reference's CUDA path is not reproducible:
 * its embedding backward and split-K reductions use atomics too.) */
int32_t rsys_model_set_deterministic(rsys_model* m, int32_t on);
/* inference forward -- model.py:531-538; task 0 = retrieval (out: rows*2S*D), 1 = ranking (out: rows*2S) */
int32_t rsys_infer(rsys_model* m, int32_t task, float* out, int64_t n);
/* the same forward, returning only the tokens a server reads (Finetune/embed.py:147-161 takes token 2n of a user for
 * retrieval and the candidates' action tokens for ranking): token_index[n_tokens] = flat token indices in [0, rows*2S);
 * out = n_tokens*D floats (retrieval: the trunk output rows) or n_tokens floats (ranking: the rating head on those rows only) */
int32_t rsys_infer_select(rsys_model* m, int32_t task, const int32_t* token_index, int64_t n_tokens, float* out, int64_t n);
/* Adapter bank of a base model (finetune = 0; fp32 or bf16): up to RSYS_ADAPTER_SLOTS rank-8 LoRA adapter sets on q_proj / v_proj
 * (model.py:235-271; alpha 16, scaling 2) held on the device beside the frozen trunk -- what Finetune/embed.py:180-255 serves as four
 * models that share one trunk.  Tensors go in and out by their state-dict names "transformers.layers.{l}.attn.{q,v}_proj_lora_{A,B}.weight"
 * (A: 8 x embed_dim; q B: num_heads*head_dim x 8; v B: num_kv_heads*head_dim x 8, row-major).  A slot is complete once all 4 * num_layers
 * tensors have been set since its last clear; get returns the float32 values that were set, bit for bit.  Setting or clearing a slot
 * changes no parameter of the model: the fused item table, the serving tables and a following training step are unaffected.
 * Errors (RSYS_ERR_ARG, nothing written): slot outside [0, RSYS_ADAPTER_SLOTS), unknown name, wrong element count, get of a tensor that
 * is not set, a finetune = 1 or fp8 model. */
#define RSYS_ADAPTER_SLOTS 8
int32_t rsys_adapter_set(rsys_model* m, int32_t slot, const char* name, const float* in, int64_t n);
int32_t rsys_adapter_get(rsys_model* m, int32_t slot, const char* name, float* out, int64_t n);
int32_t rsys_adapter_clear(rsys_model* m, int32_t slot);
/* bit s of *mask_out: slot s is complete */
int32_t rsys_adapter_slots(rsys_model* m, int32_t* mask_out);
/* rsys_infer_select with one adapter slot per batch row: row_adapter[rows] in [-1, RSYS_ADAPTER_SLOTS); the tokens of row r run with
 * q += 2 (xn A_q^T) B_q^T, v += 2 (xn A_v^T) B_v^T of slot row_adapter[r] in every layer, -1 = the base model.  One forward for the
 * whole batch, whatever the number of distinct slots; a row's result does not depend on the other rows' slots.  Output and limits as
 * rsys_infer_select.  RSYS_ERR_ARG (out untouched): row_adapter NULL, an entry out of range or naming an incomplete slot, no batch. */
int32_t rsys_infer_select_adapters(rsys_model* m, int32_t task, const int32_t* row_adapter, const int32_t* token_index, int64_t n_tokens,
                                   float* out, int64_t n);
/* rsys_infer_select_adapters on packed serving rows: several users share a batch row, each in a segment that starts at
 * an interaction column that is a multiple of 32 (a multiple of 64 tokens), so no 64-token tile holds two users and a slot per tile is
 * enough.  tile_adapter int32 [rows][ceil(S / 32)] in the caller's geometry (S = max_sequence_length): entry j of row r is the slot, or
 * -1 = the base model, of interactions [32 j, 32 j + 32) of row r.  On a trimmed batch the entries behind row_len are range-checked and
 * otherwise unused; token_index keeps r * 2S + t.  The per-token arithmetic is that of rsys_infer_select_adapters: a user's result does
 * not depend on the slots of other tiles.  tile_adapter == NULL behaves as rsys_infer_select.  RSYS_ERR_ARG (out untouched): an entry
 * outside [-1, RSYS_ADAPTER_SLOTS) or naming an incomplete slot, no batch, an fp8 or finetune = 1 model. */
int32_t rsys_infer_select_tiles(rsys_model* m, int32_t task, const int32_t* tile_adapter, const int32_t* token_index, int64_t n_tokens,
                                float* out, int64_t n);
/* Training through the adapter bank: the reference's daily finetune -- four rank-8 adapters, one per medium and metric, as
 * four sequential jobs on the same frozen trunk (Finetune/run.jl:9-13; transformer.py:591-597, 259-276) -- as ONE pass over a batch whose
 * rows name their slot and task.
 * rsys_adapter_train_enable (model.py:238, nn.Dropout(lora_dropout) on the LoRA input): allocates, on first use, fp32 gradients and AdamW
 *   moments in the bank's layout and La per layer; dropout in [0, 1) applies to training passes only.  May be called again to change it.
 * rsys_adapter_forward_backward (model.py:417-435, 493-529 + loss.backward() of train.py:259-272, per task): row r of the resident batch
 *   runs with slot row_slot[r] in [-1, RSYS_ADAPTER_SLOTS) and task row_task[r] = medium * 2 + metric in {0,1,2,3} (the order of task_w), or
 *   -1 / -1: the base model, no loss.  Within one call a task belongs to at most one slot.  A row of task (m, x) is masked by the finetune
 *   rule with metric x, its masked weights of every other task are zero; loss_i and its weight sum therefore come from the rows of task i
 *   alone and are read with rsys_losses_get / _push / _drain.  evaluate == 0: the gradient of sum_i loss_i * grad_scale is ACCUMULATED into
 *   the slots' LoRA gradients (trunk frozen: no other gradient is formed or written); every sum has a fixed order, so a call is bitwise
 *   reproducible and a slot's gradient does not depend on other slots' rows.  seed / step key the dropout mask (with layer and element).
 * rsys_adapter_grad_get / rsys_adapter_zero_grad: a slot's gradient by the state-dict name of its tensor; all slots' gradients to zero.
 * rsys_adapter_adamw_step (clip_grad_norm_ + AdamW.step + zero_grad of train.py:273-275, per slot): per_slot[n_slots][3] = {active (0 / 1),
 *   lr factor, max_norm (<= 0: no clip)}; an active slot's tensors are scaled by min(1, max_norm / (norm + 1e-6)) of the slot's own global
 *   norm (norms_out[n_slots], 0 for inactive slots), take one AdamW step at lr0 * factor (decoupled decay wd on every LoRA tensor, all 2-D;
 *   bias correction by the slot's own step count) and their gradients are zeroed; the compute-type copies the forward reads are refreshed.
 *   An inactive slot's masters, moments, step count and gradient stay bit for bit.  rsys_adapter_clear also zeroes the slot's gradient,
 *   moments and step count: an adapter loaded into a used slot starts a fresh optimizer state (rsys_adapter_set of single tensors keeps it).
 * rsys_adapter_adamw_state_get / _set: a slot's moments by tensor name (name NULL: only the step count), step_in < 0 leaves the count.
 * RSYS_ERR_ARG, nothing written: an fp8, finetune = 1 or row-sharded model; training not enabled; no batch; a NULL vector; a slot out of
 * range or incomplete; a task out of range; slot -1 with a task or a slot without one; one task named by two slots; n_slots outside
 * [1, RSYS_ADAPTER_SLOTS]; dropout outside [0, 1). */
int32_t rsys_adapter_train_enable(rsys_model* m, float dropout);
int32_t rsys_adapter_forward_backward(rsys_model* m, int32_t evaluate, const int32_t* row_slot, const int32_t* row_task, float grad_scale,
                                      uint64_t seed, uint64_t step);
/* rsys_adapter_forward_backward on packed rows: several users share a batch row, each in a SEGMENT -- the live prefix of
 * its finetune row -- that starts at an interaction column that is a multiple of 32 (64 tokens) and lies inside one row, so no 64-token
 * tile holds two users.  seg int32 [n_seg][5] = (row, first_column, columns, slot, task); slot and task as above, -1 / -1 = the base model,
 * no loss.  Semantics are those of rsys_adapter_forward_backward with "row" read as "segment": the finetune mask rule uses the segment's
 * metric, masked weights of every other task are zero, a task belongs to at most one slot.  A slot's gradient is alpha times the sum over
 * its segments IN DESCRIPTOR ORDER of per-segment partials, each summed over the segment's tokens in ascending order: bitwise
 * reproducible, independent of other slots' segments, and the unpacked call's order when descriptors follow the rows' order.  The last
 * layer runs dense in this call (no compact top).  Dropout is keyed on the element index in the packed batch.  Rows are full-length rows
 * (rsys_batch_upload); a trimmed batch is RSYS_ERR_STATE.  THE CALLER GUARANTEES THE RESIDENT COLUMNS: inside a segment one non-zero
 * userid, distinct within its row, rope_input_pos relative to the segment; zeros in every column no segment covers.
 * RSYS_ERR_ARG, nothing written or enqueued: everything rsys_adapter_forward_backward refuses; seg NULL; n_seg < 1 or > rows * ceil(S / 32);
 * first_column % 32 != 0; a segment outside its row (columns < 1 or first_column + columns > S); two segments sharing a tile. */
int32_t rsys_adapter_forward_backward_packed(rsys_model* m, int32_t evaluate, const int32_t* seg, int32_t n_seg, float grad_scale,
                                             uint64_t seed, uint64_t step);
int32_t rsys_adapter_grad_get(rsys_model* m, int32_t slot, const char* name, float* out, int64_t n);
int32_t rsys_adapter_zero_grad(rsys_model* m);
int32_t rsys_adapter_adamw_step(rsys_model* m, float lr0, float beta1, float beta2, float eps, float wd, const float* per_slot,
                                int32_t n_slots, float* norms_out);
int32_t rsys_adapter_adamw_state_get(rsys_model* m, int32_t slot, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n,
                                     int32_t* step_out);
int32_t rsys_adapter_adamw_state_set(rsys_model* m, int32_t slot, const char* name, const float* exp_avg, const float* exp_avg_sq, int64_t n,
                                     int32_t step);
/* Ranking forward over full-length histories through a per-user K/V cache (Finetune/embed.py:74-161).  The reference ranks a user in one
 * row of max_user_len + max_ranking_items interactions: up to max_user_len - 1 history events (token_mask_ids 0) followed by the candidates
 * (token_mask_ids n_hist + j, all at rope_input_pos n_hist).  Under the mask a history token never sees a candidate and a candidate sees the
 * whole history plus its own two tokens, so the history's K and V of every layer do not depend on the candidates: they are computed once,
 * in a row of at most S events, kept post-RoPE per layer, and the candidates run as query-only rows against them -- the reference's function
 * without a 4 S-token row, for histories of up to S - 1 events, and without recomputing the history per chunk of candidates.
 * rsys_rank_cache_reserve: n_slots >= 1 cache slots of [num_layers][2 S][2 num_kv_heads head_dim] values in the compute dtype (0 frees them;
 *   a new size drops what was stored).  RSYS_ERR_STATE when they do not fit in free device memory: the model stays usable, and when the
 *   size is refused before anything was freed the slots stored so far stay; when the allocation itself fails it has no cache.
 * rsys_rank_cache_store: the inference trunk forward of the resident batch, whose row r holds a history alone (events 0 .. n_hist[r] - 1
 *   with token_mask_ids 0 and rope_input_pos 0 .. n_hist[r] - 1; what follows in the row is padding the history never sees), with the
 *   adapter slot row_adapter[r] as in rsys_infer_select_adapters (NULL: the base model); K and V of tokens [0, 2 n_hist[r]) of every layer,
 *   after RoPE and the adapters' updates, go to slot slot[r].  0 <= n_hist[r] <= S; the slots of one call are distinct.
 * rsys_rank_cache_candidates: the same trunk over the resident batch of CANDIDATE rows: row r holds n_cand[r] in [1, S] candidates at
 *   events 0 .. n_cand[r] - 1 (item, status, rating, ... as the reference's candidate events) and reads slot slot[r]; several rows may read
 *   one slot.  Every event of row r runs at RoPE position n_hist of its slot (the call sets it; the batch's rope_input_pos,
 *   token_mask_ids and userid are not read), so the slot must hold at most S - 1 events.  A token of candidate j attends to the slot's
 *   2 n_hist cached tokens and to tokens 2 j, 2 j + 1 of its own row.  out[sum n_cand], row order = the rating head at action tokens
 *   2 j + 1.  n_hist = 0: a candidate sees only itself.  (Deviation: the reference gives candidate 0 of an EMPTY history
 *   token_mask_ids 0, which makes it visible to the other candidates; here it is not.  Hosts that need that row use rsys_infer_select.)
 * Both calls are synchronous, replace the resident batch's derived arrays as every inference call does, and touch no parameter, gradient
 * or optimizer state.  RSYS_ERR_ARG (out and the cache untouched): no batch uploaded, nothing reserved, a slot outside the reserve, a slot
 * never stored, duplicate slots in one store, a count out of range, an adapter slot that is not complete, an fp8 or row-sharded model. */
int32_t rsys_rank_cache_reserve(rsys_model* m, int32_t n_slots);
int32_t rsys_rank_cache_store(rsys_model* m, const int32_t* row_adapter, const int32_t* n_hist, const int32_t* slot);
int32_t rsys_rank_cache_candidates(rsys_model* m, const int32_t* row_adapter, const int32_t* slot, const int32_t* n_cand, float* out);
/* The two cache calls on PACKED rows: several users per row of the resident batch (full or trimmed), each in a segment -- a run
 * of whole 64-token attention tiles of one row that starts at an interaction column that is a multiple of 32; no tile holds two segments;
 * the columns between segments are zero padding with userid 0.  seg_adapter[n_seg]: the adapter-bank slot of every segment or -1 (NULL:
 * the base model), applied per tile as in rsys_infer_select_tiles.
 * rsys_rank_cache_store_packed: seg[n_seg][4] = (row, first_column, n_hist, slot).  A store segment holds one user's n_hist history events
 *   alone (token_mask_ids 0; userid distinct among the segments of the forward, so that no history sees another); the call runs event i of a
 *   segment at RoPE position i itself, whatever the batch's rope_input_pos says.  K and V of the segment's tokens of every layer go to rows
 *   [0, 2 n_hist) of its slot: the slot rsys_rank_cache_store fills from the same history in a row of its own.
 * rsys_rank_cache_candidates_packed: seg[n_seg][4] = (row, first_column, n_cand, slot).  A candidate segment holds n_cand in [1, S] candidates
 *   at columns first_column + j and reads its slot as a row of rsys_rank_cache_candidates does; every token of its tiles runs at RoPE
 *   position n_hist of that slot.  A user's list may be cut into several segments, in one row or in several, and several segments may read
 *   one slot.  out[sum n_cand]: the rating head at the candidates' action tokens, segment after segment in descriptor order.
 * Both are synchronous.  RSYS_ERR_ARG (nothing is written, no slot is marked stored, out untouched): what the row calls refuse, n_seg outside
 * [1, max_rows x ceil(S / 32)], a row outside the batch, a first column that is not a multiple of 32, a segment that crosses its row's end
 * or shares a tile with another, n_hist outside [0, row length], n_cand outside [1, row length], duplicate slots in one store, a candidate
 * slot never stored or holding more than S - 1 events, an incomplete adapter slot, an fp8, finetune = 1 or row-sharded model.  A store that
 * fails while it runs invalidates the slots it names. */
int32_t rsys_rank_cache_store_packed(rsys_model* m, const int32_t* seg_adapter, int32_t n_seg, const int32_t* seg);
int32_t rsys_rank_cache_candidates_packed(rsys_model* m, const int32_t* seg_adapter, int32_t n_seg, const int32_t* seg, float* out);
/* debug/parity: trunk output of the last forward (rows*2S*D floats).  A training pass computes it only at the positions the heads
 * select; this call then runs the dense tail of the last layer first (results as model.py:335-343 over every token). */
int32_t rsys_trunk_output_get(rsys_model* m, float* out, int64_t n);

/* torch.nn.utils.clip_grad_norm_(params, max_norm) -- train.py:273; norm_out may be NULL */
int32_t rsys_clip_grad_norm(rsys_model* m, float max_norm, float* norm_out);

/* create_optimizer -- train.py:285-298 (AdamW, betas 0.9/0.95, wd on dim>=2) */
int32_t rsys_adamw_create(rsys_model* m, float lr, float beta1, float beta2, float eps, float weight_decay,
                          rsys_optimizer** out);
int32_t rsys_adamw_destroy(rsys_optimizer* o);
/* optimizer.step(); optimizer.zero_grad() with lr = lr0*lr_factor (LambdaLR, train.py:684-689).
 * fused_clip_max_norm > 0 fuses clip_grad_norm_ (global norm over the flat gradient buffer) and the
 * data-parallel mean (grads / grad_div) into the update -- one pass over the parameters. */
int32_t rsys_adamw_step(rsys_optimizer* o, float lr_factor, float fused_clip_max_norm, float grad_div);
/* (beyond the reference, opt-in) ZeRO-1 for the replicated data-parallel model: rsys_adamw_set_zero1, right after the create, keeps
 * AdamW moments for this rank's 1/world of the flat parameter range only; rsys_adamw_step_zero1 then replaces rsys_allreduce_grads +
 * rsys_adamw_step: reduce-scatter of the gradient, global-norm clip from the ranks' partial sums, AdamW on the rank's part,
 * all-gather of the parameters.  No early gradient buckets in this mode (do not arm rsys_set_grad_sync). */
int32_t rsys_adamw_set_zero1(rsys_optimizer* o, int32_t rank, int32_t world);
int32_t rsys_adamw_step_zero1(rsys_optimizer* o, rsys_comm* c, float lr_factor, float fused_clip_max_norm, float grad_div);
int32_t rsys_adamw_state_get(rsys_optimizer* o, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step);
int32_t rsys_adamw_state_set(rsys_optimizer* o, const char* name, const float* exp_avg, const float* exp_avg_sq, int64_t n, int32_t step);

/* init_process_group("nccl") + DDP gradient all-reduce -- train.py:582, 678-682, 268-272;
 * RCCL over xGMI, one communicator per process.  id_buf: 128 bytes made on rank 0 and
 * distributed by the host (the reference uses torchrun's store). */
int32_t rsys_comm_unique_id(uint8_t id_buf[128]);
int32_t rsys_comm_init(const uint8_t id_buf[128], int32_t rank, int32_t world, int32_t device, rsys_comm** out);
int32_t rsys_comm_destroy(rsys_comm* c);
/* DDP launches a bucket's all-reduce as soon as its gradients are final (train.py:678-682): call before the backward of
 * the LAST micro-step of an optimizer step; the trunk backward then starts the all-reduce of each finished >= 25 MB run
 * of per-layer weight gradients on the communicator's stream while it continues, and rsys_allreduce_grads reduces the
 * rest.  comm == NULL disarms.  (Micro-steps before the last one accumulate locally: DDP no_sync, train.py:268-271.) */
int32_t rsys_set_grad_sync(rsys_model* m, rsys_comm* c);
/* (beyond the reference, opt-in; replicated table, bf16) split the reduce of the item table's gradient, 80 % of the flat buffer:
 * with this on, an armed rsys_set_grad_sync also starts -- as soon as the heads' part of dF is complete, before the trunk backward --
 * an out-of-place all-reduce of that part; the backward's token scatter is kept as a list of distinct rows, and rsys_allreduce_grads
 * all-gathers the ranks' lists instead of all-reducing the table: G[E] = sum of the head parts + every rank's token rows, added in
 * rank order.  Same gradient up to the order of the additions.  Not combined with ZeRO-1. */
int32_t rsys_model_set_split_table_reduce(rsys_model* m, int32_t on);
/* row-sharded table mode: the communicator the forward / backward use for the row exchange and the vocabulary-parallel
 * cross entropy (world must equal cfg.table_shard_world; NULL only when that is 1) */
int32_t rsys_model_set_shard_comm(rsys_model* m, rsys_comm* c);
/* rows [lo, hi) of the (V + 1)-row item table this model holds (the whole table when it is replicated) */
int32_t rsys_table_rows(rsys_model* m, int64_t* lo, int64_t* hi);
/* sum-all-reduce of (the rest of) the flat gradient buffer in buckets (the mean is folded into rsys_adamw_step's
 * grad_div); *early_floats (optional query): how many gradient elements the last call found already reduced */
int32_t rsys_allreduce_grads(rsys_model* m, rsys_comm* c);
int32_t rsys_grad_sync_early(rsys_model* m, int64_t* early_floats);
/* what the last optimizer step's gradient reduction enqueued, in enqueue order (the DDP bucket schedule of train.py:678-682 as this
 * library runs it): up to cap triples {first element, one past the last element, phase} of the flat gradient buffer; phase 0 = early
 * bucket from inside the backward, 1 = tail beside the metadata-projection gradient GEMM, 2 = that GEMM's output, 3 / 4 = the two parts of
 * the split table reduce (head part out of place; the ranks' token rows, elements = gathered floats).  *n = entries recorded. */
int32_t rsys_grad_sync_schedule(rsys_model* m, int64_t* triples, int32_t cap, int32_t* n);
/* {rank, world, transport (1 = RCCL, 2 = in-process rank group of the tests), RCCL version code (ncclGetVersion) or 0} */
int32_t rsys_comm_info(rsys_comm* c, int32_t out[4]);
int32_t rsys_allreduce_f64(rsys_comm* c, double* x, int32_t n);   /* reduce_mean, train.py:199-204 */
int32_t rsys_self_test(rsys_comm* c);                              /* hardware_check.py:6-12 */
/* Replica consistency (the reference's DDP constructor broadcasts rank 0's parameters, train.py:678-682; here every rank builds the
 * same parameters from the same seed / the same checkpoint file and the ranks COMPARE): out = {fp64 sum, fp64 sum of squares, low and
 * high 32 bits of a position-weighted wrapping integer sum of the bit patterns} of this rank's flat fp32 parameter buffer, computed on the
 * device in a fixed order (equal parameters give equal words on every rank; the integer word notices a single differing bit).  A
 * row-sharded model leaves out its own table rows (they differ by construction).  The host gathers the ranks' words through
 * rsys_allreduce_f64 with one slot per rank and every rank checks min == max (recommendersystem_amd/dist.py assert_replicas_equal:
 * after init, after resume, at every epoch end).  Synchronises. */
int32_t rsys_param_checksum(rsys_model* m, double out[4]);

/* raw views for hosts that run collectives themselves (e.g. torch.distributed on aliased memory) */
int32_t rsys_grad_buffer(rsys_model* m, void** dev_ptr, int64_t* n_floats);
int32_t rsys_param_buffer(rsys_model* m, void** dev_ptr, int64_t* n_floats);
int32_t rsys_refresh_shadow(rsys_model* m);   /* re-derive the bf16 compute copies after external parameter writes */

/* per-step time distribution (bench.py): rsys_step_mark records an event on the model's stream at an optimizer-step
 * boundary; rsys_step_marks_get writes the milliseconds between consecutive marks (at most cap) and clears the marks */
int32_t rsys_step_mark(rsys_model* m);
int32_t rsys_step_marks_get(rsys_model* m, float* ms_out, int32_t cap, int32_t* n_out);
int32_t rsys_op_timing(rsys_model* m, int32_t enable);  /* collect per-call-site HIP-event timings; 2: accepted, the same as 1;
                                                          * 3: pause -- stop recording without a host wait and keep the recorded spans for rsys_timing_get */
int32_t rsys_timing_get(rsys_model* m, char* buf, size_t cap);
/* time only the call sites whose name contains `substr` (NULL or "": all); cleared by rsys_op_timing(m, 0).  Call after rsys_op_timing(m, 1|2). */
int32_t rsys_op_timing_filter(rsys_model* m, const char* substr);
/* Environment switches (RSYS_*; the table is in DESIGN.md "Environment switches", the fields in csrc/switches.hpp).  The library parses the
 * environment when a model or communicator is created and at the entry of every rsys_op_* operator, never inside a training step;
 * rsys_switches_reload parses it on demand.  rsys_switches_describe writes "NAME=value" of the switches that differ from their defaults
 * (space separated, NUL terminated when it fits) and returns the number of characters that takes. */
int32_t rsys_switches_reload(void);
int32_t rsys_switches_describe(char* buf, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
