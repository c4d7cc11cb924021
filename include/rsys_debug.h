/* rsys_debug.h -- TEST AND PARITY HOOKS of librsys_hip.so.  Not part of the drop-in boundary: a host that trains or serves binds
 * include/rsys.h only.  These entry points exist for the parity suite (tests/), the micro benchmarks (tools/) and
 * bench.py's per-kernel timing: bit-exact read-back of the index paths, raw per-kernel access on caller-provided device buffers,
 * an in-process rank group that lets the multi-rank arithmetic run on a one-GPU box, and a delay kernel for cross-stream ordering
 * tests.  Same conventions as rsys.h (status codes, rsys_last_error, opaque handles). */
#ifndef RSYS_DEBUG_H
#define RSYS_DEBUG_H
#include "rsys.h"

#ifdef __cplusplus
extern "C" {
#endif

/* debug/parity: integer and index paths of the last forward, read back bit-exactly (tests compare them with the
 * reference's mask_tokens, model.py:417-462, and position selection, model.py:501-513).  Keys: "masked.token_mask_ids",
 * "masked.matchedid", "masked.status" (int32 [rows*S]); "masked.rating", "masked.progress" (f32); "masked.<medium>.
 * <watch|rating>.<label|weight|position>"; "idx.<task>" (int32 [mask_topk*rows], task = medium*2 + metric); "npos"
 * (int32 [4]); "tokens.userid", "tokens.token_mask_ids" (int32 [rows*2S], model.py:468-469); "embed.x0" (f32
 * [rows*2S*D]); "table.fused" (f32 [(V+1)*D]); after a training pass also the compact top of the trunk: "top.cap",
 * "top.n" (int32 [1]: capacity / number of selected tokens), "top.sel" (int32 [top.cap], the sorted selected tokens), "top.slot"
 * (int32 [rows*2S], token -> compact row or -1); "host_syncs" (int32 [2]: stream drains and event waits inside the last
 * rsys_forward_backward).  `bytes` must be the exact size of the array. */
int32_t rsys_debug_get(rsys_model* m, const char* key, void* out, int64_t bytes);

/* in-process rank group (tests): `world` ranks of ONE process on one device, each driven by its own host thread; the
 * collectives are device copies between the ranks' buffers.  Two RCCL ranks cannot share a GPU; this lets the multi-rank
 * partition arithmetic run on a one-GPU box with the real kernels. */
int32_t rsys_local_group_create(int32_t world, int32_t device, void** group);
int32_t rsys_local_group_destroy(void* group);
int32_t rsys_comm_init_local(void* group, int32_t rank, rsys_comm** out);
/* tests: occupy the communicator's stream for `microseconds` (<= 2e6) with a spinning kernel -- a collective that starts late; what
 * the cross-stream ordering test of the split table reduce delays (tests/test_gpu_split_table_reduce.py) */
int32_t rsys_comm_debug_delay(rsys_comm* c, int32_t microseconds);

/* per-kernel access for unit tests (device pointers from rsys_dev_alloc) */
int32_t rsys_dev_alloc(void** p, size_t bytes);
int32_t rsys_dev_free(void* p);
int32_t rsys_dev_h2d(void* dst, const void* src, size_t bytes);
int32_t rsys_dev_d2h(void* dst, const void* src, size_t bytes);
int32_t rsys_dev_memset(void* dst, int value, size_t bytes);
/* C[M,N] = sum_k A(m,k)B(n,k); dtype RSYS_DTYPE_*; a_km/b_km: operand stored K-major; a_f32: A is f32 in memory */
int32_t rsys_op_gemm(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K,
                     int64_t lda, int64_t ldb, int64_t ldc, int32_t a_km, int32_t b_km, int32_t a_f32, int32_t c_f32,
                     int32_t splitk);
/* the same product with the row count taken from device memory, as the head GEMMs over the selected positions do
 * (model.py:501-516: only rows with a positive target weight reach the heads): rows >= *rows_dev are not computed
 * (rows up to the end of the last started tile may be written); row-major A, c_f32 / b_km as above; c_f32 == 3: fp32 C ACCUMULATED by
 * split-K atomics (the tied head's dEw = dlogits . F) */
int32_t rsys_op_gemm_rows(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K,
                          int64_t lda, int64_t ldb, int64_t ldc, int32_t b_km, int32_t c_f32, const int32_t* rows_dev);
/* K-major operands (A [K][lda >= M], B [K][ldb >= N]), f32 C stored (accumulate = 0) or added to (1), the reduction limited to the first
 * *k_dev rows of the operands (device memory): the tied head's table gradient dF (+)= dlogits^T Ew over the live selected rows
 * (model.py:153-170 backward); rows >= *k_dev may hold anything */
int32_t rsys_op_gemm_klimit(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K,
                            int64_t lda, int64_t ldb, int64_t ldc, int32_t accumulate, const int32_t* k_dev);
/* one launch_gemm call with any fused epilogue but EPI_ATOMIC (GemmEpi, csrc/gemm.hpp: 0 store, 1 accumulate, 3 bias, 4 residual, 5 QKV +
 * RoPE, 6 SwiGLU, 7 table, 8 GELU, 9 SwiGLU backward), row-major A, one K split; synchronises.  Fields as in GemmParams; T = the dtype.
 *   A [M][lda >= K], B [N][ldb >= K] or with b_km [K][ldb >= N], T-typed, 16-byte aligned, rows padded to 16 bytes.
 *   C [M][ldc]: fp32 when c_f32 != 0 and always for epi 1, 4 and 7, else T-typed; ldc % 4 == 0 (T = bf16 outputs: % 8).  Only columns
 *     < N of rows < M are written (epi 9: columns < 2 N); with m_dev see below.
 *   alpha: epi 0 and 5 store alpha * acc (the register epilogues take alpha != 1 for epi 0 only).  accum != 0: epi 0 / 5 with a T-typed
 *     C add the result to what C holds (the 128x128 kernel only).
 *   bias [N] f32: epi 3 C = acc + bias; epi 7; epi 8.      resid [M][ldr] f32: epi 4 C = resid + acc.      epi 1: C += acc.
 *   epi 6: N % 32 == 0, the columns come in blocks [16 a | 16 b]; C = the [a|b] values as they are, C2 [M][ldc2 >= N / 2] (T) =
 *     silu(a) b, block u of 16 columns from the u-th [a|b] block.
 *   epi 9: N % 16 == 0 is the width of acc = dg; C2 [M][ldc2] (T, ldc2 == ldc) holds the saved [a|b] blocks (2 N columns), C (T) gets
 *     [da|db] in the same blocks: da = dg b s (1 + a (1 - s)), db = dg a s, s = sigmoid(a).
 *   epi 7: f = acc + E + bias with E [M][...] f32 READ WITH STRIDE ldc (it has no stride of its own); C (fp32) = f, C2 [M][ldc2] (T) = f.
 *   epi 8: z = acc + bias; C (T) = z, C2 [M][ldc2] (T) = z (1 + erf(z / sqrt 2)) / 2.
 *   epi 5: columns [0, n_q) are q, [n_q, n_q + n_k) k, the rest v; q and k are whole heads of hd columns (hd a power of two >= 16) and
 *     each interleaved pair (x0, x1) = columns (2 d, 2 d + 1) of a head becomes (x0 c - x1 s, x0 s + x1 c) with c = rope_cos[pos][d],
 *     s = rope_sin[pos][d] (tables [positions][hd / 2] f32); pos = rope_pos[row] (int32 [M], values inside the tables) or, when null,
 *     row % T.  rope_cs: the same values as [pos][hd / 2][2] = (cos, sin); the 256x256 family needs it and reads ONLY it (without it
 *     the product runs on the 128x128 kernel, which reads only the two plain tables).  The register epilogue rotates the v columns
 *     too, with table row 0: ROW 0 MUST BE (cos 1, sin 0) -- position 0 of a true RoPE table.
 *   m_dev (device int, may be null): tiles whose first row is >= *m_dev are not computed; rows < min(*m_dev, M) are written, rows up to
 *     the end of the last started tile (128 rows; 256 in gemm8p and gemm8c's full form) may be, later rows are untouched.
 * It fills no fp8 field.  `tag` gets the timing tag of the kernel that ran (as rsys_debug_gemm_route) and *half whether that was gemm8c
 * in its HALF form (128 x 256 tiles), both decided by the code launch_gemm runs, from the RSYS_GEMM* switches as the call parsed them. */
int32_t rsys_op_gemm_epi(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                         int64_t ldb, int64_t ldc, int32_t b_km, int32_t c_f32, int32_t epi, float alpha, int32_t accum,
                         const float* bias, const float* resid, int64_t ldr, void* C2, int64_t ldc2, const float* E,
                         const float* rope_cos, const float* rope_sin, const float* rope_cs, const int32_t* rope_pos, int32_t T,
                         int32_t hd, int32_t n_q, int32_t n_k, const int32_t* m_dev, char* tag, int32_t tag_bytes, int32_t* half);
/* the kernel launch_gemm would run for this problem, decided on the host without launching anything: `tag` gets its timing tag
 * ("nt", "nn", "tn", "8p", "8c", "4p", "8t", "4k", "8ts", "8s", "8m"), `splits` the K-split count it runs with.  Fields as in
 * GemmParams (csrc/gemm.hpp); `set` says which pointer fields the problem has: bit 0 m_dev, 1 k_dev, 2 slab, 3 rope_cs, 4 rope_pos,
 * 5 C2.  `cus`: the CU count the route assumes.  Reads the RSYS_GEMM* switches as parsed last (rsys_switches_reload). */
int32_t rsys_debug_gemm_route(int32_t dtype, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t a_km,
                              int32_t b_km, int32_t a_f32, int32_t c_f32, int32_t epi, int32_t splitk, int32_t flags, float alpha,
                              int32_t accum, int32_t set, int32_t m_expect, int32_t cus, char* tag, int32_t tag_bytes, int32_t* splits);
/* the host side of rsys_batch_upload (row_len == max_sequence_length) and rsys_batch_upload_trimmed (a shorter row_len) alone, on the
 * host only: the check of batch `b` and the packing of columns [0, row_len) of its rows into the caller's buffer `stage` of
 * stage_bytes bytes, exactly as an upload fills its staging buffer -- no model, no device, no HIP call.  limits = {max_rows,
 * max_sequence_length, RoPE table positions (2 max_sequence_length in a model), V = vocab_0 + vocab_1, vocab_0, vocab_1, vocab_status,
 * vocab_gender, vocab_source}.  offsets [30]: where each array starts in `stage`, in the order the layout places them -- time,
 * userid, token_mask_ids, gender, source, matchedid, status, rating, progress, then label / weight / position of target 0 .. 5, then
 * watch_mask, rating_mask and the token positions (2 p, 2 p + 1 per rope_input_pos p); an array the batch or the form does not have
 * keeps its place and stays unwritten.  *total_bytes: the end of the last array; *distinct_ids: the distinct matchedid values >= 0 of
 * the packed columns + 1.  A rejected batch (RSYS_ERR_ARG) writes nothing; a buffer below *total_bytes is RSYS_ERR_STATE. */
int32_t rsys_debug_batch_pack(const rsys_batch* b, const int32_t limits[9], int32_t row_len, void* stage, int64_t stage_bytes,
                              int64_t offsets[30], int64_t* total_bytes, int32_t* distinct_ids);
/* attention fwd+bwd on caller-provided device buffers (T-typed): qkv [B*T][(H+2KV)*hd] post-RoPE, dO [B*T][H*hd],
 * uid/tm [B*T] int32 with 0 <= uid < 2^19 and 0 <= tm < 4096, rope tables [T][hd/2] f32; outputs O [B*T][H*hd], lse [B][H][T] f32,
 * dqkv [B*T][(H+2KV)*hd] (gradients w.r.t. the un-rotated q, k and v).  T a multiple of 8, T <= 4096 (64 tiles of 64 tokens: rows of
 * more than 2048 tokens run the kernels' 64-bit tile-map instantiations), a row of qkv below 2 GiB */
int32_t rsys_op_attention(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv,
                          const int32_t* uid, const int32_t* tm, void* O, float* lse, const void* dO, void* dqkv,
                          const float* rope_cos, const float* rope_sin);
/* the same launches with the remaining AttnParams fields (csrc/kernels.hpp); rsys_op_attention is this call with all of them null and
 * rope_rows = T.  rope tables [rope_rows][hd/2] f32.  rope_pos (device int32 [B*T], or null: token t of a row has position t): the
 * table row each token's gradient is un-rotated with; the host copies it back once and checks 0 <= pos < rope_rows (null: rope_rows
 * >= T).  q_active (device int32 [B], or null): only the first q_active[b] 64-token query tiles of row b matter -- O / lse of the
 * others are not written, their dq rows are zeros, and dk / dv leave them out (THEIR dO ROWS MUST BE ZERO); delta of those tiles is
 * NaN during the call.  amax_fwd / amax_bwd (device, 64 shards of 32 floats each, zeroed by the caller, or null): AttnParams::f8_amax
 * of the forward / the backward launches -- the maximum over the shards of element 0 of amax_fwd = max |O|, of elements 0 / 1 / 2 of
 * amax_bwd = max |dq| / |dk| / |dv|, of the stored (rounded) values */
int32_t rsys_op_attention_ex(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv,
                             const int32_t* uid, const int32_t* tm, void* O, float* lse, const void* dO, void* dqkv,
                             const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows,
                             const int32_t* q_active, float* amax_fwd, float* amax_bwd);
/* the selected-query attention of the serving compact top alone (attn_sel_kernel), on caller-provided device buffers: qkv
 * [B*T][(H+2KV)*hd] (T-typed, q and k already rotated), uid / tm int32 [B*T], sel int32 [n_sel] (device; flat token indices b * T + t, any
 * order, duplicates allowed; copied back once and checked).  Query sel[i] attends to the keys of its row under the model's mask (key k
 * allowed iff uid[k] == uid[q] and (tm[k] == 0 or tm[k] == tm[q])), one soft-max at scale 1/sqrt(hd); its H*hd outputs go to row i of O
 * [>= n_sel][H*hd] (T-typed).  Rows of O from n_sel on are not written; there is no lse.  The tile maps are built here, as in
 * rsys_op_attention_ex (T a multiple of 8, T <= 4096; rows of more than 2048 tokens use the 64-bit map words) */
int32_t rsys_op_attention_selected(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv,
                                   const int32_t* uid, const int32_t* tm, int32_t n_sel, const int32_t* sel, void* O);
/* the tile maps, pair bits and launch orders of an attention launch alone (launch_attn_tilemap, csrc/attention_maps.hip), built as
 * rsys_op_attention_ex and rsys_op_attention_selected build them before their first attention kernel; no attention kernel runs.  dtype,
 * KV and hd only decide the query heads per workgroup and whether order_k lists kv tile pairs.  uid / tm (device int32 [B*T]) are copied
 * back and checked: 0 <= uid < 2^19, 0 <= tm < 4096; q_active (device int32 [B], or null): 0 <= q_active[b] <= nt = ceil(T / 64); T a
 * multiple of 8, T <= 4096, H a multiple of KV; RSYS_ERR_ARG otherwise, with nothing launched.  Every byte of the map set holds 0xA5
 * before the first launch.  uid_prev / tm_prev (device, both or neither): launch_attn_tilemap runs on them first, into the same set.
 * Outputs, HOST buffers, W = 32-bit words for nt <= 32, else 64-bit: qmap / kmap / qmap_full / kmap_full W [B][nt]; qmap16 / kmap16
 * W [B][nt][4]; qbits uint64 [B][nt q][nt kv][64 queries], kbits uint64 [B][nt kv][nt q][64 keys]; order_q int32 [B*H*nt] and order_k
 * int32 [B*KV*nt], the whole buffers (the lists sit back to back at their start, 0xA5 behind them); info int32 [8] = 32-bit words per
 * map entry, query heads per workgroup, kv tile pairs (0 / 1), eight XCD lists (1) or one list (0), slots per (row, kv head) on the
 * q side, on the k side, identity fallback taken (0 / 1), nt */
int32_t rsys_op_attention_maps(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const int32_t* uid, const int32_t* tm,
                               const int32_t* q_active, const int32_t* uid_prev, const int32_t* tm_prev, void* qmap, void* kmap,
                               void* qmap_full, void* kmap_full, void* qmap16, void* kmap16, uint64_t* qbits, uint64_t* kbits,
                               int32_t* order_q, int32_t* order_k, int32_t* info);
/* the candidate attention of rsys_rank_cache_candidates alone, on caller-provided device buffers (T-typed): qkv [rows*T][(H+2KV)*hd] the
 * candidate rows' post-RoPE q | k | v, cache [n_slots][T][2*KV*hd] (K | V per cached token), slot / n_hist / n_cand int32 [rows] (device;
 * 0 <= n_hist[r] <= T/2, 0 <= n_cand[r] <= T/2; T a multiple of 8, T <= 4096); O [rows*T][H*hd]: rows of tokens >= 2 n_cand[r] are zeros up to the end of the last
 * 64-token tile that holds a candidate and left as they were behind it */
int32_t rsys_op_attention_cached(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const void* cache,
                                 int32_t n_slots, const int32_t* slot, const int32_t* n_hist, const int32_t* n_cand, void* O);
/* the candidate attention of rsys_rank_cache_candidates_packed alone (attn_cand_tiles_kernel), buffers as above: seg (HOST int32 [n_seg][5]) =
 * (row, first_tile, n_cand, slot, n_hist): the segment's candidate j sits at tokens 64 first_tile + 2 j, + 1 of its row and reads the 2 n_hist
 * cached tokens of slot; segments lie inside their rows and share no 64-token tile (RSYS_ERR_ARG otherwise); cache [n_slots][Tc][2*KV*hd]
 * (Tc = 0: T).  O: a tile no segment covers is left as it was; rows of tokens behind a segment's candidates are zeros up to the end of its last tile */
int32_t rsys_op_attention_cached_tiles(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const void* cache,
                                       int32_t n_slots, int32_t Tc, int32_t n_seg, const int32_t* seg, void* O);
/* the copy of rsys_rank_cache_store_packed alone (rank_cache_copy_segments_kernel): seg (HOST int32 [n_seg][4]) = (row, first column c0, n_hist,
 * slot); K | V of tokens [2 c0, 2 c0 + 2 n_hist) of the row of qkv [rows*T][(H+2KV)*hd] -> rows [0, 2 n_hist) of the slot of cache
 * [n_slots][Tc][2*KV*hd] (Tc = 0: T); nothing else is written */
int32_t rsys_op_rank_cache_copy_segments(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, void* cache,
                                         int32_t n_slots, int32_t Tc, int32_t n_seg, const int32_t* seg);
/* K | V rows a ranking-cache slot holds for one layer: out (host) [2 n_hist][2*KV*hd] in the compute dtype; bytes must be exact */
int32_t rsys_rank_cache_get(rsys_model* m, int32_t layer, int32_t slot, void* out, int64_t bytes);
/* the selection of rsys_retrieve_topk alone, on caller-provided device buffers: per row r of scores [rows][ld >= V] the min(k, admissible)
 * best columns by descending value, ties by ascending column, -inf / NaN excluded, -0.0 == +0.0; ids / vals [rows][k] (padding -1 / -inf),
 * counts [rows]; 1 <= k <= min(V, 8192), 1 <= rows <= 65535 */
int32_t rsys_op_topk(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k,
                     int32_t* ids, float* vals, int32_t* counts);
/* the windowed selection of rsys_retrieve_window alone (win_*_kernel), on caller-provided device buffers: per row r of scores
 * [rows][ld >= V] the ranks [start[r], start[r] + len[r]) of rsys_op_topk's ordering; start (int64) and len are HOST arrays, 1 <= len <= 1024,
 * start >= 0, 1 <= rows <= 65535.  ids / vals [rows][1024] (padding -1 / -inf), counts [rows] = clip(total - start, 0, len), totals [rows] =
 * the admissible count.  bounds (device, may be NULL) [rows][2][2] = (threshold key T as its uint32 bits, need) of the window's end bound
 * and of its start bound after the select: the top-c set of a bound is every key above T plus the first `need` keys equal to T by
 * ascending id; need == 0 with T != 0 and T != 0xffffffff is the "between two keys" form (T = a bin's smallest key - 1) */
int32_t rsys_op_topk_window(const float* scores, int64_t ld, int32_t rows, int32_t V, const int64_t* start, const int32_t* len,
                            int32_t* ids, float* vals, int32_t* counts, int32_t* totals, int32_t* bounds);
/* the log-sum-exp of rsys_retrieve_topk's scoring alone (lse_partial_kernel, lse_final_kernel: 64 slices per row, online max, a fixed
 * fold order), on device buffers: lse[r] = log sum_i exp(z[r][i]) over i < V of z [rows][ldz >= V]; 1 <= rows <= 65535.  -inf entries add
 * nothing; a row that is all -inf gives -inf (every item of such a query is then NaN or -inf downstream and excluded); rows are expected to hold no NaN */
int32_t rsys_op_lse(const float* z, int64_t ldz, int32_t rows, int32_t V, float* lse);
/* the scoring of rsys_query_texts_set alone, to HOST outputs: z_out [n][V_m] = the logits of n texts x [n][Q] (host) over the search
 * handle's items and lse_out [n] = their log-sum-exp, the same bits the setter computes; 1 <= n <= min(64, the handle's max_batch).
 * Like the setter it rewrites the handle's query and projection buffers, so rsys_search_debug_get has no forward to report until the next one */
int32_t rsys_op_text_rows(void* search, const float* x, int32_t n, float* z_out, float* lse_out);
/* the three weighted accumulations of rsys_query_weights_set alone, one launch each on caller-provided DEVICE buffers (host: cand_offsets,
 * retrieval_coef, rating_coefs); a section runs when its output is not NULL.  Shared by the first two: z [rows][ldz] and lse (indexed by
 * query / user q, row q - q0 of z), members (the queries of every group, group by group), ranges int32 [n_groups][2] = the slice of
 * members each group adds in this launch, user_w indexed as lse.
 * dst != NULL (combine_w_kernel): dst[g][i] = src[g][i] + sum of w_q * (z_q[i] - lse_q), rows of V floats; last != 0 writes the
 *   order-preserving uint32 key of the score instead (0 = NaN / -inf); last == 0 leaves the row of a group with an empty range unwritten.
 * sc != NULL (rank_score_w_kernel): groups of cand_offsets[g + 1] - cand_offsets[g] <= 1024 candidates cand (column ids of z);
 *   sc[c] = (first ? 0 : sc[c]) + sum of w_u * (lp_u + r_u), r_masked ragged with user u's values at rm_offsets[u] (int64, device).
 * S != NULL (selected_sum_w_kernel): S[g][dim] = sum over a in [sel_offsets[g], sel_offsets[g + 1]) (int64, device) of sel_w[a] * x_a,
 *   x_a = emb_m[sel_ids[a]] when sel_medium[a] == medium, else X[a] (rows of dim floats). */
int32_t rsys_op_query_weights(const float* z, int64_t ldz, const float* lse, const int32_t* members, const int32_t* ranges, int32_t q0,
                              const float* user_w, int32_t n_groups, const float* src, float* dst, int32_t V, int32_t last,
                              const int64_t* cand_offsets, const int32_t* cand, const float* r_masked, const int64_t* rm_offsets,
                              const float* retrieval_coef, const float* rating_coefs, float rating_mean, int32_t first, float* sc,
                              const int64_t* sel_offsets, const int32_t* sel_medium, const int32_t* sel_ids, int32_t medium, const float* emb_m,
                              const float* X, int32_t dim, const float* sel_w, float* S);
/* the count of rsys_retrieve_target_rank alone, on caller-provided device buffers: per row r of scores [rows][ld >= V] (NaN or -inf marks
 * an inadmissible entry, -0.0 == +0.0) rank_out[r] = 1 + #{admissible i : s_i > s_t} + #{admissible i < t : s_i == s_t} with
 * t = targets[r] in [0, V), or 0 when s_t is NaN or -inf; 1 <= rows <= 65535 */
int32_t rsys_op_target_rank(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* targets, int32_t* rank_out);
/* the count of rsys_sim_pair_ranks alone: scores [rows][ld >= V] is a DEVICE array of final (already masked) score rows; self [rows],
 * tgt_offsets [rows + 1], tgt_ids and ranks_out [tgt_offsets[rows]] are host arrays.  Per row r with s = self[r] and every target t of its
 * CSR slice: ranks_out = 1 + #{i != s : v_i sorts above v_t} + #{i != s, i < t : v_i equal to v_t} under isless (-inf < ... < -0.0 < +0.0
 * < ... < +inf < NaN, all NaNs equal), 0 where t == s.  Columns >= V are never read.  1 <= rows <= 65535 */
int32_t rsys_op_pair_ranks(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* self, const int64_t* tgt_offsets,
                           const int32_t* tgt_ids, int32_t* ranks_out);
/* the masked score rows rsys_sim_pair_ranks ranks: out[n_src][V] (host) = v[sources[s]][:], from the same row gather, GEMM and mask
 * arithmetic (the mask is applied by a kernel of its own here, on load in the ranking) */
int32_t rsys_sim_pair_scores(void* h, int32_t n_src, const int32_t* sources, float* out);
/* rsys_rank_request's Gram matrices alone, as its loop reads them: out = per group in order, G_g [n_g][n_g] row-major (sum of n_g^2 floats),
 * computed by the same kernel from the model's item-similarity table of `medium`; host arrays */
int32_t rsys_rank_gram_get(rsys_model* m, int32_t medium, int32_t n_groups, const int64_t* cand_offsets, const int32_t* cand_ids,
                           float* out, int64_t n_out);
/* rsys_rank_request's greedy loop alone for one group, on caller-provided device buffers: r [n], gram [n][n] (row b is read as column b),
 * ss_bits [n][ceil(n / 32)] (bit i of row j: candidate i is a stored row of related's column ids[j]), related_bits [ceil(n / 32)] (the
 * flags); pen[4] (host) = (decay, mmr, same_series, related); picks [min(partialk, n)] = the position chosen per round; 1 <= n <= 1024 */
int32_t rsys_op_rerank(int32_t n, int32_t partialk, const float* pen, const float* r, const float* gram, const int32_t* ss_bits,
                       const int32_t* related_bits, int32_t* picks);
/* rsys_render_request's intermediates.  rsys_render_debug_keep(m, 1): every following request copies its intermediates to host memory as
 * it goes (off again with 0, which also drops them).  rsys_render_debug_get: *bytes = the size of the array kept under `key` by the last
 * request; it is copied to out when out != NULL and cap >= *bytes.  Keys: "forwards" int32 [2] (forwards of the last request: retrieval,
 * ranking; kept always); "queries" f32 [n_users][D] (the query buffer, user order); "ret.counts" int32 [n_groups]; "ret.ids" int32 (the
 * groups' retrieved ids, counts[g] each, group order); "rows" int32 [n_rows][6] = (user, group, first candidate slot, candidates, row in
 * its wave, wave) per ranking row in run order; "batch.<array>" (userid, token_mask_ids, gender, source, matchedid, status, rope_input_pos
 * int32; rating, progress f32; time f64) [n_rows][S], the assembled ranking rows; "token_index" int32 (the rows' action tokens, flat within
 * their wave); "groups" int32 [n_active][6] = (group, medium, first slot in "r" / "picks", candidates, sidx, eidx) per group with a page;
 * "rm_users" int32 [n][3] = (user, first value in "r_masked", values); "r_masked" f32; "r" f32 (ranking scores) and "picks" int32 (picked
 * positions; the slots after a group's eidx rounds hold -1).
 * "forward_rows" int32 [n_forwards][3] = (stage, rows, row_len) of every trunk forward of the last request in run order (kept always): stage
 * 0 = retrieval wave, 1 = store wave, 2 = candidate rows against the cache, 3 = assembled rows; row_len < S only under
 * rsys_serving_trim_set.  The kept batches are what the switch-off call keeps, shapes [n][S] and values: trimmed rows are widened with what
 * the full rows hold behind them (zeros; rope_input_pos: the row's fill position), token indices are reported as r * 2S + t.
 * After rsys_render_request_full: "forwards" [1] counts every ranking-stage forward; "forwards.full" int32 [3] = (store forwards, candidate
 * forwards, empty-history chunk forwards; kept always); "store.<array>" the store rows [n_store_rows][S] in run order with "store.rows"
 * int32 [n][4] = (user, slot, events, wave); "cand.<array>" the candidate rows of the cached path with "cand.token_index"; "rows" int32
 * [n_rows][7] = (user, group, first candidate slot, candidates, row in its forward, forward, kind): kind 0 = a candidate row of the cached
 * path (forward = index among the candidate forwards), kind 1 = an assembled row of a user with an empty history (forward = index among
 * those forwards; its arrays under "batch.<array>" / "token_index" as above); the cached rows come first. */
int32_t rsys_render_debug_keep(rsys_model* m, int32_t on);
int32_t rsys_render_debug_get(rsys_model* m, const char* key, void* out, int64_t cap, int64_t* bytes);
/* the last rsys_sim_forward_backward / rsys_sim_ndcg call of an item-similarity handle (host arrays): "ranks" int32 [n_q][n] (1-based
 * order of each slot), "scores" f32 [n_q][n] (x), "dldx" f32 [n_q][n] (d batch loss / dx), "dropout_mask" uint8 [rows][F] (1 = kept, the
 * mask of every gathered row: rows = 2 n_q n in training, [source copies | targets], slot-major; all ones without dropout), "splits"
 * int32 [1] (the K-split count the last call's dW product ran with, as routed: the requested count rounded by the GEMM route; 0 when the
 * call ran no backward) */
int32_t rsys_sim_debug_get(void* h, const char* name, void* out, int64_t n);
/* the last rsys_search_forward_backward / rsys_search_topk call of a search handle (host arrays, f32): "lse" [B] (the per-row logsumexp of
 * the logits), "dP" [B][D] (d loss / d (x Wenc) in fp32, before the bf16 mode rounds it for dWenc; training calls only), "splits" [2] (the
 * column splits the row statistics of the last call ran with, and the K-split count its dP product ran with as routed, 0 when the call
 * ran no backward) */
int32_t rsys_search_debug_get(void* h, const char* name, float* out, int64_t n);
/* embedding-gradient scatter of the backward (nn.Embedding backward, model.py:21) on caller-provided device buffers:
 * gE[id'] += sum over tokens n of gx0[n*ldx .. +D) with id' = m_matchedid[n] (-1 -> row V); matchedid = the raw ids the
 * token index is built from (m_matchedid differs from it only where it is -1).  One writer per table row, fixed summation
 * order: bitwise reproducible.  atomic != 0: the float-atomic form (A/B reference; needs ldx == 2 D). */
int32_t rsys_op_embedding_scatter(const float* gx0, int64_t ldx, const int32_t* matchedid, const int32_t* m_matchedid, int32_t N,
                                  int32_t V, int32_t D, float* gE, int32_t atomic);
/* fp8 trunk (RSYS_DTYPE_FP8: the reference's torchao "tensorwise" float8 linears, transformer.py:671-676), unit-test access on
 * caller-provided device buffers.  fmt: 0 = e4m3, 1 = e5m2.
 * rsys_op_f8_quantize: amax_dev (64 shards of 32 floats; the maximum over the shards of element seg) = max |src| per column segment (layout 0: one; 1: column units of seg_cols, the first seg_rep
 *   units are segment 0 and every further unit its own segment -- q | k | v with grouped-query heads; 2: the [16 a | 16 b] column
 *   blocks of the W13 output, two segments), then dst = sat_rne(src * FMAX / amax) as fp8 bytes (layout 2: columns de-interleaved
 *   to [all a | all b]); src bf16 [rows][cols].  desc_mode 1 / 2 also writes the descales a consumer GEMM takes (1: desc[u] =
 *   1 / (s_src s_w[weight of output unit u]) for n_w weight amaxes, the first w_rep units on weight 0; 2: K segments, desc[0] =
 *   last segment, desc[16 + j] = ratios); desc_dev holds 32 floats.
 * rsys_op_f8_weights: the same for one fp32 weight matrix [rows][cols] (row segments), plus its transposed copy dst_t [cols][ld_t].
 * rsys_op_gemm_f8: C[M,N] = descale * sum_k A8[m][k] B8[n][k] on the 256x256 fp8 pipeline (K % 128 == 0, K >= 256); a_fmt as fmt,
 *   B is e4m3; desc_dev / seg_cols / alt / kb0..kb2 as GemmParams::f8_* (csrc/gemm.hpp); C bf16 or f32. */
int32_t rsys_op_f8_quantize(const void* src, int64_t ld_src, int32_t rows, int32_t cols, int32_t fmt, int32_t layout, int32_t seg_cols,
                            int32_t seg_rep, void* dst, int64_t ld_dst, float* amax_dev, float* desc_dev, const float* wamax_dev,
                            int32_t n_w, int32_t w_rep, int32_t desc_mode);
int32_t rsys_op_f8_weights(const float* src, int64_t ld, int32_t rows, int32_t cols, int32_t layout, int32_t seg_rows, int32_t seg_rep,
                           float* amax_dev, void* dst, void* dst_t, int64_t ld_t);
int32_t rsys_op_gemm_f8(const void* A8, const void* B8, void* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                        int32_t a_fmt, int32_t c_f32, const float* desc_dev, int32_t seg_cols, int32_t alt, int32_t kb0, int32_t kb1,
                        int32_t kb2);
/* The grouped weight-gradient launch (csrc/gemm8p.hip: gemm8p_group_plan_create + launch_gemm8p_group), one plan of n products
 * C_i[M_i][ldc_i] += A_i^T B_i with fp32 atomics, built as the training step builds them (c_f32, EPI_ATOMIC, alpha 1).  Host arrays of
 * n entries each; A / B / C / f8_desc hold device pointers.
 *   bf16 products (f8[i] == 0, desc / rseg / rowmode 0): K-major operands A [K][lda >= M], B [K][ldb >= N], M, N, lda, ldb % 8 == 0.
 *   fp8 products (f8[i] == 2): A e5m2 [M][lda >= K], B e4m3 [N][ldb >= K], K % 128 == 0, K >= 256, lda, ldb % 16 == 0, N % 8 == 0;
 *     f8_desc[i] = 32 device floats, output row r scaled by desc[r / f8_rseg] (f8_rseg 0: desc[0]; at most 16 segments);
 *     f8_rowmode 1 (M % 32 == 0): row r is added to row (j >> 4) * 32 + is_b * 16 + (j & 15), j = r - is_b * M / 2 (GemmParams::f8_*).
 *   One form per plan.  ordered != 0 (bf16 only, N % 4 == 0 and ldc % 4 == 0, C 16-byte aligned): the deterministic form, per-product
 *     slabs cleared per launch and summed in split order.
 *   launches >= 1: the one plan is launched that many times (C accumulates), then the call synchronises and destroys the plan.
 * Reads the switches as the call parses them (RSYS_GEMM4K, RSYS_DEBUG_8G_SPLITK).  *splitk_out = the plan's K-split count, *kernel_out
 * = the kernel launch_gemm8p_group ran (RSYS_GROUP_KERNEL_*).  What the plan refuses is RSYS_ERR_ARG with nothing launched.
 * rsys_op_gemm_f8_splitk: one fp8 product of that form through launch_gemm8p_f8_splitk (its own K-split count), `launches` times. */
#define RSYS_GROUP_KERNEL_8G 0  /* gemm8p_group_kernel (bf16, eight waves; also the ordered form) */
#define RSYS_GROUP_KERNEL_4KG 1 /* gemm4k_group_kernel (bf16, the default where every product is eligible) */
#define RSYS_GROUP_KERNEL_8GF 2 /* gemm8p_group_f8_kernel */
int32_t rsys_op_gemm_group(int32_t n, const void* const* A, const void* const* B, void* const* C, const int32_t* M, const int32_t* N,
                           const int32_t* K, const int64_t* lda, const int64_t* ldb, const int64_t* ldc, const int32_t* f8,
                           const float* const* f8_desc, const int32_t* f8_rseg, const int32_t* f8_rowmode, int32_t ordered,
                           int32_t launches, int32_t* splitk_out, int32_t* kernel_out);
int32_t rsys_op_gemm_f8_splitk(const void* A8, const void* B8, void* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb,
                               int64_t ldc, const float* desc_dev, int32_t rseg, int32_t rowmode, int32_t launches);
/* row kernels between the products and the optimiser (csrc/elementwise.hip, csrc/optim.hip), unit-test access on caller-provided
 * device buffers; each calls the training step's launcher unchanged and synchronises.  dtype RSYS_DTYPE_FP32 / BF16 = the T of the
 * launcher (the storage type of y, g, dx_t, logits, z, hact; the shadow copy of AdamW).  deterministic != 0: the call runs with
 * deterministic-mode scratch of its own (per-workgroup partial sums added in a fixed order) and fails if the launch did not take that
 * branch.  Optional pointers may be null.
 * rsys_op_rmsnorm_fwd: y = x rstd scale, rstd = 1 / sqrt(mean x^2 + 1e-5) (model.py:193-202); x, scale, rstd f32 [rows][D] / [D] /
 *   [rows].  rows_dev (device int): rows [0, *rows_dev) live, rows up to the next multiple of 256 (and below `rows`) written as
 *   zeros, the rest untouched; in_rows (device int [rows]): output row r from input row in_rows[r]; amax (64 shards of 32 floats,
 *   zeroed by the caller): max |y| after the storage rounding, in element 0 of the shards.
 * rsys_op_rmsnorm_bwd: dx = resid + r g scale - x r^3 sum(g scale x) / D, dx_t its dtype copy (+ amax as above), dscale += sum over
 *   rows of g x r; g is dtype-typed, or f32 with g_f32 != 0 (the final norm; resid_slot, io_rows null).  resid_slot (device int
 *   [rows]): the residual is row resid_slot[r] of resid, none where -1; io_rows (device int [rows]): x read at, dx / dx_t written to,
 *   row io_rows[r]; rows_dev as in the forward (not together with io_rows).
 * rsys_op_ce: per row r < n of logits [n][ldl >= V] with i = idx[r]: loss[0] += (lse - logit[position[i]]) label[i] weight[i], and the
 *   row is overwritten with task_w label[i] weight[i] / max(stats[0], 1e-8) (softmax - onehot), zero in columns >= V and in rows whose
 *   label weight is zero; rows from round_up(*npos, 128) on are untouched.  Requires 0 <= position[i] < V where label weight != 0.
 * rsys_op_rating_tail: pred = hact[r].w2 + b2, e = pred - (label[i] - rating_mean); loss[0..2] += weight[i] (e^2, t^2, (-pred - t)^2);
 *   unless evaluate: dpred = 2 task_w e weight[i] / max(stats[0], 1e-8), z[r] overwritten with dpred w2 gelu'(z[r]), dw2 += dpred
 *   hact[r], db0 += that dz, db2 += dpred; rows from round_up(*npos, 128) on are skipped.
 * rsys_op_sumsq: *out = sum of g[0, n)^2 in a fixed order (g 16-byte aligned).
 * rsys_op_clip_adamw: *sumsq = |g|^2; then fused != 0: AdamW with the clip coefficient min(1, max_norm / (|g| / grad_div + 1e-6)) /
 *   grad_div applied inside (no clip where max_norm <= 0), or fused == 0: g *= that coefficient first, then AdamW without a clip.
 *   Decay on [0, n_decay); the bf16 shadow (dtype BF16) gets every element outside [sh_skip_lo, sh_skip_hi); zero_grad clears g.
 *   n_decay, n_total and the skip bounds are multiples of 4; RSYS_DEBUG_ADAMW is read at the call. */
int32_t rsys_op_rmsnorm_fwd(int32_t dtype, const float* x, const float* scale, void* y, float* rstd, int64_t rows, int32_t D,
                            const int32_t* rows_dev, const int32_t* in_rows, float* amax);
int32_t rsys_op_rmsnorm_bwd(int32_t dtype, int32_t g_f32, const void* g, const float* x, const float* scale, const float* rstd,
                            const float* resid, const int32_t* resid_slot, const int32_t* io_rows, const int32_t* rows_dev,
                            float* dx, void* dx_t, float* dscale, int64_t rows, int32_t D, float* amax, int32_t deterministic);
int32_t rsys_op_ce(int32_t dtype, void* logits, int64_t ldl, int32_t n, int32_t V, const int32_t* idx, const float* label,
                   const float* weight, const int32_t* position, const float* stats, const int32_t* npos, float task_w, float* loss,
                   int32_t deterministic);
int32_t rsys_op_rating_tail(int32_t dtype, void* z, const void* hact, int32_t n, int32_t D, const float* w2, const float* b2,
                            const int32_t* idx, const float* label, const float* weight, const float* stats, float rating_mean,
                            float task_w, int32_t evaluate, float* loss, float* dw2, float* db2, float* db0, const int32_t* npos,
                            int32_t deterministic);
int32_t rsys_op_sumsq(const float* g, int64_t n, float* out);
int32_t rsys_op_clip_adamw(int32_t dtype, float* p, float* g, float* m, float* v, void* shadow, int64_t n_decay, int64_t n_total,
                           float lr, float b1, float b2, float eps, float wd, int32_t step, float max_norm, float grad_div,
                           int32_t zero_grad, int64_t sh_skip_lo, int64_t sh_skip_hi, int32_t fused, float* sumsq);
/* the adapter bank's kernels (csrc/adapter_bank.hip), unit-test access on caller-provided device buffers: each call fills the arguments of
 * the launch routines the model path calls, runs the selected launches on the null stream and synchronises.  dtype RSYS_DTYPE_FP32 / BF16 =
 * the compute type T.  Nq = H hd, Nk = Nv = KV hd, ld = Nq + Nk + Nv.
 * rsys_op_adapter_bank: `stages` is a mask, run in this (the production) order: 1 stage A (train != 0: the training form, with the
 *   dropout mask of (p, seed, stream); stream in [0, 2^32) is the model's step * 64 + layer), 2 stage B, 4 dLa, 8 the dB partials, 16 the
 *   dA partials, 32 dx, 64 both row reductions.  A stage reads its inputs from the buffers below, so one bit runs that kernel alone on
 *   given intermediates.  Buffers (T-typed unless fp32 is said):
 *     row_slot int32 [rows] (device), values in [-1, RSYS_ADAPTER_SLOTS); a row with -1 is neither read nor written by any stage
 *     bankA [slots][L][16][D] ([A_q; A_v]), bankB [slots][L][Nq + Nv][8] (B_q rows, then B_v rows), slots >= 1 + the largest slot named
 *     xn [rows*Ttok][D]                read by 1, 16
 *     La [rows*Ttok][16]               written by 1, read by 2, 8
 *     qkv [rows*Ttok][ld]              q and v columns updated in place by 2 (k columns untouched)
 *     dqkv [rows*Ttok][ld]             read by 4, 8 (gradients w.r.t. the un-rotated q and v)
 *     dLa [rows*Ttok][16]              written by 4, read by 16, 32
 *     dxn [rows*Ttok][D]               added to by 32
 *     partA fp32 [rows][16][D]         written by 16, read by 64
 *     partB fp32 [rows][Nq + Nv][8]    written by 8 (without the factor 2), read by 64
 *     gA fp32 [slots][L][16][D], gB fp32 [slots][L][Nq + Nv][8]: layer `layer` of every slot with a row is added to by 64
 *     rope_cos / rope_sin fp32 [rope_rows][hd / 2]; rope_pos int32 [rows*Ttok] (device) or null: token t of a row has position t
 *   Buffers of stages that are not selected may be null.  RSYS_ERR_ARG before anything is launched unless Ttok % 8 == 0, D % 16 == 0,
 *   D == H hd, hd in {16, 32, 64, 128}, H % KV == 0, 0 <= layer < L, 0 <= p < 1, every row_slot value in range and (stage B) every
 *   rope_pos value in [0, rope_rows), resp. rope_rows >= Ttok without rope_pos (row_slot and rope_pos are copied back once for this).
 * rsys_op_adapter_bank_adamw: the per-slot clip + AdamW kernel, one workgroup per slot, all RSYS_ADAPTER_SLOTS slots.  fp32 masters A32 /
 *   B32, gradients gA / gB and moments mA, vA / mB, vB: [RSYS_ADAPTER_SLOTS][nA] resp. [..][nB]; A / B: the T-typed copies of the masters
 *   (bf16; null in fp32); per_slot (host) float [RSYS_ADAPTER_SLOTS][4] = (active, lr, max_norm, step) with step >= 1 the count the bias
 *   corrections are taken at (computed by the host code of rsys_adapter_adamw_step); norms (device) fp32 [RSYS_ADAPTER_SLOTS]: the slot's
 *   gradient norm, 0 for an inactive slot, of which nothing else is read or written.
 * rsys_op_dropout: the finetune model's dropout launch on src / dst T-typed [n]: dst = (accumulate ? dst : 0) + (kept ? src / (1 - p) : 0),
 *   element e kept iff u01(Philox(seed)(e >> 2, stream)[e & 3]) >= p. */
int32_t rsys_op_adapter_bank(int32_t dtype, int32_t stages, int32_t train, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd,
                             int32_t L, int32_t layer, float p, uint64_t seed, int64_t stream, const int32_t* row_slot, const void* bankA,
                             const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv, void* dLa, void* dxn, float* partA, float* partB,
                             float* gA, float* gB, const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows);
/* rsys_op_adapter_bank restricted to the forward (stages a mask of 1 and 2, train == 0) in the per-tile form of packed serving rows:
 * tile_slot int32 [rows][ceil(Ttok / 64)] (device) in place of row_slot, tokens [64 j, 64 j + 64) of row r run with slot
 * tile_slot[r][j]; a tile with -1 is neither read nor written.  Same buffers and argument checks. */
int32_t rsys_op_adapter_bank_tiles(int32_t dtype, int32_t stages, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd, int32_t L,
                                   int32_t layer, const int32_t* tile_slot, const void* bankA, const void* bankB, const void* xn, void* La, void* qkv,
                                   const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows);
/* rsys_op_adapter_bank in the forms of packed finetune rows: segs int32 [n_seg][5] (device) = (row, first interaction
 * column, columns, slot, task) in place of row_slot, on rows of Ttok / 2 interactions.  Stages 1 (train != 0: under the dropout mask), 2, 4
 * and 32 run per 64-token tile with the slot of the segment that owns the tile; 8 and 16 write one partial per segment over the segment's
 * whole tiles, partA fp32 [n_seg][16][D], partB fp32 [n_seg][Nq + Nv][8]; 64 adds, per slot, its segments' partials in descriptor order.
 * A tile no segment owns and a segment with slot -1 are neither read nor written.  The table is copied back once and checked as
 * rsys_adapter_forward_backward_packed checks it (RSYS_ERR_ARG before anything is launched); otherwise buffers and checks of
 * rsys_op_adapter_bank. */
int32_t rsys_op_adapter_bank_segments(int32_t dtype, int32_t stages, int32_t train, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd,
                                      int32_t L, int32_t layer, float p, uint64_t seed, int64_t stream, const int32_t* segs, int32_t n_seg, const void* bankA,
                                      const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv, void* dLa, void* dxn, float* partA,
                                      float* partB, float* gA, float* gB, const float* rope_cos, const float* rope_sin, const int32_t* rope_pos,
                                      int32_t rope_rows);
int32_t rsys_op_adapter_bank_adamw(int32_t dtype, float* A32, float* B32, float* gA, float* gB, float* mA, float* vA, float* mB, float* vB, void* A,
                                   void* B, int64_t nA, int64_t nB, const float* per_slot, float b1, float b2, float eps, float wd, float* norms);
int32_t rsys_op_dropout(int32_t dtype, const void* src, void* dst, int64_t n, float p, uint64_t seed, int64_t stream, int32_t accumulate);
/* the kernels of the row-sharded table (csrc/shard.hip), unit-test access on caller-provided device buffers: every stage calls the launch
 * routine the model path calls, unchanged, on the null stream; the call synchronises.  There is NO collective and NO GEMM inside: the logits
 * are an input, and what the model all-reduces between two stages (lmax -> gmax, sums, the target logit) the caller reduces on the host and
 * writes back, so "W ranks" are W calls with each rank's (Vloc or len, col0, logits block, rank).  `stages` is a mask, run in ascending bit
 * order (the production order); a stage reads its inputs from the buffers below, so one bit runs that launcher alone on given
 * intermediates; buffers of stages that are not selected may be null.  dtype RSYS_DTYPE_FP32 / BF16 = the T of the launcher (rows, logits).
 * deterministic != 0: the call runs with deterministic-mode scratch of its own and returns RSYS_ERR_STATE if a launcher that has an ordered
 * form (vp finish, ss finish, ss target_grad) did not take it.  RSYS_ERR_ARG before anything is launched where an argument is out of range;
 * index arrays that address a caller buffer are copied back once for that.
 * A row's meta is 4 floats {target id inside the medium (int bits), label * weight, gradient coefficient, 0}.
 * rsys_op_vp_ce, stages 1 meta, 2 compact, 4 stats, 8 rebase, 16 finish:
 *     meta      own f32 [KBmax * 4 + 1]: row j < KB gets {position[i], label[i] weight[i], task_w label[i] weight[i] / max(stats[0], 1e-8), 0}
 *               with i = idx[j] (idx int32 [KB]; label, weight, position indexed by it), rows [KB, KBmax) zeros, own[KBmax * 4] = *npos (int
 *               bits).  0 <= KB <= KBmax.
 *     compact   EwAll T [W][KBmax][D], metaAll f32 [W][KBmax * 4 + 4] (element KBmax * 4 of a block = its live count n_q <= KBmax, int bits):
 *               EwC T [W * KBmax][D] and metaC f32 [W * KBmax][4] get rows (q, i < n_q) packed at pre[q] + i; *nlive = sum n_q, pre int32
 *               [W + 1] the prefix.  metaC rows [nlive, min(round_up(nlive, 256), W * KBmax)) are zeroed, everything behind is untouched
 *               (so are the EwC rows from nlive on).  D a multiple of 16 bytes of T, 1 <= W <= 47.
 *     stats     logits T [>= rows][ldl], ldl % 8 == 0, Vloc <= ldl local columns, the first being class col0.  For row < rows (rows <= cap):
 *               lmax[row] = the row's maximum, sums[row] = sum exp(x - lmax), sums[cap + row] = the target's logit where col0 <= target <
 *               col0 + Vloc, else 0; rows >= *nlive and Vloc == 0 give (-3e38, 0, 0).  lmax f32 [cap], sums f32 [2 cap].  Columns
 *               [Vloc, ldl) are not interpreted.
 *     rebase    sums[row] *= exp(lmax[row] - gmax[row]) for row < rows.
 *     finish    grid of rows_finish <= cap rows (the model's min(cap, round_up(nlive, 256))).  Live rows: lse = gmax + log(sums[row]); a row
 *               in [pre[rank], pre[rank + 1]) with label weight != 0 adds (lse - sums[cap + row]) label weight to loss[0]; the row becomes
 *               coef (exp(x - lse) - [column == target - col0]) on [0, Vloc) and zeros on [Vloc, ldl).  Rows [nlive, rows_finish) are
 *               zeroed over [0, ldl); later rows are untouched.
 * rsys_op_ss (sampled soft-max), stages 1 sample, 2 targets, 4 drop_hits, 8 gather_rows_plain, 16 target_logit, 32 stats, 64 max_with_target,
 * 128 rebase, 256 finish, 512 add_rows_plain, 1024 target_grad:
 *     sample    cols int32 [n_s]: one class per stratum [floor(j len / n_s), floor((j + 1) len / n_s)) from Philox(seed)(j, stream)[0];
 *               1 <= n_s <= len, stream in [0, 2^32).
 *     targets   bitmap int32 [ceil(len / 32)] (bit b of word w = class 32 w + b) is cleared, the classes target - col0 in [0, len) of metaC rows < *nlive (< cap_rows = the
 *               grid) are marked; tlist gets them ascending, *tcount their number; tlist behind that is untouched.
 *     drop_hits cols[j] = -1 where the bitmap holds cols[j] (values in [0, len)).
 *     gather_rows_plain   gdst T [rn][D] row j = gsrc row (rbase + ridx[j]) (row stride rld), zeros where ridx[j] < 0.
 *     add_rows_plain      adst f32 row (rbase + ridx[j]) (stride rld) += asrc f32 [rn][D] row j; ridx[j] < 0 skipped; the others distinct.
 *               Both: 0 <= rbase + ridx[j] < rtable_rows.
 *     target_logit   tl[row] = <EwC row, Floc row (target - col0)> where that lies in [0, len), else 0, for row < min(rows, *nlive); EwC T
 *               [rows][D], Floc T [len][D].
 *     stats     logits T [>= rows][ldl >= n_tot]: column c < n_s belongs to sampled class cols[c] (weight s_c = its stratum's size), column
 *               n_s <= c < n_tot to an in-batch target cols[c] (weight 1).  lmax / lsum [rows] = maximum and sum-exp of x + log weight
 *               over the columns with cols[c] >= 0 and cols[c] != target - col0; rows >= *nlive and n_tot == 0 give (-3e38, 0).
 *     max_with_target   gmax[row] = max(lmax[row], tl[row]), row < rows (tl summed over the ranks by the caller).
 *     rebase    lsum[row] *= exp(lmax[row] - gmax[row]) (0 stays 0), row < rows.
 *     finish    grid of rows_finish rows.  lse = gmax + log(exp(tl - gmax) + lsum); dt[row] = coef (exp(tl - lse) - 1); the owner of the row
 *               ([pre[rank], pre[rank + 1]), label weight != 0) adds (lse - tl) label weight to loss[0]; column c becomes coef weight_c
 *               exp(x - lse), or 0 at a dropped entry, at the row's own target and on [n_tot, ldl).  Rows [nlive, rows_finish): zeros,
 *               dt = 0.  A rank without classes calls it with n_s = n_tot = 0, ldl = 8.
 *     target_grad    for row < min(rows, *nlive) with a local target t and dt[row] != 0: gE_loc f32 [len][D] row t += dt[row] EwC[row] and
 *               dEwC f32 [rows][D] row += dt[row] Floc[t]: float atomics, or (deterministic) the first row of a class adds for all rows
 *               that share it, in row order; D <= 2048 there.
 * rsys_op_shard_rows, stages 1 plan_unique, 2 plan_offsets, and at most one of 4 gather_rows_by_id, 8 add_rows_by_id, 16
 * add_rows_by_id_counted, then 32 gather_items_remote:
 *     plan_unique    skey int32 [N] ascending in [0, V] (V = the mask row), sidx [N] a permutation: slot[p] = rank of skey[p] among the distinct
 *               keys, uniq[slot] = key, tok2u[sidx[p]] = slot[p]; V gets a slot even when absent (uniq [N + 1]); plan = {U, uV}.
 *     plan_offsets   off[o] = first slot of uniq[0, plan[0]) with id >= bound[o], o < nb, 2 <= nb <= 64.
 *     gather    packed f32 [n][D] row j = table row (ids[j] - sub) (stride ld);  add: table row (ids[j] - sub) += packed row j (ids distinct);
 *               counted: table row ids[j] += packed row j for j < min(*count, n) (n is the capacity).  Ids inside [sub, sub + table_rows).
 *     gather_items_remote   x0 f32 [2 Ntok][D] row 2 t = Frem row (m_matchedid[t] == -1 ? plan[1] : tok2u[t]) (odd rows untouched), uid_t /
 *               tm_t int32 [2 Ntok] = userid[t] / m_tmid[t] twice; Frem f32 [frem_rows][D]. */
int32_t rsys_op_vp_ce(int32_t dtype, int32_t stages, int32_t deterministic, const int32_t* idx, const float* label, const float* weight,
                      const int32_t* position, const float* stats, const int32_t* npos, float task_w, int32_t KB, int32_t KBmax, float* own,
                      const void* EwAll, const float* metaAll, int32_t W, int32_t D, void* EwC, float* metaC, int32_t* nlive, int32_t* pre,
                      void* logits, int64_t ldl, int32_t Vloc, int32_t col0, float* lmax, const float* gmax, float* sums, int32_t cap,
                      int32_t rank, float* loss, int32_t rows, int32_t rows_finish);
int32_t rsys_op_ss(int32_t dtype, int32_t stages, int32_t deterministic, int32_t len, int32_t n_s, int32_t n_tot, int32_t col0, uint64_t seed,
                   int64_t stream, int32_t* cols, int32_t* bitmap, int32_t* tlist, int32_t* tcount, const float* metaC, const int32_t* nlive,
                   const int32_t* pre, int32_t rank, int32_t cap_rows, int32_t rows, int32_t rows_finish, const void* EwC, const void* Floc,
                   int32_t D, void* logits, int64_t ldl, float* lmax, float* lsum, float* tl, float* gmax, float* loss, float* dt,
                   float* gE_loc, float* dEwC, const int32_t* ridx, int32_t rbase, int64_t rld, int32_t rn, int32_t rtable_rows,
                   const void* gsrc, void* gdst, const float* asrc, float* adst);
int32_t rsys_op_shard_rows(int32_t stages, const int32_t* skey, const int32_t* sidx, int32_t N, int32_t V, int32_t* slot, int32_t* uniq,
                           int32_t* tok2u, int32_t* plan, const int32_t* bound, int32_t nb, int32_t* off, float* table, int64_t ld,
                           int32_t table_rows, const int32_t* ids, int32_t sub, float* packed, int32_t n, int32_t D, const int32_t* count,
                           const int32_t* m_matchedid, const int32_t* userid, const int32_t* m_tmid, int32_t Ntok, const float* Frem,
                           int32_t frem_rows, float* x0, int32_t* uid_t, int32_t* tm_t);
/* the index and compaction kernels (csrc/compact.hip, the position selection, row movers and column sums of csrc/elementwise.hip, the batched
 * transpose of csrc/optim.hip), unit-test access on caller-provided device buffers: every call runs the launcher the model path calls,
 * unchanged, on the null stream and synchronises.  RSYS_ERR_ARG before anything is launched where an argument is out of range; index arrays
 * that address a caller buffer are copied back once for that.  These kernels decide WHICH rows the products run on: their integer outputs
 * and the rows they move are exact, whatever the launch shape.
 * rsys_op_select_positions: per task t < ntask (1 .. 4) of w f32 [ntask][N]: idx [ntask][topk] = the positions with w > 0 in ascending
 *   order, then the others ascending, CUT AT topk (slot topk and later do not exist and are not written); npos[t] = min(#(w > 0), topk);
 *   stats [ntask][2] = (sum of w over the selected positions, sum over all).  form 0: launch_select_positions_batch (one workgroup per task),
 *   form 1: launch_select_positions_chunked (32 chunks per task, scratch allocated by the call); neither is restricted by N here (the model
 *   takes the chunked form from N >= 4096).  1 <= topk <= N <= 2^24 (the chunked form counts in fp32).
 * rsys_op_token_union: idx int32 [ntask][cap], npos int32 [ntask] (device).  bits [ceil(NT / 32)] (int32 words read as bit patterns): bit (tok & 31) of word tok >> 5 is
 *   set iff tok = 2 idx[t][r] + (t & 1) for some task t and r < npos[t]; pre [ceil(NT / 32)]: the number of set bits in the words before;
 *   *nsel their total.  Bit t of null_mask passes task t with a null list (skipped; its npos is not read).  The call checks 0 <= npos[t] <= cap
 *   and 0 <= 2 idx + 1 < NT for the live entries (both tokens of a position exist); 1 <= NT <= 2^19 is the launcher's own bound (the
 *   bitmap lives in LDS).
 * rsys_op_selected_first: bits / pre as above over the B T tokens of B rows (the call checks that pre is the exclusive prefix count of bits
 *   over those words and that the total is <= sel_cap; B T <= 2^19, T <= 4096), uid / tm int32 [B T], rope_pos int32 [B T] or null.
 *   slot [B T] = rank of the token among the selected (ascending token order) or -1; sel [sel_cap]: sel[slot[t]] = t, later entries untouched.
 *   Placement rule: inside row b the selected tokens come first in their original order, then the others in theirs; perm [B T] = the
 *   (global) token at each place, uid_p / tm_p = its ids, pos_p = its rope_pos (null: its index inside the row), slot_p = its slot,
 *   sel_p [sel_cap]: sel_p[slot_p[p]] = p.  q_active [B] = ceil(selected tokens of the row / 64).  Under RSYS_TOP_ORDER=0 (read as parsed at
 *   the call) the order is the identity (perm[p] = p) and q_active = ceil(T / 64); slot / sel are the same.
 * rsys_op_rows: the row movers; T = dtype (fp32 / bf16; kinds 4 and 6 are fp32 only), D and every ld a multiple of 16 bytes of T, ld >= D.
 *   A "token" is 2 idx[r] + parity, parity 0 / 1.  The launchers size their grid from n (kind 0: from cap): n >= 1, cap >= 1.
 *   kind 0 gather_rows_sel: dst [cap = dst_rows][D] row r < *count = src [src_rows][ld] row map[r]; rows [*count, min(cap, round_up(*count,
 *     256))) are zeros; later rows untouched.  0 <= *count <= min(cap, map_len), map values in [0, src_rows).
 *   kind 1 scatter_rows_fill: n batch rows of Tseq places, dst [n Tseq = dst_rows][ld], map = slot_p [map_len = dst_rows], count = q_active
 *     [n]: place p < min(Tseq, 64 q_active[b]) of row b = src [src_rows][D] row slot_p, or zeros where slot_p = -1; the places behind are
 *     untouched, and so are columns [D, ld).
 *   kind 2 scatter_rows_map: dst [dst_rows][ld] row map[r] = src [n][D] row r; map distinct, in [0, dst_rows); other rows untouched.
 *   kind 3 gather_rows_slot: dst [n][D] row r = src [src_rows][D] row map[token] (map = slot [map_len]), zeros where that is -1.
 *   kind 4 scatter_rows_add_slot: dst [dst_rows][D] row map[token] += src [n][D] row r for r < min(n, *count), skipped where -1.
 *   kind 5 gather_rows: dst [n][D] row r = src [src_rows][ld] row token.
 *   kind 6 scatter_rows_add: dst [dst_rows][ld] row token += src [n][D] row r for r < min(n, *count) (count null: r < n).
 *   Kinds 4 and 6 take distinct destination rows among the live r (one task at a time in the model); tokens and slots inside their arrays.
 * rsys_op_colsum: colsum [D] += column sums of src f32 [rows][ld] (1 <= rows <= 2^24).  kind 0 launch_colsum_add (D = cols, any ld >= D);
 *   kind 1 launch_cast_colsum (ld == D, D / 4 divides 1024): also dst bf16 [rows][D] = src rounded to nearest even; kind 2
 *   launch_cast_transpose_colsum (ld == D, D % 64 == 0, ldt % 8 == 0, ldt >= round_up(rows, 64)): also dst bf16 [D][ldt], dst[c][r] = src[r][c]
 *   rounded, columns [rows, round_up(rows, 64)) zeros, columns behind untouched.  deterministic != 0: per-workgroup partials added in
 *   workgroup order, scratch sized from the launcher's grid; RSYS_ERR_STATE if that branch did not run.
 * rsys_op_transpose_bf16: one launch_transpose_bf16 of n_jobs (1 .. 64) jobs given as HOST arrays: dst[j] bf16 [cols][ld_dst] = the transpose of
 *   src[j] bf16 [rows][ld_src] (device pointers, 16-byte aligned); ld_src >= cols, ld_dst >= rows, both multiples of 8 (16-byte row strides:
 *   the kernel moves 8 elements per access); the padding columns of dst are untouched. */
int32_t rsys_op_select_positions(int32_t form, int32_t ntask, const float* w, int32_t N, int32_t topk, int32_t* idx, float* stats, int32_t* npos);
int32_t rsys_op_token_union(int32_t ntask, const int32_t* idx, int32_t cap, const int32_t* npos, int32_t null_mask, int32_t NT, int32_t* bits,
                            int32_t* pre, int32_t* nsel);
int32_t rsys_op_selected_first(const int32_t* bits, const int32_t* pre, int32_t B, int32_t T, const int32_t* uid, const int32_t* tm,
                               const int32_t* rope_pos, int32_t* slot, int32_t* sel, int32_t sel_cap, int32_t* perm, int32_t* uid_p,
                               int32_t* tm_p, int32_t* pos_p, int32_t* slot_p, int32_t* sel_p, int32_t* q_active);
int32_t rsys_op_rows(int32_t kind, int32_t dtype, const void* src, int64_t src_rows, void* dst, int64_t dst_rows, int64_t ld, int32_t n, int32_t D,
                     const int32_t* map, int64_t map_len, const int32_t* idx, int32_t parity, const int32_t* count, int32_t Tseq);
int32_t rsys_op_colsum(int32_t kind, int32_t deterministic, const float* src, int64_t ld, int64_t rows, int32_t D, float* colsum, void* dst,
                       int64_t ldt);
int32_t rsys_op_transpose_bf16(int32_t n_jobs, const void* const* src, void* const* dst, const int32_t* rows, const int32_t* cols,
                               const int64_t* ld_src, const int64_t* ld_dst);

#ifdef __cplusplus
}
#endif
#endif
