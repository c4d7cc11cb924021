// Model state + step orchestration (host side of the HIP path).
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/rsys.h"
#include "../../include/rsys_debug.h"
#include "comm.hpp"
#include "gemm.hpp"
#include "kernels.hpp"
#include "workspace.hpp"

namespace rsys {

enum RowMap { MAP_DIRECT = 0, MAP_W1 = 1, MAP_W3 = 2 };

struct TensorInfo {
  std::string name;      // reference state_dict key
  int64_t rows, cols;    // external (reference) shape; 1-D tensors have rows = 1
  int ndim;
  int64_t off;           // offset (floats) of the internal block inside the flat buffers
  int64_t ld;            // internal row stride
  int map;               // RowMap
  bool trainable;
  bool frozen_table;     // metadata embedding (stored separately, T-typed)
};

struct LayerOff {  // offsets into the flat buffers
  int64_t wqkv, wo, w13, w2, sa, mlp;
  int64_t la, lb;   // finetune: LoRA A = [Aq; Av] (16 x D), B = block matrix (Nqkv x 16): q rows x cols 0-7, v rows x cols 8-15
};

struct PhaseTimer {
  bool enabled = false;
  std::vector<std::pair<std::string, hipEvent_t>> marks;
  std::map<std::string, double> acc_ms;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  // only call sites whose name contains `filter` are timed ("" = all): bench.py times the dominant kernel family alone inside its timed
  // region (two event records per site cost the step ~4 us each; all ~120 sites of a step: +7 %)
  std::string filter;
  std::vector<char> open;   // per open tic: 1 = recorded, 0 = filtered out (its toc records nothing)
};

// The text queries held for one medium (rsys_query_texts_set): per text the logits z [n][ldz] over the medium's
// items, their log-sum-exp and the weight on the device (one grow-on-demand buffer), the group on the host.
struct TextSet {
  DevScratch buf;
  int n = 0; long long ldz = 0;
  float *z = nullptr, *lse = nullptr, *d_w = nullptr;
  std::vector<int32_t> group;
};
// The texts of one request or of one inner call of a pipeline: rows `row[i]` of a TextSet's device arrays, in text order, with the group
// of the call each belongs to (host arrays; the C entry points have checked the groups against the call's, capi.hip PendingQueries, and
// the pipelines renumber them).  n == 0: none, and the call launches what it always has.
struct QueryTexts {
  int n = 0;
  const float *z = nullptr, *lse = nullptr, *d_w = nullptr; long long ldz = 0;
  const int32_t *row = nullptr, *group = nullptr;
};
// Query weights of one request (rsys_query_weights_set), host arrays: user [n_queries / n_users] and sel
// [sel.off[n_groups]], each null when that kind is unweighted -- the request then launches the unweighted kernels.  The C entry points
// take them from the model's pending pair (capi.hip PendingQueries) and have checked the counts; inner calls pass their slices.
struct QueryWeights { const float* user = nullptr; const float* sel = nullptr; };
// The ragged lists of a request, host arrays with offsets [rows + 1]: the list items of every user and the selected items of every
// group.  All null: the request has no such list.
struct HistoryList { const int64_t* off = nullptr; const int32_t *medium = nullptr, *ids = nullptr, *status = nullptr; };
struct SelectedList { const int64_t* off = nullptr; const int32_t *medium = nullptr, *ids = nullptr; };
// What a serving request is handed, the same value on every path (retrieval, ranking, the stages of a page): nq users -- their queries
// [nq][D] on the host, or null where the call reads them from the device (RetrieveDev, RankDev) or scores none --, the group of each
// (null: user u is group u) out of ng, the two lists, the weights and the text queries.
struct Request {
  const float* queries = nullptr; int64_t nq = 0; const int32_t* group = nullptr; int32_t ng = 0;
  HistoryList hist; SelectedList sel;
  QueryWeights qw; QueryTexts qt;
};
// per group of a call the texts' rows in text order (members) and their range in it (ranges: 2 ints per group), as GroupPlan lays users out
inline void text_plan(const QueryTexts& qt, int ng, std::vector<int32_t>& members, std::vector<int32_t>& ranges) {
  members.clear(); ranges.assign((size_t)2 * ng, 0);
  for (int g = 0; g < ng; ++g) {
    ranges[2 * g] = (int32_t)members.size();
    for (int i = 0; i < qt.n; ++i) if (qt.group[i] == g) members.push_back(qt.row[i]);
    ranges[2 * g + 1] = (int32_t)members.size();
  }
}

struct RetrievalTables;  // retrieve_request.hip
struct RankTables;       // rank_request.hip
struct AdapterBank;      // adapter_bank.hip
struct RenderState;      // render_request.hip

// A batch as the device holds it, the only description of one outside the kernels (model_batch.hip): bd's input arrays point into a
// slot's blob; bd.watch_mask / rating_mask / rope_pos are set when the batch has them and null when not; the mask_tokens outputs are the
// model's own.  rows of row_len interactions (row_len < max_sequence_length: a trimmed, inference-only batch); distinct_ids: the
// distinct matchedid values + 1 (the mask row), an upper bound of the split table reduce's token-row list (0: not counted).
struct ResidentBatch { BatchDev bd{}; int rows = 0, row_len = 0, distinct_ids = 0; };
struct BatchLimits { int rows_max, Sa, Ta, V, V0, V1, vocab_status, vocab_gender, vocab_source; };   // what a host batch is checked against
// Where the arrays of a batch of N interactions sit in a slot's blob and staging buffer, back to back at 64-byte steps: the one layout
// of uploaded and device-assembled (model_batch_device_begin) batches.
struct BlobLayout { size_t time, userid, tmid, gender, source, matchedid, status, rating, progress, label[6], weight[6], position[6], wm, rm, rope, bytes; };
BlobLayout blob_layout(size_t N);
// Host only, no Model and no HIP call.  batch_check: columns [0, row_len) of every row of b (row stride lim.Sa) against the limits;
// row_len == lim.Sa is the ordinary upload (targets and masks too), a shorter one the trimmed form (neither, and userid 0 from column
// row_len on).  id_seen (null: not counted): scratch bitmap of the table's rows for *distinct_ids; nothing else is written.
// batch_pack: those columns of a checked batch into `stage` at layout L = blob_layout(rows * row_len).
int batch_check(const BatchLimits& lim, const rsys_batch* b, int row_len, std::vector<unsigned long long>* id_seen, int* distinct_ids);
void batch_pack(const BatchLimits& lim, const rsys_batch* b, int row_len, const BlobLayout& L, unsigned char* stage);

struct Model {
  rsys_config cfg;
  int device = 0;
  hipStream_t stream = nullptr;
  // DDP-style early gradient reduction (train.py:678-682): when set, the trunk backward hands every finished bucket of
  // per-layer weight gradients [lo, hi) of the flat buffer to this hook (>= 25 MB each, reverse layer order); the hook
  // enqueues its all-reduce on the communicator's stream behind an event and records the range in `reduced`
  std::function<int(int64_t, int64_t)> grad_bucket_hook;
  std::vector<std::pair<int64_t, int64_t>> reduced;
  // Split reduce of the replicated item table's gradient (opt-in, rsys_model_set_split_table_reduce): the head part of dF
  // (complete when heads() returns) is all-reduced OUT OF PLACE into tbl_R while the trunk backward runs and G[E] goes on
  // accumulating the local gradient; the token scatter of that backward goes to a compact list (tok_T rows, u_ids ids, u_plan = {U, uV})
  // and is added to G[E] from there; in the tail only the ranks' lists travel (all-gather), and G[E] = tbl_R + every rank's rows.
  bool split_table = false;          // buffers allocated, the hook may be armed
  bool split_head_reduced = false;   // this backward: the head part is on its way, the token scatter goes through tok_T
  bool split_plan_valid = false;     // u_slot / u_ids / u_plan describe the resident batch (replicated table)
  std::function<int()> table_head_hook;
  hipEvent_t split_head_event = nullptr;   // recorded behind the head part's all-reduce (which reads G[E]); the token-row add into G[E] waits for it
  float *tbl_R = nullptr, *tok_T = nullptr, *tok_Tall = nullptr;
  int *tok_Uall = nullptr, *tok_Pall = nullptr;
  int64_t tok_cap = 0;               // rows of tok_T and ids of u_ids: rows_max * S + 1
  // The tail gathers max_r U_r rows per rank instead of tok_cap (round 6).  A rank knows an upper bound of its own U on the HOST as soon
  // as the batch is staged (distinct matchedid values + the mask row: u_bound_host, counted by batch_check); when the reduce is armed
  // (rsys_set_grad_sync) the bounds' maximum over the ranks is formed by a one-float all-reduce at the head of the communicator's stream
  // and copied to pinned memory (h_umax[1], event ev_umax): by the time the tail is enqueued it has been there for a whole backward.
  int u_bound_host = 0;
  std::vector<unsigned long long> id_seen;   // batch_check's bitmap of table rows
  float* h_umax = nullptr; float* d_umax = nullptr; hipEvent_t ev_umax = nullptr; bool umax_pending = false;
  int64_t tok_all_rows = 0;          // rows per rank tok_Tall / tok_Uall are sized for
  int tok_all_world = 0;             // ranks tok_Tall / tok_Uall / tok_Pall are sized for
  int gemm_flags = 0;          // OR-ed into GemmParams.flags: GEMM_ONE_WG_PER_TILE while all-reduce kernels may share the CUs with the backward
  int64_t early_reduced = 0;   // elements the last rsys_allreduce_grads found already reduced (tests)
  // what the last optimizer step's gradient reduction enqueued, in order: {first element, one past the last, phase}; phase 0 = early bucket
  // (from inside the backward), 1 = tail beside the dWp GEMM, 2 = dWp itself, 3 = split table reduce: head part out of place (under the
  // trunk backward), 4 = split table reduce: the ranks' token rows (all-gather; elements = gathered floats).  rsys_grad_sync_schedule reads it.
  struct BucketLog { int64_t lo, hi; int phase; };
  std::vector<BucketLog> bucket_log;
  int bucket_phase = 0;
  bool bf16_mode = false;
  size_t esz = 4;
  // dims
  int L, H, KV, D, I, Ip, S, T, V0, V1, V, M, Mp, K, hd, Nqkv, rows_max;
  // S / T above are the RESIDENT BATCH's row length (interactions / tokens): everything that walks the batch reads them.  Sa / Ta are the
  // allocated geometry (cfg.max_sequence_length, twice that): buffer sizes, the RoPE tables,
  // the ranking cache's slot stride, the render pipelines' chunking.  S == Sa except under rsys_batch_upload_trimmed and the trimmed
  // forwards of the render pipelines; every ordinary upload, swap and device-assembled batch sets S = Sa.
  int Sa = 0, Ta = 0;
  bool serving_pack = false;      // rsys_serving_pack_set: the retrieval stage of the two render entry points packs several users into a row
  bool serving_pack_ranking = false;   // rsys_serving_pack_ranking_set: rsys_render_request_full packs its K/V-cache store rows
  bool serving_trim = false;      // rsys_serving_trim_set: the two render entry points run every forward at its longest live row
  int64_t fwd_tokens = 0;         // tokens the last forward_trunk ran over (rsys_debug_get "forward.tokens")
  int64_t n_decay = 0, n_total = 0;
  int64_t n_opt = 0, n_opt_decay = 0;   // range the optimizer / clip / all-reduce cover (finetune: the LoRA segment only)
  std::vector<TensorInfo> tensors;
  std::map<std::string, int> by_name;
  // flat offsets
  int64_t o_status, o_gender, o_source, o_lin_w, o_E, o_Wp, o_r0w, o_r2w;
  int64_t o_pcos, o_psin, o_lin_b, o_bp, o_norm, o_r0b, o_r2b;
  std::vector<LayerOff> lo;
  // device memory
  float *P = nullptr, *G = nullptr;
  void* Sh = nullptr;        // bf16 shadow of P (bf16 mode); == P in fp32 mode
  void* ShT = nullptr;       // bf16 mode: the trunk weight matrices of Sh, transposed ([in][out]), same offsets: the dx GEMMs then
                             // read row-major operands (256x256 LDS-DMA kernel); rebuilt lazily when wt_dirty
  bool wt_dirty = true;
  // fp8 trunk (cfg.dtype == RSYS_DTYPE_FP8; f8.hip): bf16 arithmetic everywhere except the transformer blocks' linears, whose
  // forward and dx products take tensor-wise scaled e4m3 / e5m2 operands (the reference's torchao recipe, transformer.py:671-676)
  bool fp8 = false;
  int64_t w8_base = 0;            // element offset of the first trunk weight: W8 / W8T hold [w8_base, end of the last layer's W2)
  unsigned char* W8 = nullptr;    // e4m3 copies of the trunk's linear weights, row-major [out][in]: forward B operands
  unsigned char* W8T = nullptr;   // transposed copies [in][out] (W13: K order [all w1 | all w3]): dx B operands
  float* f8_wamax = nullptr;      // [L][8]: amax of q k v o w1 w3 w2 (this step's weights)
  float* f8_aamax = nullptr;      // [L][64 shards][32]: sharded amax slots (common.hpp f8_amax_note) of xn O hn g | dy2 da db dh dq dk dv (this pass)
  float* f8_desc = nullptr;       // [L][8 products][32]: descales the casts write for their consumer GEMMs (GemmParams::f8_desc)
  unsigned char* a8 = nullptr;    // fp8 copy of the current product's A operand
  void* f8_jobs = nullptr; int* f8_tile_job = nullptr; int* f8_tile_first = nullptr; int f8_ntiles = 0;
  bool w8_dirty = true;
  void* sel_scratch = nullptr;    // chunk counts / sums of the multi-workgroup position selection
  float* rope_cs = nullptr;       // [T][hd/2][2]: (cos, sin) interleaved copy of the RoPE tables for the QKV epilogue
  // fp8 weight gradients dW = q_e5m2(dY)^T . q_e4m3(X): every cast also leaves a K-contiguous (transposed, [features][tokens]) copy
  // per layer, consumed by the split-K fp8 form after (or, grouped, at the end of) the backward.  RSYS_F8_DW=0: bf16 operands instead.
  bool f8_dw = false;
  bool f8_tcopies = true;         // this pass is followed by a backward (forward-only passes skip the transposed copies)
  struct F8T { unsigned char *xn, *O, *hn, *g, *gxt, *dab, *dht, *dqkv; };
  std::vector<F8T> f8t;
  float* f8_desc_dw = nullptr;    // [L][4 products: w2 w13 o qkv][32]: row descales of the weight-gradient products
  int64_t f8_ldt = 0;             // row stride of the transposed copies (tokens of a full batch)
  // RSYS_F8_DW_ROUND_BF16=1: every fp8 weight-gradient product is summed (fp32, all its split-K parts) into dw_stage, rounded to
  // bf16 once and only then added to the fp32 gradient -- what autograd does under autocast, where the product's output tensor is
  // bf16 and param.grad is fp32.  Default: the fp32 sum goes to the gradient unrounded.
  float* f8_dw_stage = nullptr;   // [trunk weights of all layers], zero between products
  int64_t f8_dw_stage_base = 0;   // offset (in the flat buffers) of its first element
  std::vector<void*> f8_keep;     // RSYS_F8_DEBUG_KEEP=1 (tests): per layer, copies of the three dx products' outputs (w13_dx, o_dx, qkv_dx)
  bool table_dirty = true;     // the fused item table F / FT must be rebuilt before the next forward: set by everything that changes a
                               // parameter or the metadata, and by the table-gradient pass (it borrows FT); clean between the
                               // micro-steps of one optimizer step, across finetune steps (frozen table) and across inference calls
  void* Meta = nullptr;      // [V+1][Mp] T
  float* F32 = nullptr;      // [V+1][D]
  void* FT = nullptr;        // [V+1][D] T
  // bf16 mode: K-contiguous (transposed) operand copies for the metadata-projection gradient dWp = dF^T Meta, which then
  // runs on the row-major LDS-DMA pipeline: MetaT [Mp][Vp] (built when the table is loaded), dFT [D][Vp] (per step);
  // Vp = V + 1 rounded up to 64, the padding stays zero
  void* MetaT = nullptr; void* dFT = nullptr; int64_t Vp = 0;
  // ---- row-sharded item table (cfg-4, shard.hip): this rank holds table rows [row_lo, row_lo + TR) of E / Meta / F
  bool sharded = false; int sh_rank = 0, sh_world = 1;
  int row_lo = 0, TR = 0;                // TR = V + 1 when the table is replicated
  rsys_comm* shard_comm = nullptr;
  // exchange plan of the resident batch: distinct ids (sorted) and who owns / asks for them
  int *u_slot = nullptr, *u_ids = nullptr, *u_tok = nullptr, *u_plan = nullptr /*{U, uV}*/, *u_bound = nullptr, *u_off = nullptr;
  int U = 0, uV = 0;
  std::vector<long long> need_off, serve_off, need_offD, serve_offD;   // per-rank element offsets (ids; rows of D floats)
  int* req_ids = nullptr; long long req_cap = 0, R = 0;                  // ids the peers ask this rank for, by requester
  float *Frem = nullptr; float* rows_xchg = nullptr; long long xchg_cap = 0;   // [U][D] fetched rows / gradient sums; [R][D] served rows / received gradients
  // vocabulary-parallel head workspaces: gathered selected rows of all ranks, packed live rows, row statistics
  void *EwAll = nullptr, *EwC = nullptr; float *metaOwn = nullptr, *metaAll = nullptr, *metaC = nullptr, *vp_max = nullptr, *vp_lmax = nullptr, *vp_sums = nullptr;
  int *vp_nlive = nullptr, *vp_pre = nullptr; float* dEwC = nullptr;
  // The sizes of the vocabulary-parallel heads' collectives (live rows per rank, in-batch targets of the sampled soft-max) depend on the
  // masked batch only, so they are computed and copied to pinned host memory BEFORE the trunk forward (sharded_counts_early); the
  // heads wait for an event that is a whole trunk forward old instead of draining the stream once per task.
  float* metaAllT[2] = {nullptr, nullptr};   // the gathered row meta of the two watch tasks (kept from the early pass)
  int* h_counts = nullptr;                   // pinned: [2][64] = per watch task pre[0 .. W] and, at [48], the number of in-batch targets
  hipEvent_t ev_counts = nullptr; bool counts_pending = false;
  int host_stream_syncs = 0, host_event_waits = 0;   // blocking host waits inside the last rsys_forward_backward (tests)
  int64_t ldl_loc = 0; float* sumsq_E = nullptr;
  // sampled softmax: sampled local classes, their rows of F, the rows' gradients, target logits and their gradients
  int* ss_cols = nullptr; void* ss_F = nullptr; float *ss_dF = nullptr, *ss_tl = nullptr, *ss_dt = nullptr;
  unsigned int* ss_bitmap = nullptr; int* ss_tcount = nullptr;   // in-batch targets: bitmap over the local classes of a medium, their number
  unsigned long long cur_seed = 0, cur_step = 0;
  float *rope_cos = nullptr, *rope_sin = nullptr;
  int rope_npos = 0;
  std::vector<void*> allocs;
  // batch (model_batch.hip).  One upload = one copy: the batch's arrays are packed back to back (for the rows it has) in a slot's
  // pinned staging buffer and land in the slot's blob with a single H2D; the ResidentBatch describes where.  Two (staging, blob) slots:
  // rsys_batch_prefetch checks, packs and copies the NEXT batch into the other slot on its own stream while the current step still runs
  // (the reference's DataLoader + non_blocking to_device overlap, train.py:162-165,178-184); rsys_batch_swap makes it the resident batch.
  ResidentBatch resident, pending;   // resident: written by batch_install only; pending: the prefetched batch while pending_valid
  bool pending_valid = false;
  int cur_rows = 0;                  // resident.rows once the batch's copy has landed, 0 without a resident batch
  unsigned char* slot_blob[2] = {nullptr, nullptr}; unsigned char* slot_stage[2] = {nullptr, nullptr}; size_t raw_bytes = 0;   // raw_bytes: of each
  int cur_slot = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t ev_copy_done = nullptr;     // the pending batch's H2D copy (copy_stream)
  hipEvent_t ev_blob_free[2] = {nullptr, nullptr};   // recorded on `stream` when slot i stops being the resident batch: its kernels are all enqueued before
  bool blob_free_valid[2] = {false, false};
  void* batch_blob = nullptr;        // the mask_tokens outputs (resident.bd.m_*), the model's own whatever batch is resident
  bool tok_index_valid = false;      // the token index of the resident batch (scatter / exchange plan) has been built
  // deterministic mode (rsys_model_set_deterministic): every float sum of the step has a fixed order -- split-K partial tiles go
  // to det_slab and are added in split order, the reduction kernels write per-workgroup partials to det_part (kernels.hpp
  // DetScratch) -- so a step is bitwise reproducible (replicated or row-sharded table, full or sampled soft-max)
  bool deterministic = false;
  float* det_slab = nullptr; long long det_slab_floats = 0;
  float* det_part = nullptr; long long det_part_floats = 0;
  float* det_tmp = nullptr; long long det_tmp_floats = 0;
  // token index of the resident batch (scatter.hip): sorted (item id, token) pairs + the partial-sum slab of the scatter
  unsigned long long* tok_keys = nullptr; int *tok_skey = nullptr, *tok_sidx = nullptr; float* scatter_slab = nullptr;
  // activations (void* = T-typed)
  void* feat; float* x0; int *uid_t, *tm_t;
  AttnMaps maps, maps_p;   // the attention tile maps of the token order and of the selected-first order (below)
  struct LayerAct { float* x; void* xn; void* xnd; void* La; void* qkv; void* O; float* lse; float* rstd1; float* h; void* hn; float* rstd2; void* ab; void* g; };
  std::vector<LayerAct> la;
  float* xL; float* rstdf; void* out;
  // heads
  // losses of finished steps parked on the device (rsys_losses_push / _drain): the loop's per-step read-back -- its only host
  // synchronisation -- becomes one read every `loss_ring_cap` steps; slot = [16 loss sums | 8 stats] of a step
  float* loss_ring = nullptr; int loss_ring_n = 0; static constexpr int loss_ring_cap = 1024;
  int* idx[4]; int* npos; float* stats; void* Ew; void* logits; int64_t ldl; float* dE; void* z; void* hact; float* loss_acc;
  // backward workspaces
  float *gy, *gxa, *gxb, *dh; void *gxa_t, *gxb_t, *dh_t;   // *_t: T-typed operand copies (bf16 mode)
  void *dab, *dhn, *dO, *dqkv; float* delta; float* gf;
  void *dLa, *dxl;   // finetune workspaces
  float* sumsq; float* sumsq_part;   // the gradient norm's scalar and the per-workgroup partial sums of its fixed-order reduction
  // Deferred, grouped weight gradients (bf16 pretraining, products too small for the chip one at a time): the backward keeps
  // every layer's dY operands (gradient of the layer's output, of the SwiGLU pre-activations, of the attention residual, of
  // q/k/v) in per-layer buffers and ONE grouped launch (per gradient bucket when buckets are reduced early) computes the four
  // products of all those layers (gemm8p.hip: gemm8p_group_kernel).  Plans are cached per (first layer, last layer, rows).
  bool defer_dw = false;
  struct DwOperands { void *gxt, *dab, *dht, *dqkv; };
  std::vector<DwOperands> dwb;
  std::map<long long, GemmGroupPlan*> dw_plans;
  // Compact top of the trunk (compact.hip).  A training pass reads the trunk's output only at the positions the heads select, and
  // everything after the last layer's attention is token-local: the last layer's output projection, MLP and the final norm run --
  // forward and backward -- on the sorted set of selected tokens c_sel[0 .. *c_n) (c_slot: token -> row of the compact buffers
  // or -1).  Rows no head reads are not computed; backward rows whose gradient is identically zero are not multiplied.
  bool sparse_top = false;        // this model uses it for its training passes (pretraining, replicated table)
  bool top_is_sparse = false;     // the resident forward ran the compact tail: la[L-1].{h,hn,ab,g}, xL and out are NOT materialised
  int ctop_cap = 0;               // rows of the compact buffers: min(tokens, 4 * mask_topk * rows) rounded up to 256
  int *c_sel = nullptr, *c_slot = nullptr, *c_n = nullptr;
  unsigned int* c_bits = nullptr; int* c_pre = nullptr;   // bitmap of the selected tokens and the selected count before each of its words
  float *c_x = nullptr, *c_h = nullptr, *c_xL = nullptr, *c_rstd2 = nullptr, *c_rstdf = nullptr;
  void *c_O = nullptr, *c_hn = nullptr, *c_ab = nullptr, *c_g = nullptr, *c_out = nullptr;
  float *c_gy = nullptr, *c_gx = nullptr, *c_dh = nullptr;
  bool loss_acc_with_c_gy = false;   // loss_acc = the 256-byte header of c_gy's allocation (one zero fill for both)
  void *c_gx_t = nullptr, *c_dab = nullptr, *c_dhn = nullptr, *c_dh_t = nullptr, *c_dO = nullptr;
  // ... and the last layer runs on a SELECTED-FIRST token order (inside every batch row the selected tokens, then the others; attention
  // is indifferent to token order): its attention kernels then visit only the leading query tiles c_qact[b] of a row.  c_perm: original
  // token of a permuted place; uid_p / tm_p / pos_p: ids and RoPE position per permuted place; c_slot_p / c_sel_p: the compact maps in
  // permuted places; maps_p: the attention tile maps of that order.  la[L-1].{xn, rstd1, qkv, O, lse} are stored in permuted order.
  int *c_perm = nullptr, *uid_p = nullptr, *tm_p = nullptr, *pos_p = nullptr, *c_slot_p = nullptr, *c_sel_p = nullptr, *c_qact = nullptr;
  bool table_grads_pending = false;
  // the item-table gradient rows of medium m are known to be zero (just zeroed by zero_grad / AdamW and not written since):
  // the first head GEMM of a step then stores dF instead of reading 245 MB of zeros to add to
  bool gE_clean[2] = {false, false};
  bool drop_active = false; unsigned long long drop_seed = 0, drop_step = 0;   // LoRA dropout of the current pass
  bool last_evaluate = false;
  PhaseTimer timer;
  std::vector<hipEvent_t> step_marks;   // rsys_step_mark: one event per optimizer-step boundary (per-step time distribution)
  DevScratch rws;                       // rsys_retrieve_topk's workspace; a RetrieveDev result lives in it until the next retrieval call
  RetrievalTables* rtab = nullptr;      // rsys_retrieve_request's serving tables and workspace (not part of checkpoints)
  RankTables* rank = nullptr;           // rsys_rank_request's "{m}.related" tables and workspace (not part of checkpoints)
  // rsys_query_weights_set: the weights the next request entry point consumes (host copies; have_*: that kind was given)
  std::vector<float> qw_user, qw_sel;
  bool qw_have_user = false, qw_have_sel = false;
  TextSet qtexts[2];                    // rsys_query_texts_set: the text queries the next request entry point consumes, per medium
  DevScratch ews;                       // rsys_retrieve_target_rank's workspace
  // adapter bank of a base model (adapter_bank.hip, allocated by the first rsys_adapter_set): LoRA adapter sets in slots beside the frozen
  // trunk.  bank_rows (device, one slot or -1 per batch row) is non-null only inside rsys_infer_select_adapters: forward_trunk then adds
  // every row's own update to q and v; every other pass leaves it null and launches what it always has
  AdapterBank* bank = nullptr;
  const int* bank_rows = nullptr;
  const int* bank_tiles = nullptr;      // packed rows: one slot or -1 per 64-token tile, [rows][ceil(T / 64)]; non-null only inside rsys_infer_select_tiles and the packed cache calls (4zd)
  // training through the bank: true only inside rsys_adapter_forward_backward.  The pass then treats the trunk as frozen
  // (the `ft` paths of the forward, heads and backward: dx chain only), keeps La per layer, draws the LoRA dropout inside the bank's
  // kernels and sends the few small gradients those paths still write (norm gains, rating-head biases) to bank_sink, never to G
  bool bank_train = false;
  // training on packed rows: true only inside rsys_adapter_forward_backward_packed.  The pass's masks take their task per 64-token
  // tile (the task vector handed to model_forward_backward_rows is the tile map), the bank's backward runs per tile / segment, and the last
  // layer runs dense (top_is_sparse stays false: its selected-first order would put tokens of several segments into one work item)
  bool bank_packed = false;
  float* bank_sink = nullptr;   // [max(D, 64)] floats nobody reads
  RenderState* render = nullptr;        // rsys_render_request's workspace, forward counters and kept intermediates (allocated on first use)
  // ranking cache (rank_cache.hip, rsys_rank_cache_*): the post-RoPE K | V of users' history tokens per layer, [L][rc_slots][T][2 KV hd] in
  // the compute dtype, and the events held per slot (-1: never stored).  rc_mode is non-zero only inside the two cache calls: 1 = store
  // (forward_trunk copies every layer's K | V of the resident history rows into their slots), 2 = candidates (the resident rows are
  // candidate rows: no tile maps, attention through launch_attn_cand); rc_rows = the rows' {slot, n_hist, n_cand} on the device.  Every
  // other pass finds rc_mode == 0 and launches what it always has.  Not part of checkpoints.
  void* rcache = nullptr; int rc_slots = 0; std::vector<int> rc_nhist;
  int* rc_rows = nullptr;               // [3][rows_max]
  int rc_mode = 0;
  // packed rows: rc_nseg is non-zero only inside rsys_rank_cache_store_packed / _candidates_packed, whose store copy then runs per
  // segment descriptor and whose candidate attention per tile.  rc_seg (device, sized at reserve for max_rows x ceil(S / 32) segments): the
  // segment table [max_seg][4] -- store: (row, first column, n_hist, slot); candidates: (slot, n_hist, first tile, n_cand) -- and behind it
  // the candidate rows' tile -> segment map [rows][ceil(T / 64)] (-1: a dead tile)
  int* rc_seg = nullptr;
  int rc_nseg = 0;
  // Serving compact top (rsys_serving_compact_top_set; inference passes only, token order kept).  With the switch on, a pass
  // with a selection runs the last layer's tail and the final norm on the selected rows (the compact buffers above, rows in the order of the
  // selection: infer_rows_t reads c_out directly) and a store pass (rc_mode == 1) ends after its last K | V copy.  top_sel / top_nsel: the
  // selection of the pass under way, set by infer_rows_t around infer_trunk (null: none).  infer_top: what the last inference pass did --
  // 0 dense, 1 compact tail behind the dense attention, 2 compact tail behind attn_sel_kernel, 3 store stopped at K | V -- and
  // infer_top_rows the rows its tail ran on.  out_pending: xL / out of the resident forward are NOT materialised (separate from
  // top_is_sparse, the permuted training form); out_attn_pending: nor is la[L-1].O.  model_materialise_trunk_output runs the rest in
  // token order; the next forward_backward or infer_trunk clears both.
  int serving_compact_top = 0;   // 0 off, 1 on; 2 / 3 (measurement only): on, with c_O always gathered from the dense attention / always from attn_sel_kernel
  bool top_serving = false;   // the pass under way is an inference pass of a model with the compact buffers, under the switch (infer_trunk)
  const int* top_sel = nullptr; int top_nsel = 0;
  int infer_top = 0, infer_top_rows = 0;
  std::vector<int32_t>* top_log = nullptr;   // non-null inside a render call: every inference pass appends (infer_top, infer_top_rows)
  bool out_pending = false, out_attn_pending = false;
};

struct Optimizer {
  Model* m;
  int device = 0;   // (kept here: the optimizer may be destroyed after its model)
  float lr, b1, b2, eps, wd;
  int step = 0;
  float *mom = nullptr, *var = nullptr;
  // ZeRO-1 (optimizer_set_zero1): this rank keeps moments for, and updates, only its chunk [z_rank * z_chunk, + z_chunk) of the flat
  // optimized range (the last rank also the < 64 * world elements behind the last chunk); mom / var hold z_chunk + z_tail floats
  bool zero1 = false;
  int z_rank = 0, z_world = 1;
  long long z_chunk = 0, z_tail = 0;
  float* z_tailbuf = nullptr;
};
int optimizer_set_zero1(Optimizer* o, int rank, int world);
int optimizer_step_zero1(Optimizer* o, struct rsys_comm* c, float lr_factor, float clip, float grad_div);

int model_create(const rsys_config* cfg, int device, Model** out);
int model_destroy(Model* m);
int model_init_random(Model* m, uint64_t seed);
int model_load_metadata(Model* m, const float* table, int64_t V, int64_t Mdim);
int model_random_metadata(Model* m, uint64_t seed);
int model_set_rope(Model* m, const float* c, const float* s, int64_t n_pos);
int model_param_io(Model* m, const char* name, float* out, const float* in, int64_t n, int which /*0 P,1 G*/);
int model_refresh_shadow(Model* m);
int model_batch_upload(Model* m, const rsys_batch* b);
// rsys_batch_upload_trimmed: b's arrays keep the row stride Sa, columns [0, row_len) of every row become the resident batch (inference-only)
int model_batch_upload_trimmed(Model* m, const rsys_batch* b, int row_len);
int check_not_trimmed(const Model* m);   // RSYS_ERR_STATE on a trimmed resident batch (the passes that read targets)
int model_forward_backward(Model* m, int evaluate, const float task_w[4], float grad_scale, uint64_t seed, uint64_t step);
int model_infer(Model* m, int task, const int32_t* token_index, int64_t n_tokens, float* out, int64_t n);   // token_index == nullptr: every token
// adapter bank (adapter_bank.hip): slot storage by state-dict name, and the inference forward with one slot per batch row
int adapter_io(Model* m, int slot, const char* name, float* out, const float* in, int64_t n);   // exactly one of out / in
int adapter_clear(Model* m, int slot);
int adapter_slots(Model* m, int32_t* mask_out);
int adapter_bind_rows(Model* m, const int32_t* row_adapter);
int adapter_bind_tiles(Model* m, const int32_t* tile_adapter);   // [rows][ceil(Sa / 32)], the caller's geometry
void adapter_unbind_rows(Model* m);                              // ends either binding
void adapter_bank_free(Model* m);
template <typename T> int adapter_bank_stage_a(Model* m, int l, const T* xn);                      // La = xn . [A_q; A_v][slot]^T
template <typename T> int adapter_bank_stage_b(Model* m, int l, T* qkv, const int* rope_pos);      // q, v += 2 La . B[slot]^T (q rotated)
// training through the bank (adapter_bank.hip)
inline void set_row_len(Model* m, int row_len) { m->S = row_len; m->T = 2 * row_len; }
inline bool batch_trimmed(const Model* m) { return m->S != m->Sa; }
inline bool trunk_frozen(const Model* m) { return m->cfg.finetune != 0 || m->bank_train; }
inline float* small_grad(Model* m, int64_t off) { return m->bank_train ? m->bank_sink : m->G + off; }   // where a frozen-trunk pass may drop a <= D-float gradient
int adapter_train_enable(Model* m, float dropout);
int adapter_forward_backward(Model* m, int evaluate, const int32_t* row_slot, const int32_t* row_task, float grad_scale, uint64_t seed, uint64_t step);
int adapter_forward_backward_packed(Model* m, int evaluate, const int32_t* seg, int n_seg, float grad_scale, uint64_t seed, uint64_t step);   // packed rows
int adapter_grad_get(Model* m, int slot, const char* name, float* out, int64_t n);
int adapter_zero_grad(Model* m);
int adapter_adamw_step(Model* m, float lr0, float b1, float b2, float eps, float wd, const float* per_slot, int n_slots, float* norms_out);
int adapter_adamw_state_io(Model* m, int slot, const char* name, float* m_out, float* v_out, const float* m_in, const float* v_in, int64_t n, int32_t* step_out, int32_t step_in);
// per layer of the backward, after the attention backward: dxn (dhn, this layer's token order) += drop'(dLa . [A_q; A_v][slot]) and the slots' dA / dB
template <typename T> int adapter_bank_backward(Model* m, int l, const T* xn, const T* dqkv, T* dxn);
// the bank's launches on caller-provided device buffers (rsys_op_adapter_bank / rsys_op_adapter_bank_adamw, rsys_debug.h)
int adapter_bank_op(int dtype, int stages, int train, int rows, int Ttok, int D, int H, int KV, int hd, int L, int layer, float p, uint64_t seed,
                    int64_t stream, const int32_t* row_slot, const void* bankA, const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv,
                    void* dLa, void* dxn, float* partA, float* partB, float* gA, float* gB, const float* rope_cos, const float* rope_sin,
                    const int32_t* rope_pos, int rope_rows, int tiles = 0 /* 1: row_slot is a tile map (rsys_op_adapter_bank_tiles); 2: a segment table */,
                    int n_seg = 0 /* tiles == 2: its length (rsys_op_adapter_bank_segments) */);
int adapter_bank_adamw_op(int dtype, float* A32, float* B32, float* gA, float* gB, float* mA, float* vA, float* mB, float* vB, void* A, void* B,
                          int64_t nA, int64_t nB, const float* per_slot, float b1, float b2, float eps, float wd, float* norms);
// the joint pass's body (model.hip): masks per row task (d_row_task: device, [rows]), forward, heads with every task at grad_scale, backward
int model_forward_backward_rows(Model* m, int evaluate, const int* d_row_task, float grad_scale, uint64_t seed, uint64_t step);
int model_infer_adapters(Model* m, int task, const int32_t* row_adapter, const int32_t* token_index, int64_t n_tokens, float* out, int64_t n);
int model_infer_tiles(Model* m, int task, const int32_t* tile_adapter, const int32_t* token_index, int64_t n_tokens, float* out, int64_t n);
// A batch whose arrays a kernel fills on the device (render_request.hip): makes `rows` rows the resident batch without a host copy and
// returns where its arrays live in the current slot's blob (target arrays stay as they are: an inference forward never reads them).
// rope_pos holds the per-token positions (2 p, 2 p + 1 for interaction position p), as rsys_batch_upload derives them.
struct BatchDevRows { double* time; int *userid, *tmid, *gender, *source, *matchedid, *status; float *rating, *progress; int* rope_pos; };
int model_batch_device_begin(Model* m, int rows, BatchDevRows* out, int row_len = 0 /* 0: the allocated length */);
// the forward of rsys_infer_select_adapters over the resident batch with the selection (n_sel flat token indices) and the result
// (task 0: n_sel x D trunk rows, task 1: n_sel rating-head values, fp32) both on the device; row_adapter (host) may be null (base model);
// stream-ordered, no host wait
// tile_adapter (host, [rows][ceil(Sa / 32)], instead of row_adapter): packed rows, one slot per 64-token tile (adapter_bind_tiles)
int model_infer_device(Model* m, int task, const int32_t* row_adapter, const int* d_sel, int n_sel, float* d_out, const int32_t* tile_adapter = nullptr);
// rank_cache.hip: full-length ranking through a per-user K/V cache of the history (rsys_rank_cache_*)
int model_rank_cache_reserve(Model* m, int n_slots);
int model_rank_cache_store(Model* m, const int32_t* row_adapter, const int32_t* n_hist, const int32_t* slot);
int model_rank_cache_candidates(Model* m, const int32_t* row_adapter, const int32_t* slot, const int32_t* n_cand, float* out);
int model_rank_cache_store_packed(Model* m, const int32_t* seg_adapter, int n_seg, const int32_t* seg);                    // seg [n_seg][4] = (row, first column, n_hist, slot)
int model_rank_cache_candidates_packed(Model* m, const int32_t* seg_adapter, int n_seg, const int32_t* seg, float* out);   // seg [n_seg][4] = (row, first column, n_cand, slot)
int model_rank_cache_get(Model* m, int layer, int slot, void* out, int64_t bytes);   // a slot's K | V rows of one layer, [2 n_hist][2 KV hd], compute dtype
void rank_cache_free(Model* m);
// the two passes without a host wait, for a caller whose rows (and, for the candidates, RoPE positions d_pos [rows][2S], selection d_sel
// [ntok] and output d_out [ntok]) are on the device: rsys_render_request_full.  tab: host [3 max_rows], filled here and read by a
// stream-ordered copy, as row_adapter is -- both stay valid until the stream has passed the call
int rank_cache_store_rows(Model* m, const int32_t* row_adapter, const int32_t* n_hist, const int32_t* slot, int* tab);
int rank_cache_candidates_rows(Model* m, const int32_t* row_adapter, const int32_t* slot, const int32_t* n_cand, int* tab, int* d_pos,
                               const int* d_sel, int64_t ntok, float* d_out);
// the packed store pass without a host wait: seg (host, [n_seg][4] = (row, first column, n_hist, slot)) and seg_adapter are read by
// stream-ordered copies; d_pos [rows][2 row_len] (device) holds the tokens' RoPE positions, relative to their segments
int rank_cache_store_packed_rows(Model* m, const int32_t* seg_adapter, int n_seg, const int32_t* seg, int* d_pos);
template <typename T> int rank_cache_store_layer(Model* m, int l, const T* qkv);      // forward_trunk, rc_mode == 1
template <typename T> int rank_cache_attention(Model* m, int l, const T* qkv, T* O);  // forward_trunk, rc_mode == 2
// the inference forward over the resident batch with the tokens to report (n_sel flat indices) and the rating head's values on the device
template <typename T> int infer_rows_device(Model* m, int task, const int* d_sel, int64_t ntok, float* dst, const float** rows_f32);
template <typename T> int infer_trunk(Model* m);   // its first part alone: the batch as given (no masking) through forward_trunk
int model_item_table(Model* m, float* out, int64_t n);
// the fp32 item table rows [V_m][D] of `medium` on the model's device (rsys_sim_features_from_model); the model's stream is idle on return
int model_item_table_device(Model* m, int medium, const float** rows, int64_t* Vm, int* D);
int model_materialise_trunk_output(Model* m);   // dense trunk output of the resident forward in m->out (a training pass computes it at the selected tokens only)
int model_finalize_grads(Model* m);
bool model_finalize_splittable(const Model* m);
int model_batch_prefetch(Model* m, const rsys_batch* b);   // stage + copy the NEXT batch beside the running step (replicated table only)
int model_batch_swap(Model* m);                            // the prefetched batch becomes the resident one
int model_split_table_enable(Model* m, int on);
int model_split_table_arm(Model* m, struct rsys_comm* c);   // at the head of the communicator's stream: the ranks' maximum of distinct ids of their resident batches
int model_split_table_tail(Model* m, struct rsys_comm* c, hipStream_t cs, int64_t* rows_out);   // on cs: gather the ranks' token rows (*rows_out per rank), G[E] = tbl_R + rows
int model_finalize_stage(Model* m, int stage /*1: prepare, 2: dWp GEMM*/, int64_t* wp_off, int64_t* wp_n);
int model_clip(Model* m, float max_norm, float* norm_out);
int model_set_deterministic(Model* m, int on);
int model_ensure_det_scratch(Model* m);   // the mode's scratch without switching the mode on (adapter_bank.hip: its passes use it whatever the mode)
// retrieve.hip: retrieval top-k over the fused item table of a medium (rsys_retrieve_topk) and the selection alone (rsys_op_topk)
int model_retrieve_topk(Model* m, int medium, const float* queries, int64_t nq, const int32_t* group, int32_t ng, const float* prior,
                        const int64_t* excl_off, const int32_t* excl_ids, int32_t k, int32_t* ids_out, float* scores_out, int32_t* counts_out);
// the same pipeline with a device-side initialiser of the group score rows sc [n_groups][V_m] (prior and NaN masks)
using RetrieveInit = std::function<int(float* sc, hipStream_t s)>;
struct RetrieveDev;
// win != nullptr (rsys_retrieve_window): instead of the top k, the ranks [start[g], start[g] + len[g]) of group g's ordering, 1 <= len <=
// 1024, in rows of 1024 (k is not read); total_out[g] = the group's admissible items; groups may be empty and nq may be 0
struct RetrieveWin { const int64_t* start; const int32_t* len; int32_t* total_out; };
int model_retrieve_run(Model* m, int medium, const float* queries, int64_t nq, const int32_t* group, int32_t ng, const RetrieveInit& init,
                       int32_t k, int32_t* ids_out, float* scores_out, int32_t* counts_out, RetrieveDev* dev = nullptr,
                       const RetrieveWin* win = nullptr, const float* user_w = nullptr);
// z = Q F_m^T and lse of one chunk of <= RETRIEVE_CHUNK query rows (part: nc * RETRIEVE_LSE_SPLIT float2), as rsys_retrieve_topk scores
constexpr int RETRIEVE_CHUNK = 256, RETRIEVE_LSE_SPLIT = 64;
template <typename T>
int retrieve_chunk_scores(Model* m, const T* qt, int nc, int q0, const T* Fm, int Vm, float* z, long long ldz, float2* part, float* lse);
// retrieve_request.hip: the serving tables of rsys_retrieve_request (relations, item similarity, released set) and the request
int model_retrieve_relations_set(Model* m, int medium, int kind, int64_t n_rows, int64_t n_cols, const int64_t* colptr, const int32_t* rowval,
                                 const float* nzval);
int model_retrieve_similarity_set(Model* m, int medium, int64_t dim, const float* emb, const float* crossproject);
int model_retrieve_released_set(Model* m, int medium, const uint8_t* mask);
// The one retrieval request: rsys_retrieve_request, rsys_retrieve_window and the retrieval stages of the page pipelines.
// win == nullptr: the top k of every group; else a window of each group's ordering (RetrieveWin; k is not read, rows of 1024).
// dev == nullptr: the queries are rq.queries and the rows [ng][k] go to ids_out / scores_out (host); else the queries are read from, and
// the result is left in, device memory (RetrieveDev; ids_out / scores_out are not read) and only counts_out crosses to the host.
int model_retrieve_request(Model* m, int medium, const Request& rq, int32_t k, const RetrieveWin* win, RetrieveDev* dev, int32_t* ids_out,
                           float* scores_out, int32_t* counts_out);
void retrieve_tables_free(Model* m);
// d_queries [nq][D] fp32; after the call *d_ids / *d_vals point at the [ng][k] result rows in the retrieval workspace (valid until the
// next retrieval call on the model)
struct RetrieveDev { const float* d_queries = nullptr; int32_t* d_ids = nullptr; float* d_vals = nullptr; };
const float* retrieve_similarity_table(Model* m, int medium, int64_t* dim);   // "embeddings.{m}" [V_m][dim] on the device, or null
// rank_request.hip: ranking and diversity reranking of retrieved candidates (rsys_rank_related_set, rsys_rank_request, test hooks)
int model_rank_related_set(Model* m, int medium, int64_t n, const int64_t* colptr, const int32_t* rowval, const float* nzval);
// The candidates of a ranking request and how they are scored, host arrays: group g's candidates cand_ids[cand_off[g] .. cand_off[g + 1])
// (null where they are on the device, RankDev), its partialk and four penalties, the users' r_masked values (n_rm of them, ragged over
// users; null with RankDev or r_in), the coefficients (null: not given) and r_in (given: the scores themselves, nothing is scored).
struct RankCands {
  const int64_t* cand_off = nullptr; const int32_t* cand_ids = nullptr; const int32_t* partialk = nullptr; const float* penalties = nullptr;
  const float* r_masked = nullptr; int64_t n_rm = 0;
  const float* retrieval_coef = nullptr; const float* rating_coefs = nullptr; float rating_mean = 0.f;
  const float* r_in = nullptr;
};
// rq: the users (rq.nq of them, rq.queries), their groups and list items; rq.sel is not read, of rq.qw only the user weights
int model_rank_request(Model* m, int medium, const Request& rq, const RankCands& rc, int32_t* ids_out, float* r_out);
int model_rank_gram(Model* m, int medium, int32_t ng, const int64_t* cand_off, const int32_t* cand_ids, float* out, int64_t n_out);
// the same request with candidates, queries and r_masked read from device memory (rsys_render_request): d_cand [n_total] distinct ids in
// [0, V_m) per group (a retrieval result), d_queries [nu][D], d_rm ragged over users.  Group g's page = picks [page_lo[g], page_hi[g]) of
// its pick order, written to page_out (host) at page_off[g]; keep_r / keep_picks (host, n_total each, may be null) receive the ranking
// scores and the picked positions.  Only those cross to the host.
struct RankDev { const int32_t* d_cand; const float* d_queries; const float* d_rm; const int32_t *page_lo, *page_hi; const int64_t* page_off;
                 int32_t* page_out; float* keep_r; int32_t* keep_picks; };
int model_rank_request_dev(Model* m, int medium, const Request& rq, const RankCands& rc, const RankDev* dev);
// reranking alone on device candidates (rsys_render_items: a state without users): r = +0.0 for every candidate, no related flags
int model_rank_items_dev(Model* m, int medium, int32_t ng, const int64_t* cand_off, const RankDev* dev, const int32_t* partialk,
                         const float* penalties);
void rank_free(Model* m);
// render_request.hip: a page from raw histories in one device pipeline (rsys_render_request) and its test hooks
// One request of rsys_render_request (full == false) or rsys_render_request_full (full == true: the ranking forward on full-length
// histories through the K/V cache; pb == nullptr, P == 0, user_desc[u][0] = the history columns of retrieval row u).  The fields are
// the C functions' arguments in their order: rb = retrieval_rows, pb / P = ranking_prefix / prefix_stride, slots = adapter_slots.
struct RenderArgs {
  bool full;
  int32_t ng; const int32_t* group_medium; const int64_t* offset; const int32_t* limit; const float* penalties;
  int64_t nu; const int32_t* group; const rsys_batch* rb; const int32_t* retrieval_token; const rsys_batch* pb; int32_t P;
  const int32_t* user_desc; const double* user_ts; const int32_t* slots;
  HistoryList hist_list; SelectedList sel_list;   // (hist_offsets .. hist_status, sel_offsets .. sel_ids)
  const int32_t* coef_have; const float* coefs;
  int32_t* ids_out; int64_t ids_cap; int64_t* ids_offsets; int32_t* total_out;
  QueryWeights qw;   // not a C argument: the pending weights the entry point took (user order / selected-item order of the call)
  QueryTexts qt[2];  // not C arguments: the pending text queries the entry point took, per medium (groups of the call)
};
int model_render(Model* m, const RenderArgs& a);
// rsys_render_items: a page per user-less state (windowed retrieval on the prior, reranking) in one device pipeline
int model_render_items(Model* m, int32_t ng, const int32_t* group_medium, const int64_t* offset, const int32_t* limit, const float* penalties,
                       const SelectedList& sel, int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out,
                       const float* sel_w = nullptr, const QueryTexts* qt = nullptr /* [2], per medium */);
int render_debug_keep(Model* m, int on);
int render_debug_get(Model* m, const char* key, void* out, int64_t cap, int64_t* bytes);
void render_free(Model* m);
int op_rerank(int32_t n, int32_t partialk, const float* pen, const float* r, const float* gram, const int32_t* ss_bits,
              const int32_t* related_bits, int32_t* picks);
int op_topk(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, int32_t* ids, float* vals, int32_t* counts);
// rsys_op_topk_window / rsys_op_lse: the windowed selection and the log-sum-exp launches alone, on device arrays (include/rsys_debug.h)
int op_topk_window(const float* scores, int64_t ld, int32_t rows, int32_t V, const int64_t* start, const int32_t* len, int32_t* ids,
                   float* vals, int32_t* counts, int32_t* totals, int32_t* bounds);
int op_lse(const float* z, int64_t ldz, int32_t rows, int32_t V, float* lse);
// the launches behind rsys_op_lse on stream s: lse[row] of z [rows][ldz] over V columns; part: rows * RETRIEVE_LSE_SPLIT float2 of scratch
int lse_rows(const float* z, long long ldz, int rows, int V, float2* part, float* lse, hipStream_t s);
// text queries.  search.hip: the setter behind rsys_query_texts_set.  retrieve.hip: sc[g][i] = weighted_add(sc[g][i],
// w_t, z_t[i] - lse_t) over group g's texts in text order, one in-place launch of combine_w_kernel<false> (members / ranges: device, text_plan)
int model_query_texts_set(Model* m, void* search, int medium, const float* x, int64_t n, const int32_t* group, const float* w);
int retrieve_text_terms(float* sc, int ng, int V, const QueryTexts& qt, const int32_t* d_members, const int32_t* d_ranges, hipStream_t s);
// rsys_op_query_weights: the three weighted accumulations alone, on device arrays (one section each; include/rsys_debug.h)
int op_combine_weighted(const float* src, float* dst, int32_t ng, int32_t V, int32_t last, const float* z, int64_t ldz, const float* lse,
                        const int32_t* members, const int32_t* ranges, int32_t q0, const float* user_w);
int op_rank_score_weighted(int32_t ng, const int64_t* cand_off, const int32_t* cand, const float* z, int64_t ldz, const float* lse,
                           const int32_t* members, const int32_t* ranges, int32_t q0, const float* rm, const int64_t* rm_off,
                           const float* retrieval_coef, const float* rating_coefs, float rating_mean, int32_t first, const float* user_w,
                           float* sc);
int op_selected_sum_weighted(int32_t ng, const int64_t* sel_off, const int32_t* sel_med, const int32_t* sel_ids, int32_t medium,
                             const float* emb_m, const float* X, int32_t dim, const float* sel_w, float* S);
// the selection of rsys_op_topk on device scores [rows][ld], stream-ordered, in a caller's device workspace of topk_rows_ws_bytes bytes
// (1 <= k <= min(V, 8192)); ids / vals / counts are device arrays
size_t topk_rows_ws_bytes(int rows, int V, int k);
int topk_rows(const float* scores, long long ld, int rows, int V, int k, void* ws, int* ids, float* vals, int* counts, hipStream_t s);
// retrieve_eval.hip: the rank and log-probability of one target item per query (rsys_retrieve_target_rank) and the count alone
int model_retrieve_target_rank(Model* m, int medium, const float* queries, int64_t nq, const int32_t* targets, const int64_t* excl_off,
                               const int32_t* excl_ids, int32_t* rank_out, float* logp_out);
int op_target_rank(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* targets, int32_t* rank_out);
// similarity_metrics.hip: catalogue ranks of the targets of item-similarity test sources (rsys_sim_pair_ranks) over a handle's fp32
// export [V][E] and test-mask bit rows, the masked score rows alone (rsys_sim_pair_scores) and the count alone (rsys_op_pair_ranks).
// ws: the caller's workspace, grown on demand
int pair_ranks_run(const float* exp32, int V, int E, const unsigned* tmask, long long tmw, int32_t n_src, const int32_t* sources,
                   const int64_t* off, const int32_t* tids, int32_t* ranks_out, DevScratch* ws, hipStream_t s);
int pair_scores_run(const float* exp32, int V, int E, const unsigned* tmask, long long tmw, int32_t n_src, const int32_t* sources,
                    float* out, DevScratch* ws, hipStream_t s);
int op_pair_ranks(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* self, const int64_t* off, const int32_t* tids,
                  int32_t* ranks_out);
int optimizer_step(Optimizer* o, float lr_factor, float clip, float grad_div);

}  // namespace rsys
