// Which batch is resident: the layout of a batch's arrays in a slot's blob, the host-side check and packer of an upload
// (no Model, no HIP: rsys_debug_batch_pack runs them without a GPU), the one installer, and the five entry points that end in it.
#include "model_internal.hpp"

namespace rsys {

BlobLayout blob_layout(size_t N) {
  BlobLayout L{};
  size_t off = 0;
  auto place = [&](size_t bytes) { const size_t at = off; off += (bytes + 63) / 64 * 64; return at; };
  L.time = place(N * 8);
  L.userid = place(N * 4); L.tmid = place(N * 4); L.gender = place(N * 4); L.source = place(N * 4);
  L.matchedid = place(N * 4); L.status = place(N * 4); L.rating = place(N * 4); L.progress = place(N * 4);
  for (int k = 0; k < 6; ++k) { L.label[k] = place(N * 4); L.weight[k] = place(N * 4); L.position[k] = place(N * 4); }
  L.wm = place(N); L.rm = place(N);
  L.rope = place(2 * N * 4);
  L.bytes = off;
  return L;
}
// the device addresses of a layout's arrays in `blob`, the optional ones only where the batch has them (the mask_tokens outputs stay the model's)
static void blob_point(unsigned char* blob, const BlobLayout& L, bool masks, bool rope, BatchDev& d) {
  d.time = (const double*)(blob + L.time);
  d.userid = (const int*)(blob + L.userid); d.tmid = (const int*)(blob + L.tmid);
  d.gender = (const int*)(blob + L.gender); d.source = (const int*)(blob + L.source);
  d.matchedid = (const int*)(blob + L.matchedid); d.status = (const int*)(blob + L.status);
  d.rating = (const float*)(blob + L.rating); d.progress = (const float*)(blob + L.progress);
  for (int k = 0; k < 6; ++k) {
    d.label[k] = (const float*)(blob + L.label[k]); d.weight[k] = (const float*)(blob + L.weight[k]); d.position[k] = (const int*)(blob + L.position[k]);
  }
  d.watch_mask = masks ? blob + L.wm : nullptr; d.rating_mask = masks ? blob + L.rm : nullptr;
  d.rope_pos = rope ? (const int*)(blob + L.rope) : nullptr;
}

// ------------------------------------------------------------------ host batch -> staging buffer (no Model, no HIP)
int batch_check(const BatchLimits& lim, const rsys_batch* b, int row_len, std::vector<unsigned long long>* id_seen, int* distinct_ids) {
  ARG_CHECK(b != nullptr, "null batch");
  ARG_CHECK(row_len >= 4 && row_len <= lim.Sa && row_len % 4 == 0, "trimmed upload: row_len % 4 == 0 and 4 <= row_len <= max_sequence_length");
  ARG_CHECK(b->rows >= 1 && b->rows <= lim.rows_max, "batch rows must be in [1, max_rows]");
  ARG_CHECK(b->userid && b->token_mask_ids && b->gender && b->source && b->matchedid && b->status && b->time && b->rating && b->progress,
            "batch arrays must not be null");
  const bool full = row_len == lim.Sa;   // (the ordinary upload; a trimmed one reads neither targets nor masks)
  if (full) {
    for (int k = 0; k < 6; ++k) {
      if (k % 3 == 2 && b->label[k] == nullptr) continue;  // status targets are never used by the losses (model.py:448-449)
      ARG_CHECK(b->label[k] && b->weight[k] && b->position[k], "target arrays must not be null");
    }
    ARG_CHECK(b->watch_mask == nullptr || b->rating_mask != nullptr, "watch_mask and rating_mask come together");
  }
  // index paths and the dead suffix are checked on the host BEFORE anything is written: a rejected batch leaves the resident one untouched
  const size_t Sa = (size_t)lim.Sa;
  const int32_t* rp = b->rope_input_pos;
  int distinct = 1;       // the mask row V: mask_tokens sends the masked events there (model.py:451)
  if (id_seen) id_seen->assign(((size_t)lim.V + 64) / 64, 0ull);
  for (int r = 0; r < b->rows; ++r) {
    const size_t r0 = (size_t)r * Sa;
    for (size_t i = r0; i < r0 + row_len; ++i) {
      ARG_CHECK(b->matchedid[i] >= -1 && b->matchedid[i] < lim.V, "matchedid out of range");
      // the attention kernels compare tokens through the key userid << 12 | token_mask_ids (attention_maps.hip: token_key)
      ARG_CHECK(b->userid[i] >= 0 && b->userid[i] < (1 << 19), "userid must be in [0, 2^19)");
      ARG_CHECK(b->token_mask_ids[i] >= 0 && b->token_mask_ids[i] < 4096, "token_mask_ids must be in [0, 4096)");
      ARG_CHECK(b->status[i] >= -1 && b->status[i] <= lim.vocab_status, "status out of range");
      ARG_CHECK(b->gender[i] >= -1 && b->gender[i] <= lim.vocab_gender, "gender out of range");
      ARG_CHECK(b->source[i] >= -1 && b->source[i] <= lim.vocab_source, "source out of range");
      if (full) {
        ARG_CHECK(b->position[0][i] >= 0 && b->position[0][i] < lim.V0 && b->position[1][i] >= 0 && b->position[1][i] < lim.V0,
                  "manga target position out of range");
        ARG_CHECK(b->position[3][i] >= 0 && b->position[3][i] < lim.V1 && b->position[4][i] >= 0 && b->position[4][i] < lim.V1,
                  "anime target position out of range");
      }
      // model.py:470-476: token positions 2 p, 2 p + 1 -- positions, not columns: the RoPE table's bound at any row_len
      if (rp) ARG_CHECK(rp[i] >= 0 && rp[i] < lim.Ta / 2, "rope_input_pos out of range");
      if (id_seen) {   // (a bitmap of the table's rows: ~30 us for 32 K ids, on the thread that packs the batch anyway)
        const int id = b->matchedid[i] < 0 ? lim.V : b->matchedid[i];
        unsigned long long& wd = (*id_seen)[(size_t)id >> 6];
        const unsigned long long bit = 1ull << (id & 63);
        if (!(wd & bit)) { wd |= bit; if (id != lim.V) ++distinct; }
      }
    }
    for (size_t i = r0 + row_len; i < r0 + Sa; ++i)
      ARG_CHECK(b->userid[i] == 0, "trimmed upload: a live event (userid != 0) at or behind column row_len");
  }
  if (id_seen) *distinct_ids = distinct;
  return RSYS_OK;
}

void batch_pack(const BatchLimits& lim, const rsys_batch* b, int row_len, const BlobLayout& L, unsigned char* stage) {
  const size_t rows = (size_t)b->rows, Sa = (size_t)lim.Sa, rl = (size_t)row_len;
  const bool full = row_len == lim.Sa;
  // an absent array's place stays unwritten (nothing reads it).  The ordinary upload is one memcpy per array; a trimmed one moves columns
  // [0, row_len) of every row from stride Sa to stride row_len
  auto put = [&](size_t at, const void* src, size_t esz) {
    if (src == nullptr) return;
    if (full) { memcpy(stage + at, src, rows * Sa * esz); return; }
    for (size_t r = 0; r < rows; ++r) memcpy(stage + at + r * rl * esz, (const unsigned char*)src + r * Sa * esz, rl * esz);
  };
  put(L.time, b->time, 8);
  put(L.userid, b->userid, 4); put(L.tmid, b->token_mask_ids, 4); put(L.gender, b->gender, 4); put(L.source, b->source, 4);
  put(L.matchedid, b->matchedid, 4); put(L.status, b->status, 4); put(L.rating, b->rating, 4); put(L.progress, b->progress, 4);
  if (full) {
    for (int k = 0; k < 6; ++k) {   // (status targets may be absent)
      put(L.label[k], b->label[k], 4); put(L.weight[k], b->weight[k], 4); put(L.position[k], b->position[k], 4);
    }
    put(L.wm, b->watch_mask, 1); put(L.rm, b->rating_mask, 1);
  }
  if (b->rope_input_pos) {   // model.py:470-476: token positions 2 p, 2 p + 1
    int* pos = (int*)(stage + L.rope);
    for (size_t r = 0; r < rows; ++r)
      for (size_t j = 0; j < rl; ++j) {
        const int p = b->rope_input_pos[r * Sa + j];
        *pos++ = 2 * p; *pos++ = 2 * p + 1;
      }
  }
}

// ------------------------------------------------------------------ the resident batch
static BatchLimits batch_limits(const Model* m) {
  return {m->rows_max, m->Sa, m->Ta, m->V, m->V0, m->V1, m->cfg.vocab_status, m->cfg.vocab_gender, m->cfg.vocab_source};
}

// The only writer of the resident value and of what follows from it: the row length everything that walks the batch reads (S / T), the host's
// bound of the split table reduce's row list, and the two "built for this batch" flags -- the inverted index "table row -> its tokens" of the
// backward's segmented scatter depends on the batch only and is built by the first backward over it (an inference or evaluation pass never
// needs it; the row-sharded table builds it at upload, for its exchange plan).  landed == false: the batch's copy is still to be enqueued --
// cur_rows stays 0 until batch_landed, so that a failing copy does not leave a half-written batch marked as resident.
static void batch_install(Model* m, const ResidentBatch& rb, bool landed) {
  m->resident = rb;
  set_row_len(m, rb.row_len);
  m->u_bound_host = rb.distinct_ids;
  m->tok_index_valid = false;
  m->split_plan_valid = false;
  m->cur_rows = landed ? rb.rows : 0;
}
static void batch_landed(Model* m) { m->cur_rows = m->resident.rows; }

// A new batch supersedes a prefetched one.  Its copy may still be reading the OTHER slot's staging buffer on the copy stream: wait for it
// here, so that the next prefetch (which skips its own wait when nothing is pending) never re-packs a buffer under a copy.
static int pending_drop(Model* m) {
  if (m->pending_valid) HIP_CHECK(hipEventSynchronize(m->ev_copy_done));
  m->pending_valid = false;
  return RSYS_OK;
}

// the check of an upload of rows of row_len interactions; rb receives what it found (the split table reduce counts full rows only)
static int batch_checked(Model* m, const rsys_batch* b, int row_len, ResidentBatch& rb) {
  RC(batch_check(batch_limits(m), b, row_len, m->split_table && row_len == m->Sa ? &m->id_seen : nullptr, &rb.distinct_ids));
  rb.rows = b->rows; rb.row_len = row_len;
  return RSYS_OK;
}
// packs a checked batch into staging buffer `slot` (pinned): one H2D of *bytes then puts its arrays into the slot's blob, where rb.bd says
static int batch_stage(Model* m, const rsys_batch* b, int slot, ResidentBatch& rb, size_t* bytes) {
  const BlobLayout L = blob_layout((size_t)rb.rows * rb.row_len);
  if (L.bytes > m->raw_bytes) { set_error("batch upload: staging buffer too small"); return RSYS_ERR_STATE; }
  batch_pack(batch_limits(m), b, rb.row_len, L, m->slot_stage[slot]);
  rb.bd = m->resident.bd;    // (the mask_tokens outputs are the model's own; only the input arrays move)
  blob_point(m->slot_blob[slot], L, rb.row_len == m->Sa && b->watch_mask != nullptr, b->rope_input_pos != nullptr, rb.bd);
  *bytes = L.bytes;
  return RSYS_OK;
}

// Row-sharded table: which rows of which rank this batch reads.  Depends on the batch only (a watch-masked token reads
// the mask row V instead of its item's row, and V is always part of the plan), so it is built once per upload:
// distinct ids (sorted) -> contiguous runs per owner -> counts all-gathered -> id lists exchanged.  Every rank calls this
// at the same point (it contains collectives).
static int build_exchange_plan(Model* m, int N) {
  const int W = m->sh_world;
  hipStream_t s = m->stream;
  ARG_CHECK(W == 1 || m->shard_comm != nullptr, "row-sharded table: call rsys_model_set_shard_comm before the first batch");
  RC(launch_plan_unique(m->tok_skey, m->tok_sidx, N, m->V, m->u_slot, m->u_ids, m->u_tok, m->u_plan, s));
  int* d_off = m->u_off; int* d_cnt = m->u_off + (W + 1); int* d_all = d_cnt + W;
  RC(launch_plan_offsets(m->u_ids, m->u_plan, m->u_bound, W + 1, d_off, s));
  int plan[2]; std::vector<int> off(W + 1), cnt(W), all((size_t)W * W);
  HIP_CHECK(hipMemcpyAsync(plan, m->u_plan, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(off.data(), d_off, (W + 1) * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  m->U = plan[0]; m->uV = plan[1];
  ARG_CHECK(off[W] == m->U && m->U >= 1 && m->U <= N + 1, "exchange plan: inconsistent unique-id list");
  for (int q = 0; q <= W; ++q) { m->need_off[q] = off[q]; m->need_offD[q] = (long long)off[q] * m->D; }
  for (int q = 0; q < W; ++q) cnt[q] = off[q + 1] - off[q];
  HIP_CHECK(hipMemcpyAsync(d_cnt, cnt.data(), W * 4, hipMemcpyHostToDevice, s));
  RC(comm_all_gather(m->shard_comm, d_cnt, d_all, (size_t)W * 4, s));
  HIP_CHECK(hipMemcpyAsync(all.data(), d_all, (size_t)W * W * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  long long acc = 0;
  for (int q = 0; q < W; ++q) { m->serve_off[q] = acc; m->serve_offD[q] = acc * m->D; acc += all[(size_t)q * W + m->sh_rank]; }
  m->serve_off[W] = acc; m->serve_offD[W] = acc * m->D; m->R = acc;
  if (acc > m->req_cap) {
    if (m->req_ids) HIP_CHECK(hipFree(m->req_ids));
    if (m->rows_xchg) HIP_CHECK(hipFree(m->rows_xchg));
    m->req_cap = acc + acc / 4 + 1024;
    HIP_CHECK(hipMalloc((void**)&m->req_ids, (size_t)m->req_cap * 4));
    HIP_CHECK(hipMalloc((void**)&m->rows_xchg, (size_t)m->req_cap * m->D * 4));
  }
  RC(comm_exchange(m->shard_comm, m->u_ids, m->need_off.data(), m->req_ids, m->serve_off.data(), 4, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

// The two uploads: a checked batch (rb: its rows, row length and id count) is packed, copied into the current slot and resident on return.
// No wait before packing: the previous upload synchronised after ITS copy, so the staging buffer is free, and the copy below is
// ordered on the stream behind the kernels that still read the old batch -- the host packs while the GPU finishes the previous
// step's optimizer pass.  (A prefetch into this slot's staging is complete too: model_batch_swap waited for its copy.)
static int upload_checked(Model* m, const rsys_batch* b, ResidentBatch& rb) {
  hipStream_t s = m->stream;
  size_t bytes = 0;
  RC(batch_stage(m, b, m->cur_slot, rb, &bytes));
  batch_install(m, rb, false);   // (a failing copy below must not leave a half-written batch marked as resident)
  HIP_CHECK(hipMemcpyAsync(m->slot_blob[m->cur_slot], m->slot_stage[m->cur_slot], bytes, hipMemcpyHostToDevice, s));
  const int N = rb.rows * rb.row_len;
  if (m->sharded) { RC(launch_token_index_build(rb.bd.matchedid, N, m->V, m->tok_keys, m->tok_skey, m->tok_sidx, s)); m->tok_index_valid = true; }
  HIP_CHECK(hipStreamSynchronize(s));
  if (m->sharded) RC(build_exchange_plan(m, N));
  batch_landed(m);
  return RSYS_OK;
}

int model_batch_upload(Model* m, const rsys_batch* b) {
  HIP_CHECK(hipSetDevice(m->device));
  RC(pending_drop(m));
  ResidentBatch rb;
  RC(batch_checked(m, b, m->Sa, rb));
  return upload_checked(m, b, rb);
}

// A trimmed batch holds no targets and no masks: every pass that reads them refuses it and touches nothing.
int check_not_trimmed(const Model* m) {
  if (!batch_trimmed(m)) return RSYS_OK;
  set_error("a trimmed batch is inference-only (rsys_batch_upload_trimmed): upload the full rows for this call");
  return RSYS_ERR_STATE;
}

// rsys_batch_upload_trimmed.  The caller's arrays keep the row stride Sa; columns [0, row_len) of every row are checked,
// packed at stride row_len and copied, and the resident batch then has rows of row_len interactions: every kernel of the inference
// forward is launched over rows * 2 row_len tokens.  Exact because the dropped columns are padding (userid 0), which no live token
// attends (the mask's first predicate is the user id) and every other operator of the trunk is token-local.  Targets and masks are not
// read; their blob places stay unwritten and nothing of an inference forward reads them.
int model_batch_upload_trimmed(Model* m, const rsys_batch* b, int row_len) {
  ARG_CHECK(b != nullptr, "null batch");
  ARG_CHECK(row_len >= 4 && row_len <= m->Sa && row_len % 4 == 0, "trimmed upload: row_len % 4 == 0 and 4 <= row_len <= max_sequence_length");
  ARG_CHECK(!m->fp8, "trimmed upload: fp32 and bf16 models only (the fp8 trunk's tensor-wise amax sees every token)");
  ARG_CHECK(!m->sharded, "trimmed upload: a model with a replicated table");
  if (row_len == m->Sa) return model_batch_upload(m, b);
  ResidentBatch rb;
  RC(batch_checked(m, b, row_len, rb));
  HIP_CHECK(hipSetDevice(m->device));
  RC(pending_drop(m));   // (as model_batch_upload: an explicit upload supersedes a prefetched batch)
  return upload_checked(m, b, rb);
}

// The resident batch as device arrays for a kernel to fill (rsys_render_request's ranking rows): the layout of an upload for `rows`
// rows in the current slot's blob, nothing copied.  Everything enqueued so far that reads the blob runs before the kernel that fills it
// (same stream); the slot's staging buffer is not touched.
int model_batch_device_begin(Model* m, int rows, BatchDevRows* out, int row_len) {
  ARG_CHECK(rows >= 1 && rows <= m->rows_max, "batch rows must be in [1, max_rows]");
  if (row_len == 0) row_len = m->Sa;
  ARG_CHECK(row_len >= 4 && row_len <= m->Sa && row_len % 4 == 0, "device-assembled batch: row_len % 4 == 0 and 4 <= row_len <= max_sequence_length");
  ARG_CHECK(!m->sharded, "device-assembled batch: replicated table only");
  HIP_CHECK(hipSetDevice(m->device));
  RC(pending_drop(m));
  const BlobLayout L = blob_layout((size_t)rows * row_len);
  if (L.bytes > m->raw_bytes) { set_error("device-assembled batch: blob too small"); return RSYS_ERR_STATE; }
  ResidentBatch rb;
  rb.bd = m->resident.bd; rb.rows = rows; rb.row_len = row_len;
  blob_point(m->slot_blob[m->cur_slot], L, false, true, rb.bd);
  const BatchDev& d = rb.bd;
  out->time = (double*)d.time; out->userid = (int*)d.userid; out->tmid = (int*)d.tmid; out->gender = (int*)d.gender;
  out->source = (int*)d.source; out->matchedid = (int*)d.matchedid; out->status = (int*)d.status; out->rating = (float*)d.rating;
  out->progress = (float*)d.progress; out->rope_pos = (int*)d.rope_pos;
  batch_install(m, rb, true);
  return RSYS_OK;
}

// The NEXT batch beside the running step: checked and packed into the other slot's staging buffer by the calling thread while the GPU
// works, copied on a stream of its own.  Nothing of the resident batch changes until model_batch_swap.
int model_batch_prefetch(Model* m, const rsys_batch* b) {
  ARG_CHECK(!m->sharded, "batch prefetch: the row-sharded table builds its exchange plan at upload (use rsys_batch_upload)");
  HIP_CHECK(hipSetDevice(m->device));
  const int slot = m->cur_slot ^ 1;
  RC(pending_drop(m));   // (a prefetch that was never swapped in: its copy still reads the staging buffer)
  ResidentBatch rb;
  size_t bytes = 0;
  RC(batch_checked(m, b, m->Sa, rb));
  RC(batch_stage(m, b, slot, rb, &bytes));
  // the slot's blob was the resident batch two swaps ago: the kernels that read it were enqueued before ev_blob_free[slot]
  if (m->blob_free_valid[slot]) HIP_CHECK(hipStreamWaitEvent(m->copy_stream, m->ev_blob_free[slot], 0));
  HIP_CHECK(hipMemcpyAsync(m->slot_blob[slot], m->slot_stage[slot], bytes, hipMemcpyHostToDevice, m->copy_stream));
  HIP_CHECK(hipEventRecord(m->ev_copy_done, m->copy_stream));
  m->pending = rb; m->pending_valid = true;
  return RSYS_OK;
}

int model_batch_swap(Model* m) {
  ARG_CHECK(m->pending_valid, "batch swap: no prefetched batch (rsys_batch_prefetch first)");
  HIP_CHECK(hipSetDevice(m->device));
  // everything enqueued so far may still read the resident batch's blob: the next prefetch into it waits for this point
  HIP_CHECK(hipEventRecord(m->ev_blob_free[m->cur_slot], m->stream));
  m->blob_free_valid[m->cur_slot] = true;
  // The copy is waited for on the HOST as well as on the stream: the next prefetch re-packs this slot's staging buffer without a wait
  // (as uploads always have), and by now -- a whole step after the copy was issued -- the wait returns at once.
  HIP_CHECK(hipStreamWaitEvent(m->stream, m->ev_copy_done, 0));
  HIP_CHECK(hipEventSynchronize(m->ev_copy_done));
  m->cur_slot ^= 1;
  batch_install(m, m->pending, true);
  m->pending_valid = false;
  return RSYS_OK;
}

}  // namespace rsys
