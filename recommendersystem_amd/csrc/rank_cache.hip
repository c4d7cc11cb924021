// Full-length ranking through a per-user K/V cache of the history (rsys_rank_cache_*; Finetune/embed.py:74-161).  The reference ranks a
// user in ONE row of max_user_len + max_ranking_items interactions: the history (token_mask_ids 0) and then the candidates (token_mask_ids
// n_hist + j, all at rope_input_pos n_hist).  Under allowed(q, kv) = same user AND (tm[kv] == 0 OR tm[q] == tm[kv]) a history token never
// sees a candidate, and a candidate sees the whole history plus its own two tokens: the history's K and V of every layer do not depend on
// the candidates.  So the history runs once, alone, in a row of the trunk's ordinary length (store: the unchanged forward_trunk, which copies K | V behind
// every layer's QKV stage -- RoPE, LoRA and adapter-bank updates included -- into the user's slot), and the candidates run as query-only
// rows against the slot (candidates: the same trunk, no tile maps, attention through attn_cand_kernel).  Everything that is not attention
// is token-local, so nothing else of the trunk changes.
#include "model_internal.hpp"

namespace rsys {

static int rc_check_model(Model* m) {
  ARG_CHECK(!m->fp8, "ranking cache: fp32 and bf16 models only");
  ARG_CHECK(!m->sharded, "ranking cache: a model with a replicated table");
  return RSYS_OK;
}
static inline size_t rc_kvw(const Model* m) { return (size_t)2 * m->KV * m->hd; }                    // values of a cached token: K | V
static inline size_t rc_layer_elems(const Model* m) { return (size_t)m->rc_slots * m->Ta * rc_kvw(m); }   // (the slot stride is the allocated row: a slot serves rows of any length)

static inline int rc_max_seg(const Model* m) { return m->rows_max * ((m->Sa + 31) / 32); }   // segments of one packed forward: one per 64-token tile at most

void rank_cache_free(Model* m) {
  if (m->rcache) (void)hipFree(m->rcache);
  if (m->rc_rows) (void)hipFree(m->rc_rows);
  if (m->rc_seg) (void)hipFree(m->rc_seg);
  m->rcache = nullptr; m->rc_rows = nullptr; m->rc_seg = nullptr; m->rc_slots = 0; m->rc_nhist.clear(); m->rc_mode = 0; m->rc_nseg = 0;
}

int model_rank_cache_reserve(Model* m, int n_slots) {
  RC(rc_check_model(m));
  ARG_CHECK(n_slots >= 0 && n_slots <= (1 << 20), "ranking cache: 0 <= n_slots <= 2^20");
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  if (n_slots == 0) { rank_cache_free(m); return RSYS_OK; }
  const size_t bytes = (size_t)m->L * n_slots * m->Ta * rc_kvw(m) * m->esz;
  const size_t held = (size_t)m->L * m->rc_slots * m->Ta * rc_kvw(m) * m->esz;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  // (checked before the old cache goes: a size that cannot fit leaves the slots that are stored where they are)
  if (bytes > free_b + held) {
    set_error("ranking cache: " + std::to_string(n_slots) + " slots need " + std::to_string(bytes) + " bytes, " + std::to_string(free_b + held) + " are free");
    return RSYS_ERR_STATE;
  }
  rank_cache_free(m);
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    set_error("ranking cache: " + std::to_string(n_slots) + " slots need " + std::to_string(bytes) + " bytes, " + std::to_string(free_b) + " are free");
    return RSYS_ERR_STATE;
  }
  // rows' {slot, n_hist, n_cand} and the candidates' RoPE positions (one per token of a full batch)
  int* rows = nullptr;
  if (hipMalloc((void**)&rows, ((size_t)3 * m->rows_max + (size_t)m->rows_max * m->Ta) * 4) != hipSuccess) {
    (void)hipGetLastError(); (void)hipFree(p);
    set_error("ranking cache: no memory for the row descriptors");
    return RSYS_ERR_STATE;
  }
  // packed rows: a segment table [max_seg][4] and the candidate rows' tile map [rows_max][ceil(Sa / 32)] behind it
  int* segs = nullptr;
  if (hipMalloc((void**)&segs, (size_t)5 * rc_max_seg(m) * 4) != hipSuccess) {
    (void)hipGetLastError(); (void)hipFree(p); (void)hipFree(rows);
    set_error("ranking cache: no memory for the segment tables");
    return RSYS_ERR_STATE;
  }
  m->rcache = p; m->rc_rows = rows; m->rc_seg = segs; m->rc_slots = n_slots;
  m->rc_nhist.assign((size_t)n_slots, -1);
  return RSYS_OK;
}

// K | V of the leading 2 n_hist[r] tokens of every row -> the row's cache slot, in 16-byte chunks (rsys_rank_cache_store, once per layer)
template <typename T>
__global__ __launch_bounds__(256) void rank_cache_copy_kernel(const T* __restrict__ qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, const int* __restrict__ slot,
                                                              const int* __restrict__ n_hist, int n_slots, T* __restrict__ cache) {
  const int r = blockIdx.y, sl = slot[r];
  if (sl < 0 || sl >= n_slots) return;
  const int ntok = 2 * min(max(n_hist[r], 0), T_len / 2);
  const int cpr = kvw * (int)sizeof(T) / 16;
  const long long n = (long long)ntok * cpr;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
    const long long tok = c / cpr; const int ch = (int)(c % cpr);
    const uint4 v = *(const uint4*)((const unsigned char*)(qkv + ((long long)r * T_len + tok) * ld + kv_off) + 16 * ch);
    *(uint4*)((unsigned char*)(cache + ((long long)sl * T_slot + tok) * kvw) + 16 * ch) = v;
  }
}
template <typename T>
int launch_rank_cache_copy(const T* qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, int rows, const int* slot, const int* n_hist, int n_slots, T* cache,
                           hipStream_t s) {
  ARG_CHECK(T_slot >= T_len, "ranking cache: rows longer than a slot");
  ARG_CHECK((kvw * sizeof(T)) % 16 == 0 && (kv_off * sizeof(T)) % 16 == 0 && (ld * sizeof(T)) % 16 == 0, "ranking cache: 16-byte row alignment");
  const int cpr = kvw * (int)sizeof(T) / 16;
  const int gx = (int)std::min<long long>(((long long)T_len * cpr + 255) / 256, 64);
  hipLaunchKernelGGL((rank_cache_copy_kernel<T>), dim3(gx, rows), dim3(256), 0, s, qkv, ld, kv_off, kvw, T_len, T_slot, slot, n_hist, n_slots, cache);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
template int launch_rank_cache_copy<bf16>(const bf16*, long long, int, int, int, int, int, const int*, const int*, int, bf16*, hipStream_t);
template int launch_rank_cache_copy<float>(const float*, long long, int, int, int, int, int, const int*, const int*, int, float*, hipStream_t);

// Packed store rows (rsys_rank_cache_store_packed): per segment descriptor seg[i] = (row, first column c0, n_hist, slot), K | V of
// tokens [2 c0, 2 c0 + 2 n_hist) of the row -> rows [0, 2 n_hist) of the slot, in 16-byte chunks; grid (chunks, segments).  A descriptor that
// does not fit the rows or the cache copies nothing.
template <typename T>
__global__ __launch_bounds__(256) void rank_cache_copy_segments_kernel(const T* __restrict__ qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, int rows,
                                                                       const int* __restrict__ seg, int n_slots, T* __restrict__ cache) {
  const int* d = seg + 4 * blockIdx.y;
  const int r = d[0], c0 = d[1], nh = d[2], sl = d[3];
  if (r < 0 || r >= rows || sl < 0 || sl >= n_slots || c0 < 0 || nh <= 0) return;
  if (2 * ((long long)c0 + nh) > T_len || 2 * (long long)nh > T_slot) return;
  const int cpr = kvw * (int)sizeof(T) / 16;
  const long long n = (long long)2 * nh * cpr;
  for (long long c = (long long)blockIdx.x * 256 + threadIdx.x; c < n; c += (long long)gridDim.x * 256) {
    const long long tok = c / cpr; const int ch = (int)(c % cpr);
    const uint4 v = *(const uint4*)((const unsigned char*)(qkv + ((long long)r * T_len + 2 * c0 + tok) * ld + kv_off) + 16 * ch);
    *(uint4*)((unsigned char*)(cache + ((long long)sl * T_slot + tok) * kvw) + 16 * ch) = v;
  }
}
template <typename T>
int launch_rank_cache_copy_segments(const T* qkv, long long ld, int kv_off, int kvw, int T_len, int T_slot, int rows, const int* seg, int n_seg, int n_slots, T* cache,
                                    hipStream_t s) {
  ARG_CHECK(T_slot >= T_len, "ranking cache: rows longer than a slot");
  ARG_CHECK(rows >= 1 && n_seg >= 1 && n_seg <= 65535 && n_slots >= 1 && seg != nullptr, "ranking cache: rows, segments and slots");
  ARG_CHECK((kvw * sizeof(T)) % 16 == 0 && (kv_off * sizeof(T)) % 16 == 0 && (ld * sizeof(T)) % 16 == 0, "ranking cache: 16-byte row alignment");
  const int cpr = kvw * (int)sizeof(T) / 16;
  const int gx = (int)std::min<long long>(((long long)T_len * cpr + 255) / 256, 64);
  hipLaunchKernelGGL((rank_cache_copy_segments_kernel<T>), dim3(gx, n_seg), dim3(256), 0, s, qkv, ld, kv_off, kvw, T_len, T_slot, rows, seg, n_slots, cache);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}
template int launch_rank_cache_copy_segments<bf16>(const bf16*, long long, int, int, int, int, int, const int*, int, int, bf16*, hipStream_t);
template int launch_rank_cache_copy_segments<float>(const float*, long long, int, int, int, int, int, const int*, int, int, float*, hipStream_t);

template <typename T>
int rank_cache_store_layer(Model* m, int l, const T* qkv) {
  tic(m, "hbm_rank_cache_store", 2.0 * sizeof(T) * m->cur_rows * m->T * (double)rc_kvw(m));
  T* const cache = (T*)m->rcache + (size_t)l * rc_layer_elems(m);
  const int rc = m->rc_nseg   // (packed store rows: one copy per segment descriptor)
                     ? launch_rank_cache_copy_segments<T>(qkv, m->Nqkv, m->H * m->hd, (int)rc_kvw(m), m->T, m->Ta, m->cur_rows, m->rc_seg, m->rc_nseg, m->rc_slots, cache, m->stream)
                     : launch_rank_cache_copy<T>(qkv, m->Nqkv, m->H * m->hd, (int)rc_kvw(m), m->T, m->Ta, m->cur_rows, m->rc_rows, m->rc_rows + m->rows_max, m->rc_slots,
                                                 cache, m->stream);
  toc(m);
  return rc;
}
template <typename T>
int rank_cache_attention(Model* m, int l, const T* qkv, T* O) {
  CandAttnParams p{};
  p.rows = m->cur_rows; p.T = m->T; p.Tc = m->Ta; p.H = m->H; p.KV = m->KV; p.hd = m->hd;
  p.qkv = qkv; p.ld = m->Nqkv;
  p.cache = (const T*)m->rcache + (size_t)l * rc_layer_elems(m); p.n_slots = m->rc_slots;
  p.slot = m->rc_rows; p.n_hist = m->rc_rows + m->rows_max; p.n_cand = m->rc_rows + 2 * m->rows_max;
  p.o = O; p.ldo = m->D;
  if (m->rc_nseg) { p.seg = m->rc_seg; p.tile_seg = m->rc_seg + 4 * rc_max_seg(m); p.n_seg = m->rc_nseg; }   // packed candidate rows: slot per tile
  tic(m, "attn_cand");
  const int rc = launch_attn_cand<T>(p, m->stream);
  toc(m);
  return rc;
}
template int rank_cache_store_layer<float>(Model*, int, const float*);
template int rank_cache_store_layer<bf16>(Model*, int, const bf16*);
template int rank_cache_attention<float>(Model*, int, const float*, float*);
template int rank_cache_attention<bf16>(Model*, int, const bf16*, bf16*);

static int rc_check_call(Model* m, const int32_t* a, const int32_t* b) {
  RC(rc_check_model(m));
  ARG_CHECK(m->rcache != nullptr, "ranking cache: nothing reserved (rsys_rank_cache_reserve)");
  ARG_CHECK(m->cur_rows > 0, "no batch uploaded");
  ARG_CHECK(a != nullptr && b != nullptr, "ranking cache: null row arrays");
  return RSYS_OK;
}

// The rows' RoPE positions are the caller's for the length of a cache call: the resident batch runs at d_pos while the scope lives and
// has its own rope_input_pos (or none) back on every way out.  Nothing else of the call is undone here.
struct RopePosScope {
  Model* m; const int* saved;
  RopePosScope(Model* m_, const int* d_pos) : m(m_), saved(m_->resident.bd.rope_pos) { m->resident.bd.rope_pos = d_pos; }
  ~RopePosScope() { m->resident.bd.rope_pos = saved; }
  RopePosScope(const RopePosScope&) = delete;
};

// The store pass over the resident batch, whose rows were uploaded (rsys_rank_cache_store) or assembled on the device
// (rsys_render_request_full).  `tab` (host, [3 max_rows]) receives the rows' {slot | n_hist | 0} table and is read by a stream-ordered
// copy, as row_adapter is: both stay as they are until the stream has passed this call.  No host wait on success.
int rank_cache_store_rows(Model* m, const int32_t* row_adapter, const int32_t* n_hist, const int32_t* slot, int* tab) {
  RC(rc_check_call(m, n_hist, slot));
  const int rows = m->cur_rows;
  std::vector<char> seen((size_t)m->rc_slots, 0);
  for (int r = 0; r < rows; ++r) {
    ARG_CHECK(n_hist[r] >= 0 && n_hist[r] <= m->S, "ranking cache: n_hist must be in [0, the resident rows' length]");
    ARG_CHECK(slot[r] >= 0 && slot[r] < m->rc_slots, "ranking cache: slot outside the reserve");
    ARG_CHECK(!seen[slot[r]], "ranking cache: the slots of one store call must be distinct");
    seen[slot[r]] = 1;
  }
  HIP_CHECK(hipSetDevice(m->device));
  if (row_adapter) RC(adapter_bind_rows(m, row_adapter));
  std::fill(tab, tab + (size_t)3 * m->rows_max, 0);
  for (int r = 0; r < rows; ++r) { tab[r] = slot[r]; tab[m->rows_max + r] = n_hist[r]; }
  auto run = [&]() -> int {
    HIP_CHECK(hipMemcpyAsync(m->rc_rows, tab, (size_t)3 * m->rows_max * 4, hipMemcpyHostToDevice, m->stream));
    m->rc_mode = 1;
    RC(m->bf16_mode ? infer_trunk<bf16>(m) : infer_trunk<float>(m));
    return RSYS_OK;
  };
  const int rc = run();
  m->rc_mode = 0;
  adapter_unbind_rows(m);
  if (rc != RSYS_OK) (void)hipStreamSynchronize(m->stream);   // (the copies above read the caller's host arrays)
  // (a failed pass may have written some layers of the slots: they no longer hold a history)
  for (int r = 0; r < rows; ++r) m->rc_nhist[slot[r]] = rc == RSYS_OK ? n_hist[r] : -1;
  return rc;
}

int model_rank_cache_store(Model* m, const int32_t* row_adapter, const int32_t* n_hist, const int32_t* slot) {
  std::vector<int> tab((size_t)3 * m->rows_max);
  RC(rank_cache_store_rows(m, row_adapter, n_hist, slot, tab.data()));
  const hipError_t e = hipStreamSynchronize(m->stream);
  if (e != hipSuccess)
    for (int r = 0; r < m->cur_rows; ++r) m->rc_nhist[slot[r]] = -1;
  HIP_CHECK(e);
  return RSYS_OK;
}

static int rc_check_candidates(Model* m, const int32_t* slot, const int32_t* n_cand, int64_t* ntok) {
  RC(rc_check_call(m, slot, n_cand));
  *ntok = 0;
  for (int r = 0; r < m->cur_rows; ++r) {
    ARG_CHECK(slot[r] >= 0 && slot[r] < m->rc_slots, "ranking cache: slot outside the reserve");
    ARG_CHECK(m->rc_nhist[slot[r]] >= 0, "ranking cache: slot never stored");
    ARG_CHECK(m->rc_nhist[slot[r]] <= m->Sa - 1, "ranking cache: candidates run at position n_hist, which must stay below max_sequence_length");
    ARG_CHECK(n_cand[r] >= 1 && n_cand[r] <= m->S, "ranking cache: n_cand must be in [1, the resident rows' length]");
    *ntok += n_cand[r];
  }
  return RSYS_OK;
}

// The candidate pass over the resident batch with everything but the row table on the device: d_pos [rows][2S] the tokens' RoPE positions
// (2 n_hist, 2 n_hist + 1), d_sel [ntok] the candidates' action tokens (row 2S + 2 j + 1, rows in order), d_out [ntok] the rating-head
// values.  `tab` (host, [3 max_rows]) receives {slot | n_hist | n_cand} and is read by a stream-ordered copy, as row_adapter is.  No
// host wait on success.
int rank_cache_candidates_rows(Model* m, const int32_t* row_adapter, const int32_t* slot, const int32_t* n_cand, int* tab, int* d_pos,
                               const int* d_sel, int64_t ntok, float* d_out) {
  int64_t want = 0;
  RC(rc_check_candidates(m, slot, n_cand, &want));
  ARG_CHECK(d_pos && d_sel && d_out && ntok == want, "ranking cache: one selected token per candidate");
  const int rows = m->cur_rows;
  HIP_CHECK(hipSetDevice(m->device));
  if (row_adapter) RC(adapter_bind_rows(m, row_adapter));
  std::fill(tab, tab + (size_t)3 * m->rows_max, 0);
  for (int r = 0; r < rows; ++r) { tab[r] = slot[r]; tab[m->rows_max + r] = m->rc_nhist[slot[r]]; tab[2 * m->rows_max + r] = n_cand[r]; }
  RopePosScope pos(m, d_pos);   // (the resident batch's rope_input_pos stays what it is)
  auto run = [&]() -> int {
    HIP_CHECK(hipMemcpyAsync(m->rc_rows, tab, (size_t)3 * m->rows_max * 4, hipMemcpyHostToDevice, m->stream));
    m->rc_mode = 2;
    const float* f = nullptr;
    RC(m->bf16_mode ? infer_rows_device<bf16>(m, 1, d_sel, ntok, d_out, &f) : infer_rows_device<float>(m, 1, d_sel, ntok, d_out, &f));
    return RSYS_OK;
  };
  const int rc = run();
  m->rc_mode = 0;
  adapter_unbind_rows(m);
  if (rc != RSYS_OK) (void)hipStreamSynchronize(m->stream);
  return rc;
}

int model_rank_cache_candidates(Model* m, const int32_t* row_adapter, const int32_t* slot, const int32_t* n_cand, float* out) {
  int64_t ntok = 0;
  RC(rc_check_candidates(m, slot, n_cand, &ntok));
  ARG_CHECK(out != nullptr, "ranking cache: null output");
  const int rows = m->cur_rows, T = m->T;
  HIP_CHECK(hipSetDevice(m->device));
  std::vector<int> tab((size_t)3 * m->rows_max), pos((size_t)rows * T), sel((size_t)ntok);
  int64_t k = 0;
  for (int r = 0; r < rows; ++r) {
    const int nh = m->rc_nhist[slot[r]];
    for (int i = 0; i < m->S; ++i) { pos[(size_t)r * T + 2 * i] = 2 * nh; pos[(size_t)r * T + 2 * i + 1] = 2 * nh + 1; }   // model.py:470-476 at rope_input_pos = n_hist
    for (int j = 0; j < n_cand[r]; ++j) sel[k++] = r * T + 2 * j + 1;
  }
  // the rows' positions live in the cache's own buffer for the length of this call
  int* const d_pos = m->rc_rows + 3 * m->rows_max;
  int* const d_sel = (int*)m->gf;   // (as rsys_infer_select: room for every token of the batch)
  hipStream_t s = m->stream;
  auto run = [&]() -> int {
    HIP_CHECK(hipMemcpyAsync(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s));
    RC(rank_cache_candidates_rows(m, row_adapter, slot, n_cand, tab.data(), d_pos, d_sel, ntok, m->delta));
    HIP_CHECK(hipStreamSynchronize(s));
    return RSYS_OK;
  };
  const int rc = run();
  if (rc != RSYS_OK) { (void)hipStreamSynchronize(s); return rc; }   // (the copies above read this call's host vectors)
  HIP_CHECK(hipMemcpy(out, m->delta, (size_t)ntok * 4, hipMemcpyDeviceToHost));   // (out is written only by a call that succeeded)
  return RSYS_OK;
}

// ------------------------------------------------------------------ packed rows
// Several users per row, each in a segment of whole 64-token tiles.  The two calls below check the caller's descriptors on the host, write
// the device tables (segments, tile map, RoPE positions, selection) and run the passes above with rc_nseg set: the trunk is the same, the
// copy and the candidate attention take their per-segment / per-tile forms, the adapter bank its slot per tile (adapter_bind_tiles).
static int rc_check_packed(Model* m, int n_seg, const int32_t* seg) {
  RC(rc_check_model(m));
  ARG_CHECK(m->cfg.finetune == 0, "ranking cache, packed rows: a base model (finetune = 0)");
  ARG_CHECK(m->rcache != nullptr, "ranking cache: nothing reserved (rsys_rank_cache_reserve)");
  ARG_CHECK(m->cur_rows > 0, "no batch uploaded");
  ARG_CHECK(seg != nullptr && n_seg >= 1 && n_seg <= rc_max_seg(m), "ranking cache, packed rows: 1 <= n_seg <= max_rows x ceil(S / 32) descriptors");
  return RSYS_OK;
}
// seg_adapter [n_seg] (or null) -> the per-tile binding, every slot on the tiles `used` gives its segment
static int rc_bind_segments(Model* m, const int32_t* seg_adapter, int n_seg, const TileOwners& used) {
  if (!seg_adapter) return RSYS_OK;
  const int nta = (m->Sa + 31) / 32;
  for (int i = 0; i < n_seg; ++i) ARG_CHECK(seg_adapter[i] >= -1 && seg_adapter[i] < RSYS_ADAPTER_SLOTS, "seg_adapter entries must be in [-1, RSYS_ADAPTER_SLOTS)");
  std::vector<int32_t> tiles((size_t)m->cur_rows * nta, -1);
  for (int r = 0; r < m->cur_rows; ++r)
    for (int t = 0; t < used.nt; ++t)
      if (used.owner[(size_t)r * used.nt + t] >= 0) tiles[(size_t)r * nta + t] = seg_adapter[used.owner[(size_t)r * used.nt + t]];
  return adapter_bind_tiles(m, tiles.data());   // (range and completeness of every entry; copies the map before it returns)
}

// The packed store pass over the resident batch, whose rows were uploaded (rsys_rank_cache_store_packed) or assembled on the device
// (rsys_render_request_full under rsys_serving_pack_ranking_set).  d_pos [rows][2 row_len] (device): the tokens' RoPE positions -- event i of
// a segment at (2 i, 2 i + 1).  `seg` (host) is read by a stream-ordered copy, as the adapter map is: it stays as it is until the stream has
// passed this call.  No host wait on success.
int rank_cache_store_packed_rows(Model* m, const int32_t* seg_adapter, int n_seg, const int32_t* seg, int* d_pos) {
  RC(rc_check_packed(m, n_seg, seg));
  ARG_CHECK(d_pos != nullptr, "ranking cache, packed rows: null positions");
  TileOwners used(m->cur_rows, m->S);
  std::vector<char> seen((size_t)m->rc_slots, 0);
  for (int i = 0; i < n_seg; ++i) {
    const int row = seg[4 * i], c0 = seg[4 * i + 1], nh = seg[4 * i + 2], sl = seg[4 * i + 3];
    ARG_CHECK(nh >= 0 && nh <= m->S, "ranking cache: n_hist must be in [0, the resident rows' length]");
    RC(used.place("ranking cache, packed rows", row, c0, nh, i));
    ARG_CHECK(sl >= 0 && sl < m->rc_slots, "ranking cache: slot outside the reserve");
    ARG_CHECK(!seen[sl], "ranking cache: the slots of one store call must be distinct");
    seen[sl] = 1;
  }
  HIP_CHECK(hipSetDevice(m->device));
  RC(rc_bind_segments(m, seg_adapter, n_seg, used));
  RopePosScope pos(m, d_pos);
  auto run = [&]() -> int {
    HIP_CHECK(hipMemcpyAsync(m->rc_seg, seg, (size_t)4 * n_seg * 4, hipMemcpyHostToDevice, m->stream));
    m->rc_mode = 1; m->rc_nseg = n_seg;
    RC(m->bf16_mode ? infer_trunk<bf16>(m) : infer_trunk<float>(m));
    return RSYS_OK;
  };
  const int rc = run();
  m->rc_mode = 0; m->rc_nseg = 0;
  adapter_unbind_rows(m);
  if (rc != RSYS_OK) (void)hipStreamSynchronize(m->stream);   // (the copy above reads the caller's host array)
  // (a failed pass may have written some layers of the slots: they no longer hold a history)
  for (int i = 0; i < n_seg; ++i) m->rc_nhist[seg[4 * i + 3]] = rc == RSYS_OK ? seg[4 * i + 2] : -1;
  return rc;
}

int model_rank_cache_store_packed(Model* m, const int32_t* seg_adapter, int n_seg, const int32_t* seg) {
  RC(rc_check_packed(m, n_seg, seg));
  const int rows = m->cur_rows, T = m->T;
  // a history token runs at its position inside the segment (model.py:470-476); padding keeps the column.  (Segments that do not fit
  // their rows are refused by the body below, before the positions are read: they are only skipped here.)
  std::vector<int> pos((size_t)rows * T);
  for (int r = 0; r < rows; ++r)
    for (int t = 0; t < T; ++t) pos[(size_t)r * T + t] = t;
  for (int i = 0; i < n_seg; ++i) {
    const int row = seg[4 * i], c0 = seg[4 * i + 1], nh = seg[4 * i + 2];
    if (row < 0 || row >= rows || c0 < 0 || nh < 0 || (long long)c0 + nh > m->S) continue;
    for (int j = 0; j < 2 * nh; ++j) pos[(size_t)row * T + 2 * c0 + j] = j;
  }
  HIP_CHECK(hipSetDevice(m->device));
  int* const d_pos = m->rc_rows + 3 * m->rows_max;
  HIP_CHECK(hipMemcpyAsync(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, m->stream));
  const int rc = rank_cache_store_packed_rows(m, seg_adapter, n_seg, seg, d_pos);
  const hipError_t e = hipStreamSynchronize(m->stream);   // (also on a refusal: the copy above reads this call's vector)
  if (rc != RSYS_OK) return rc;
  if (e != hipSuccess)
    for (int i = 0; i < n_seg; ++i) m->rc_nhist[seg[4 * i + 3]] = -1;
  HIP_CHECK(e);
  return RSYS_OK;
}

int model_rank_cache_candidates_packed(Model* m, const int32_t* seg_adapter, int n_seg, const int32_t* seg, float* out) {
  RC(rc_check_packed(m, n_seg, seg));
  ARG_CHECK(out != nullptr, "ranking cache: null output");
  const int rows = m->cur_rows, T = m->T;
  TileOwners used(rows, m->S);
  int64_t ntok = 0;
  for (int i = 0; i < n_seg; ++i) {
    const int row = seg[4 * i], c0 = seg[4 * i + 1], nc = seg[4 * i + 2], sl = seg[4 * i + 3];
    ARG_CHECK(sl >= 0 && sl < m->rc_slots, "ranking cache: slot outside the reserve");
    ARG_CHECK(m->rc_nhist[sl] >= 0, "ranking cache: slot never stored");
    ARG_CHECK(m->rc_nhist[sl] <= m->Sa - 1, "ranking cache: candidates run at position n_hist, which must stay below max_sequence_length");
    ARG_CHECK(nc >= 1 && nc <= m->S, "ranking cache: n_cand must be in [1, the resident rows' length]");
    RC(used.place("ranking cache, packed rows", row, c0, nc, i));
    ntok += nc;
  }
  HIP_CHECK(hipSetDevice(m->device));
  // device tables: (slot, n_hist, first_tile, n_cand) per segment, the tile map, the positions (every token of a segment's tiles at
  // (2 n_hist, 2 n_hist + 1), as a candidate row's; padding keeps the column) and the candidates' action tokens in descriptor order
  const int max_seg = rc_max_seg(m);
  std::vector<int> tab((size_t)5 * max_seg, -1), pos((size_t)rows * T), sel((size_t)ntok);
  for (int r = 0; r < rows; ++r)
    for (int t = 0; t < T; ++t) pos[(size_t)r * T + t] = t;
  int64_t k = 0;
  for (int i = 0; i < n_seg; ++i) {
    const int row = seg[4 * i], c0 = seg[4 * i + 1], nc = seg[4 * i + 2], sl = seg[4 * i + 3], nh = m->rc_nhist[sl];
    tab[4 * i] = sl; tab[4 * i + 1] = nh; tab[4 * i + 2] = c0 / 32; tab[4 * i + 3] = nc;
    for (int c = c0; c < std::min(m->S, 32 * ((c0 + nc + 31) / 32)); ++c) { pos[(size_t)row * T + 2 * c] = 2 * nh; pos[(size_t)row * T + 2 * c + 1] = 2 * nh + 1; }
    for (int j = 0; j < nc; ++j) sel[k++] = row * T + 2 * (c0 + j) + 1;
  }
  std::copy(used.owner.begin(), used.owner.end(), tab.begin() + (size_t)4 * max_seg);
  RC(rc_bind_segments(m, seg_adapter, n_seg, used));
  int* const d_pos = m->rc_rows + 3 * m->rows_max;
  int* const d_sel = (int*)m->gf;   // (as rsys_infer_select: room for every token of the batch)
  RopePosScope rows_pos(m, d_pos);
  hipStream_t s = m->stream;
  auto run = [&]() -> int {
    HIP_CHECK(hipMemcpyAsync(m->rc_seg, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_pos, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s));
    m->rc_mode = 2; m->rc_nseg = n_seg;
    const float* f = nullptr;
    RC(m->bf16_mode ? infer_rows_device<bf16>(m, 1, d_sel, ntok, m->delta, &f) : infer_rows_device<float>(m, 1, d_sel, ntok, m->delta, &f));
    HIP_CHECK(hipStreamSynchronize(s));
    return RSYS_OK;
  };
  const int rc = run();
  m->rc_mode = 0; m->rc_nseg = 0;
  adapter_unbind_rows(m);
  if (rc != RSYS_OK) { (void)hipStreamSynchronize(s); return rc; }   // (the copies above read this call's host vectors)
  HIP_CHECK(hipMemcpy(out, m->delta, (size_t)ntok * 4, hipMemcpyDeviceToHost));   // (out is written only by a call that succeeded)
  return RSYS_OK;
}

int model_rank_cache_get(Model* m, int layer, int slot, void* out, int64_t bytes) {
  ARG_CHECK(m->rcache != nullptr, "ranking cache: nothing reserved");
  ARG_CHECK(layer >= 0 && layer < m->L && slot >= 0 && slot < m->rc_slots && out != nullptr, "ranking cache: layer or slot out of range");
  ARG_CHECK(m->rc_nhist[slot] >= 0, "ranking cache: slot never stored");
  const size_t want = (size_t)2 * m->rc_nhist[slot] * rc_kvw(m) * m->esz;
  ARG_CHECK(bytes == (int64_t)want, "ranking cache: out holds [2 n_hist][2 KV hd] values of the compute dtype");
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  const unsigned char* src = (const unsigned char*)m->rcache + ((size_t)layer * rc_layer_elems(m) + (size_t)slot * m->Ta * rc_kvw(m)) * m->esz;
  if (want) HIP_CHECK(hipMemcpy(out, src, want, hipMemcpyDeviceToHost));
  return RSYS_OK;
}

}  // namespace rsys
