// A page from raw histories in one device pipeline (Inference/compute.jl:512-531 + render.jl:437-474): the retrieval forward, `retrieval(state)`,
// the page window, the ranking forward and `ranking` + `reranking!` chained on the device for states of both media.  In: histories (as
// inference rows and as list items), selected items, penalties, pagination.  Out: the pages' ids and the totals.  User embeddings,
// retrieved candidates and rating-head values never leave the device; the per-group counts do (they size the ranking rows).
// One request is one Render context run through these stages by model_render (DESIGN.md sections 4u, 4w):
//   render_check          the arguments, before anything is enqueued; full: the K/V cache's reserve
//   render_carve          the call's device arrays inside RenderState::ws
//   retrieval_forward     the users' rows in waves of <= max_rows (media mixed, one adapter slot per row); the trunk output at each
//                         user's query token goes to the query buffer Q [n_users][D] fp32; full: the rows' history columns stay on the device
//                         (rsys_serving_pack_set: retrieval_forward_packed instead -- several users per row, one adapter slot per tile)
//   retrieve_and_window   per medium the body of rsys_retrieve_request on the medium's rows of Q (gathered in user order), then
//                         render.jl:447-465 on the host from the counts; window_kernel copies each group's slice to the candidate list
//   plan_ranking          the ranking rows of every group with a page, as row descriptors: split rows (user x chunk of <= S - S/2
//                         candidates behind the user's prefix); full: a user with a history is ranked through the cache instead
//   rank_cached_waves     full: per wave of <= max_rows users with a history one store forward (rc_mode = 1, slot = the user's place in the
//                         wave) over their history columns, then their candidate rows (<= S candidates each) in rank_waves of <= max_rows rows
//   rank_assembled_waves  the split rows in rank_waves of <= max_rows rows (full: the empty histories' rows, in waves of their own)
//   rank_and_rerank       per medium the body of rsys_rank_request on device candidates, queries and r_masked; the page's ids come back
//   write_outputs         the caller's arrays, once everything has succeeded
// Every batch a ranking forward reads is filled by rows_kernel from row descriptors (RowDesc), one workgroup per row, one launch per wave;
// rank_wave is the one forward over such rows: rating head at the candidates' action tokens, rank_scatter_kernel puts the values into the
// ragged r_masked layout of rsys_rank_request.
// rsys_render_items (model_render_items) is the same page for states without users: no forward, the windowed
// retrieval of rsys_retrieve_window on the prior alone, window_kernel, then the reranking of rsys_rank_request on zeros.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <map>

#include "model_internal.hpp"

namespace rsys {

namespace {

constexpr int RN_THREADS = 256;
constexpr int RN_MAXQ = 4096;           // users per call (the limit of the two request bodies)
constexpr int RN_MAX_RANK = 1024;       // render.jl:449 max_items_to_rank
constexpr int RN_CAP = 8192;            // candidates a retrieval returns at most

// Where the history columns of a row come from: per-user rows [n_users][stride] on the device.  tmid / rope are null for the kept
// retrieval rows (rsys_render_request_full): mask id 0, position = column.
struct HistSrc {
  double* time;
  int *userid, *tmid, *gender, *source, *matchedid, *status, *rope;
  float *rating, *progress;
  int stride;
};

// One row of a batch assembled on the device.  Columns [0, ncopy) are columns [0, ncopy) of the history source's row `user`; columns
// [ncopy, ncopy + ncand) are the candidates cand[cand0 + c] + moff (serve.build_batch's tail: time = ts, status -1, rating = progress = 0,
// the descriptor's userid / gender / source) with mask id mask0 + c (mask0 < 0: mask id 0) at RoPE position cpos; the other columns are
// zero, at RoPE position fill_pos.
//                   ncopy    ncand        mask0   cpos     fill_pos   source
//   split row       nh       <= S - S/2   nh      nh       0          uploaded prefix, stride P
//   store row       n_hist   0            -       -        0          kept retrieval rows, stride S
//   candidate row   0        <= S         -1      n_hist   n_hist     -
struct RowDesc {
  int user, med, userid, gender, source;
  int moff;          // added to a candidate id: V_0 for medium 1
  int cand0, ncand;
  int ncopy, mask0, cpos, fill_pos;
  int sel0;          // first slot of the row's action tokens in the wave's selection (and in its rating-head output)
  int rm0;           // first slot of the row's values in r_masked
  double ts;         // the user's timestamp: `time` of every candidate token
};

struct Win { int src, n, dst; };

// row blockIdx.x of the wave from its descriptor: all ten arrays, the per-token RoPE positions (2 p, 2 p + 1) as rsys_batch_upload derives
// them, and candidate c's action token r 2S + 2 (ncopy + c) + 1 at sel[sel0 + c].  S is the wave's row length (the model's S, or the trimmed one)
__global__ void __launch_bounds__(RN_THREADS) rows_kernel(const RowDesc* rows, HistSrc h, int S, const int32_t* cand, BatchDevRows out, int* sel) {
  const int r = blockIdx.x;
  const RowDesc d = rows[r];
  for (int j = threadIdx.x; j < S; j += RN_THREADS) {
    const long long i = (long long)r * S + j;
    double time = 0.0;
    int userid = 0, tmid = 0, gender = 0, source = 0, matchedid = 0, status = 0, p = d.fill_pos;
    float rating = 0.f, progress = 0.f;
    if (j < d.ncopy) {
      const long long q = (long long)d.user * h.stride + j;
      time = h.time[q]; userid = h.userid[q]; gender = h.gender[q]; source = h.source[q];
      matchedid = h.matchedid[q]; status = h.status[q]; rating = h.rating[q]; progress = h.progress[q];
      tmid = h.tmid ? h.tmid[q] : 0; p = h.rope ? h.rope[q] : j;
    } else if (j < d.ncopy + d.ncand) {
      const int c = j - d.ncopy;
      time = d.ts; userid = d.userid; gender = d.gender; source = d.source;
      matchedid = cand[d.cand0 + c] + d.moff; status = -1; p = d.cpos; tmid = d.mask0 < 0 ? 0 : d.mask0 + c;
      sel[d.sel0 + c] = r * 2 * S + 2 * j + 1;
    }
    out.time[i] = time; out.userid[i] = userid; out.tmid[i] = tmid; out.gender[i] = gender; out.source[i] = source;
    out.matchedid[i] = matchedid; out.status[i] = status; out.rating[i] = rating; out.progress[i] = progress;
    ((int2*)out.rope_pos)[i] = make_int2(2 * p, 2 * p + 1);
  }
}

// the rating-head values of row blockIdx.x (wave order) to its user's slice of r_masked (user order, chunks concatenated)
__global__ void __launch_bounds__(RN_THREADS) rank_scatter_kernel(const RowDesc* rows, const float* pred, float* rm) {
  const RowDesc d = rows[blockIdx.x];
  for (int c = threadIdx.x; c < d.ncand; c += RN_THREADS) rm[d.rm0 + c] = pred[d.sel0 + c];
}

// the page's slice of group blockIdx.x's retrieved ids to the candidate list
__global__ void __launch_bounds__(RN_THREADS) window_kernel(const Win* w, const int32_t* ids, int32_t* cand) {
  const Win d = w[blockIdx.x];
  for (int i = threadIdx.x; i < d.n; i += RN_THREADS) cand[d.dst + i] = ids[d.src + i];
}

// Packed retrieval rows (rsys_serving_pack_set): user d.user's segment -- columns [col0, col0 + cols) of row d.row of the
// resident batch (rows of S columns) -- to columns [0, cols) of its kept history row (stride h.stride), the eight arrays a store row reads.
// userid: the caller's value, not the segment's number inside the forward.  One workgroup per user of the wave.
struct SegDesc { int user, row, col0, cols, userid; };
struct SegSrc { const double* time; const int *userid, *gender, *source, *matchedid, *status; const float *rating, *progress; };
__global__ void __launch_bounds__(RN_THREADS) unpack_rows_kernel(const SegDesc* segs, SegSrc b, int S, HistSrc h) {
  const SegDesc d = segs[blockIdx.x];
  for (int j = threadIdx.x; j < d.cols; j += RN_THREADS) {
    const long long i = (long long)d.row * S + d.col0 + j, q = (long long)d.user * h.stride + j;
    h.time[q] = b.time[i]; h.userid[q] = b.userid[i] != 0 ? d.userid : 0; h.gender[q] = b.gender[i]; h.source[q] = b.source[i];
    h.matchedid[q] = b.matchedid[i]; h.status[q] = b.status[i]; h.rating[q] = b.rating[i]; h.progress[q] = b.progress[i];
  }
}

// Packed store rows (rsys_serving_pack_ranking_set): row blockIdx.x of the resident batch from the segments that lie in it --
// columns [col0, col0 + cols) are columns [0, cols) of user d.user's kept history row, with mask id 0, RoPE position = the column inside
// the segment and userid d.userid (1 + the segment's place in the forward); every other column is zero.  The inverse of unpack_rows_kernel.
__global__ void __launch_bounds__(RN_THREADS) pack_store_rows_kernel(const SegDesc* segs, int n_seg, HistSrc h, int S, BatchDevRows out) {
  const int r = blockIdx.x;
  for (int j = threadIdx.x; j < S; j += RN_THREADS) {
    const long long i = (long long)r * S + j;
    double time = 0.0;
    int userid = 0, gender = 0, source = 0, matchedid = 0, status = 0, p = 0;
    float rating = 0.f, progress = 0.f;
    for (int k = 0; k < n_seg; ++k) {
      const SegDesc d = segs[k];
      if (d.row != r || j < d.col0 || j >= d.col0 + d.cols) continue;
      const long long q = (long long)d.user * h.stride + (j - d.col0);
      time = h.time[q]; userid = d.userid; gender = h.gender[q]; source = h.source[q];
      matchedid = h.matchedid[q]; status = h.status[q]; rating = h.rating[q]; progress = h.progress[q];
      p = j - d.col0;
      break;
    }
    out.time[i] = time; out.userid[i] = userid; out.tmid[i] = 0; out.gender[i] = gender; out.source[i] = source;
    out.matchedid[i] = matchedid; out.status[i] = status; out.rating[i] = rating; out.progress[i] = progress;
    ((int2*)out.rope_pos)[i] = make_int2(2 * p, 2 * p + 1);
  }
}

#define RN_LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

// render.jl:447-465 for one group (serve.page_window, clamp included): false when the page starts past the list
bool page_window(int n, int64_t offset, int limit, int* start, int* stop, int* sidx, int* eidx) {
  const int mitr = RN_MAX_RANK - RN_MAX_RANK % limit;
  const int64_t s1 = offset + 1;
  if (s1 > n) return false;
  const int64_t e1 = std::min<int64_t>(offset + limit, n);
  const int64_t page = (s1 - 1) / mitr;
  *start = (int)(page * mitr);
  *stop = (int)std::min<int64_t>((page + 1) * mitr, n);
  *sidx = (int)(s1 - *start);
  *eidx = (int)(e1 - *start);
  return true;
}

// (debug channel) the ten arrays of a device-assembled batch: key suffix, device array, bytes per value, values per token
struct KeptCol { const char* suffix; const void* src; int size, per; };
std::array<KeptCol, 10> kept_cols(const BatchDevRows& b) {
  return {{{".time", b.time, 8, 1}, {".userid", b.userid, 4, 1}, {".token_mask_ids", b.tmid, 4, 1}, {".gender", b.gender, 4, 1},
           {".source", b.source, 4, 1}, {".matchedid", b.matchedid, 4, 1}, {".status", b.status, 4, 1}, {".rating", b.rating, 4, 1},
           {".progress", b.progress, 4, 1}, {".rope_input_pos", b.rope_pos, 4, 2}}};
}
// the batches a call may keep, each with the key that goes with its rows: rsys_render_request keeps the first, _full all three
constexpr const char* KEPT_BATCHES[3][2] = {{"batch", "token_index"}, {"store", "store.rows"}, {"cand", "cand.token_index"}};

}  // namespace

struct RenderState {
  DevScratch ws;
  bool keep = false;                                   // rsys_render_debug_keep: the next calls keep their intermediates
  int forwards[2] = {0, 0};                            // forwards of the last call: retrieval, ranking
  int forwards_full[3] = {0, 0, 0};                    // rsys_render_request_full's ranking forwards: store, candidates, empty-history chunks
  std::vector<int32_t> forward_rows;                   // (stage, rows, row_len) of every forward of the last call, run order: stage 0 retrieval, 1 store, 2 cached candidates, 3 assembled
  void note_forward(int stage, int rows, int row_len) { forward_rows.push_back(stage); forward_rows.push_back(rows); forward_rows.push_back(row_len); }
  std::vector<int32_t> forward_top;                    // (infer.top, infer.top_rows) of every forward of the last call, in the order of forward_rows (Model::top_log)
  std::map<std::string, std::vector<unsigned char>> kept;
  void begin() {   // a call starts
    forwards[0] = forwards[1] = 0;
    forwards_full[0] = forwards_full[1] = forwards_full[2] = 0;
    forward_rows.clear();
    forward_top.clear();
    kept.clear();
  }
  void put_bytes(const std::string& key, const void* p, size_t n) {
    std::vector<unsigned char>& v = kept[key];
    const size_t at = v.size();
    v.resize(at + n);
    if (n) memcpy(v.data() + at, p, n);
  }
  template <typename X> void put(const char* key, const X* p, size_t n) { put_bytes(key, p, n * sizeof(X)); }
  // the ten arrays of the nr device-assembled rows under "<name>.*", as [nr][S]: rows of rl < S interactions (a trimmed forward) are
  // widened with what the untrimmed rows hold there: zeros, and the row's fill position fill_pos[r] as rope_input_pos
  int keep_rows(const std::string& name, const BatchDevRows& bd, int nr, int S, int rl, const std::vector<int>& fill_pos) {
    const size_t N = (size_t)nr * rl;
    std::vector<int64_t> h(N), wide((size_t)nr * S);
    for (const KeptCol& c : kept_cols(bd)) {
      HIP_CHECK(hipMemcpy(h.data(), c.src, N * c.size * c.per, hipMemcpyDeviceToHost));
      int32_t* hi = (int32_t*)h.data();
      for (size_t i = 0; i < N && c.per == 2; ++i) hi[i] = hi[2 * i] / 2;   // (the per-token positions 2 p, 2 p + 1 back to rope_input_pos)
      if (rl == S) { put_bytes(name + c.suffix, h.data(), N * c.size); continue; }
      std::fill(wide.begin(), wide.end(), 0);
      for (int r = 0; r < nr && c.per == 2; ++r) std::fill((int32_t*)wide.data() + (size_t)r * S + rl, (int32_t*)wide.data() + (size_t)(r + 1) * S, fill_pos[r]);
      for (int r = 0; r < nr; ++r)
        memcpy((unsigned char*)wide.data() + (size_t)r * S * c.size, (const unsigned char*)h.data() + (size_t)r * rl * c.size, (size_t)rl * c.size);
      put_bytes(name + c.suffix, wide.data(), (size_t)nr * S * c.size);
    }
    return RSYS_OK;
  }
  void complete_keys(int batches) {   // every key is present, maybe empty: the first `batches` of KEPT_BATCHES
    for (const char* k : {"rows", "groups", "rm_users", "r", "picks", "r_masked"}) kept[k];
    for (int b = 0; b < batches; ++b) {
      for (const KeptCol& c : kept_cols(BatchDevRows{})) kept[std::string(KEPT_BATCHES[b][0]) + c.suffix];
      kept[KEPT_BATCHES[b][1]];
    }
  }
};

static RenderState* render_state(Model* m) {
  if (!m->render) m->render = new RenderState();
  return m->render;
}

void render_free(Model* m) {
  if (!m->render) return;
  m->render->ws.release();
  delete m->render;
  m->render = nullptr;
}

int render_debug_keep(Model* m, int on) {
  RenderState* R = render_state(m);
  R->keep = on != 0;
  if (!on) R->kept.clear();
  return RSYS_OK;
}

int render_debug_get(Model* m, const char* key, void* out, int64_t cap, int64_t* bytes) {
  ARG_CHECK(key && bytes, "render_debug_get: null key or size");
  RenderState* R = render_state(m);
  if (std::string(key) == "forwards") {
    *bytes = 8;
    if (out && cap >= 8) memcpy(out, R->forwards, 8);
    return RSYS_OK;
  }
  if (std::string(key) == "forward_rows") {
    *bytes = (int64_t)R->forward_rows.size() * 4;
    if (out && cap >= *bytes && *bytes) memcpy(out, R->forward_rows.data(), (size_t)*bytes);
    return RSYS_OK;
  }
  if (std::string(key) == "forward_top") {
    *bytes = (int64_t)R->forward_top.size() * 4;
    if (out && cap >= *bytes && *bytes) memcpy(out, R->forward_top.data(), (size_t)*bytes);
    return RSYS_OK;
  }
  if (std::string(key) == "forwards.full") {
    *bytes = 12;
    if (out && cap >= 12) memcpy(out, R->forwards_full, 12);
    return RSYS_OK;
  }
  auto it = R->kept.find(key);
  ARG_CHECK(it != R->kept.end(), std::string("render_debug_get: nothing kept under \"") + key + "\" (rsys_render_debug_keep, then a request)");
  *bytes = (int64_t)it->second.size();
  if (out && cap >= *bytes && *bytes) memcpy(out, it->second.data(), (size_t)*bytes);
  return RSYS_OK;
}

namespace {

// The list items / selected items of a subset of a request's users / groups, in subset order: the list value an inner call is handed.
// The vectors own its arrays, so a SubCsr outlives the inner call's stream-ordered copies.  An absent outer list gives an absent
// subset (all null); a given one gives non-null pointers even when the subset holds no item (one padding element per array).
struct SubCsr {
  const bool given;
  std::vector<int64_t> off;
  std::vector<int32_t> medium, ids, status;
  SubCsr(const std::vector<int>& rows, const SelectedList& l) : SubCsr(rows, HistoryList{l.off, l.medium, l.ids, nullptr}) {}
  SubCsr(const std::vector<int>& rows, const HistoryList& l) : given(l.off != nullptr) {
    if (!given) return;
    off.assign(1, 0);
    for (int r : rows) {
      for (int64_t j = l.off[r]; j < l.off[r + 1]; ++j) {
        medium.push_back(l.medium[j]); ids.push_back(l.ids[j]);
        if (l.status) status.push_back(l.status[j]);
      }
      off.push_back((int64_t)medium.size());
    }
    if (medium.empty()) { medium.push_back(0); ids.push_back(0); }
    if (status.empty()) status.push_back(0);
  }
  HistoryList history() const { return given ? HistoryList{off.data(), medium.data(), ids.data(), status.data()} : HistoryList{}; }
  SelectedList selected() const { return given ? SelectedList{off.data(), medium.data(), ids.data()} : SelectedList{}; }
};
// the query weights (rsys_query_weights_set) of a subset of a request, in subset order: per user, and per selected item of a subset of
// groups.  w == nullptr: unweighted, `out` stays empty and the slice is null.
const float* sub_weights(const std::vector<int>& users, const float* w, std::vector<float>& out) {
  if (!w) return nullptr;
  out.clear();
  out.reserve(users.size() + 1);   // (a non-null pointer for an empty subset too)
  for (int u : users) out.push_back(w[u]);
  return out.data();
}
const float* sub_sel_weights(const std::vector<int>& groups, const int64_t* off, const float* w, std::vector<float>& out) {
  if (!w || !off) return nullptr;
  out.clear();
  out.reserve(1);
  for (int g : groups) out.insert(out.end(), w + off[g], w + off[g + 1]);
  return out.data();
}

// the text queries (rsys_query_texts_set) of a subset of a request's groups, in text order: local[g] = the group's index in the inner call,
// or -1 for a group the call does not hold.  No text left: n == 0, and the inner call launches what it always has.
struct SubTexts { std::vector<int32_t> row, group; };
QueryTexts sub_texts(const QueryTexts& qt, const std::vector<int>& local, SubTexts& out) {
  out.row.clear(); out.group.clear();
  for (int i = 0; i < qt.n; ++i) {
    const int l = local[qt.group[i]];
    if (l < 0) continue;
    out.row.push_back(qt.row[i]); out.group.push_back(l);
  }
  QueryTexts r = qt;
  r.n = (int)out.row.size(); r.row = out.row.data(); r.group = out.group.data();
  return r;
}

// a group with a page: its slice [c0, c0 + n) of the candidate list, the page = picks [sidx - 1, eidx) of it
struct Active { int g, c0, n, sidx, eidx; };

// the two forwards a rank_wave runs: the K/V cache's candidate pass, or the plain forward over rows that carry their history.  The
// value is the last field of the rows' 7-field record; their assembly's timer label, the keys of their kept rows and token indices
enum WaveKind { WAVE_CACHED = 0, WAVE_ASSEMBLED = 1 };
constexpr const char* WAVE_KEYS[2][3] = {{"render_cand_rows", "cand", "cand.token_index"}, {"render_rank_rows", "batch", "token_index"}};

// One request: the arguments, the call's device arrays, the host plan and the stages over them.  Host tables that a stream-ordered copy
// reads live here, so that they outlive a stage that fails: model_render waits for the stream before the context goes.
struct Render : RenderArgs {
  Model* const m;
  const int S, D, chunk, RM;
  RenderState* R = nullptr;
  hipStream_t s = nullptr;
  bool keep = false;
  // device (render_carve)
  float *Q, *Qs, *pred, *rm; int *d_sel, *d_order; int32_t* cand; RowDesc *d_rows, *d_store; Win* d_win; SegDesc* d_segs;
  HistSrc hist;                                  // the ranking prefixes as uploaded; full: the history columns of the retrieval rows
  // host plan: users and groups by medium, the groups with a page, the r_masked layout, the ranking rows, the result
  std::vector<int> users_m[2], groups_m[2], gloc;
  std::vector<Active> act_m[2];
  std::vector<int> gact;                         // group -> index in its medium's active list
  std::vector<int> ausers_m[2];                  // users of active groups, user order
  std::vector<int64_t> rm_off;
  int64_t rm_n[2] = {0, 0}, rm_base[2] = {0, 0};
  std::vector<RowDesc> rows;                     // the split rows (full: of the users with an empty history only)
  std::vector<RowDesc> cached;                   // full: per user ranked through the cache its whole window as one candidate row, r_masked order
  std::vector<int32_t> total;
  std::vector<std::vector<int32_t>> pages;
  // host tables of a wave, read by stream-ordered copies: the retrieval waves' tokens, a wave's adapter slots and candidate counts, the
  // store forward's rows (s_*, sd) and the candidate rows of a cached wave with their cache slots
  struct WaveTabs {
    std::vector<int32_t> tok, ra, nc, s_nh, s_slot, s_ad, crow_slot, tiles, place;
    std::vector<SegDesc> segs;
    std::vector<int> s_tab, c_tab;
    std::vector<RowDesc> sd, crows;
  } t;

  ~Render() { m->top_log = nullptr; }
  Render(Model* model, const RenderArgs& a) : RenderArgs(a), m(model), S(m->Sa), D(m->D), chunk(S - S / 2), RM(m->rows_max), trim(m->serving_trim), pack(m->serving_pack), pack_rank(m->serving_pack_ranking) {}

  // rsys_serving_trim_set: a forward whose longest row has `live` live columns runs at this row length -- whole 64-token attention tiles,
  // clamped to S (serve.trim_length); off: S.  Chunking, waves and slots are planned on S either way.
  const bool trim;
  const bool pack;   // rsys_serving_pack_set: the retrieval stage runs several users per row (retrieval_forward_packed)
  const bool pack_rank;   // rsys_serving_pack_ranking_set (full only): the K/V-cache store rows hold several users (rank_cached_waves_packed)
  int row_len_for(int live) const { return trim ? std::min(S, (std::max(live, 1) + 31) / 32 * 32) : S; }

  // ---- arguments.  Checked here, before anything is enqueued: the request's shape, pagination, groups, offsets' monotonicity, adapter
  // slots, descriptors and prefixes.  Checked later, by the code that owns them: the retrieval rows (rsys_batch_upload's checks, wave by
  // wave) and the ids of list and selected items and the tables they need (the request bodies) -- by then the retrieval forward may have
  // run and the resident batch is replaced.  In every case the outputs are written only after the last stage has succeeded.
  // full == false: pb / P are the ranking prefixes; full == true: pb == nullptr, P == 0, user_desc[u][0] = n_hist = the history columns
  // of retrieval row u.
  int render_check() {
    ARG_CHECK(!m->fp8, "render_request: fp32 and bf16 models only (the adapter bank's dtypes)");
    ARG_CHECK(!m->sharded, "render_request: the row-sharded item table is not supported (replicated table only)");
    ARG_CHECK(ng >= 1 && nu >= 1 && nu <= RN_MAXQ && ng <= nu, "render_request: 1 <= n_groups <= n_users <= 4096 (every group needs a user)");
    ARG_CHECK(group_medium && offset && limit && penalties && group && rb && retrieval_token && (pb || full) && user_desc && user_ts && ids_out &&
                  ids_offsets && total_out,
              "render_request: null argument");
    RC(check_ragged("render_request", hist_list, nu));
    RC(check_ragged("render_request", sel_list, ng));
    ARG_CHECK(coef_have == nullptr || coefs != nullptr, "render_request: coef_have needs coefs");
    int64_t need_ids = 0;
    for (int g = 0; g < ng; ++g) {
      ARG_CHECK(group_medium[g] == 0 || group_medium[g] == 1, "render_request: medium must be 0 or 1");
      ARG_CHECK(limit[g] >= 1 && limit[g] <= RN_MAX_RANK, "render_request: 1 <= limit <= 1024");
      ARG_CHECK(offset[g] >= 0, "render_request: offset >= 0");
      need_ids += limit[g];
    }
    ARG_CHECK(ids_cap >= need_ids, "render_request: ids_out must hold the sum of the limits");
    std::vector<int> members(ng, 0);
    for (int64_t u = 0; u < nu; ++u) {
      ARG_CHECK(group[u] >= 0 && group[u] < ng, "render_request: group ids must be in [0, n_groups)");
      ++members[group[u]];
    }
    for (int g = 0; g < ng; ++g) ARG_CHECK(members[g] > 0, "render_request: every group needs at least one user");
    if (slots) {
      int32_t mask = 0;
      RC(adapter_slots(m, &mask));
      for (int i = 0; i < 4; ++i) {
        ARG_CHECK(slots[i] >= -1 && slots[i] < RSYS_ADAPTER_SLOTS, "render_request: adapter slots must be in [-1, RSYS_ADAPTER_SLOTS)");
        ARG_CHECK(slots[i] < 0 || ((mask >> slots[i]) & 1), "render_request: an adapter slot is not complete");
      }
    }
    ARG_CHECK(rb->rows == nu && (full || pb->rows == nu), "render_request: the retrieval rows and the ranking prefixes hold one row per user");
    ARG_CHECK(rb->userid && rb->token_mask_ids && rb->gender && rb->source && rb->matchedid && rb->status && rb->time && rb->rating &&
                  rb->progress && rb->rope_input_pos,
              "render_request: the retrieval rows need the ten inference arrays");
    ARG_CHECK(P >= 0 && P <= S, "render_request: 0 <= prefix_stride <= max_sequence_length");
    ARG_CHECK(full || P == 0 || (pb->userid && pb->token_mask_ids && pb->gender && pb->source && pb->matchedid && pb->status && pb->time && pb->rating &&
                         pb->progress && pb->rope_input_pos),
              "render_request: the ranking prefixes need the ten inference arrays");
    for (int64_t u = 0; u < nu; ++u) {
      const int32_t* d = user_desc + 4 * u;
      ARG_CHECK(retrieval_token[u] >= 0 && retrieval_token[u] < 2 * S, "render_request: retrieval_token must be in [0, 2 S)");
      if (full) ARG_CHECK(d[0] >= 0 && d[0] <= S - 1, "render_request: n_hist must be in [0, max_sequence_length - 1]");
      else ARG_CHECK(d[0] >= 0 && d[0] <= P && d[0] <= S - chunk, "render_request: a prefix length must be in [0, min(prefix_stride, S / 2)]");
      ARG_CHECK(d[1] >= 0 && d[1] < (1 << 19), "render_request: userid must be in [0, 2^19)");
      ARG_CHECK(d[2] >= -1 && d[2] <= m->cfg.vocab_gender, "render_request: gender out of range");
      ARG_CHECK(d[3] >= -1 && d[3] <= m->cfg.vocab_source, "render_request: source out of range");
      for (int j = 0; j < d[0] && !full; ++j) {   // the checks rsys_batch_upload makes on a host batch (full: the retrieval rows' own)
        const int64_t q = u * P + j;
        ARG_CHECK(pb->matchedid[q] >= -1 && pb->matchedid[q] < m->V, "render_request: prefix matchedid out of range");
        ARG_CHECK(pb->userid[q] >= 0 && pb->userid[q] < (1 << 19), "render_request: prefix userid must be in [0, 2^19)");
        ARG_CHECK(pb->token_mask_ids[q] >= 0 && pb->token_mask_ids[q] < 4096, "render_request: prefix token_mask_ids must be in [0, 4096)");
        ARG_CHECK(pb->status[q] >= -1 && pb->status[q] <= m->cfg.vocab_status, "render_request: prefix status out of range");
        ARG_CHECK(pb->gender[q] >= -1 && pb->gender[q] <= m->cfg.vocab_gender, "render_request: prefix gender out of range");
        ARG_CHECK(pb->source[q] >= -1 && pb->source[q] <= m->cfg.vocab_source, "render_request: prefix source out of range");
        ARG_CHECK(pb->rope_input_pos[q] >= 0 && 2 * pb->rope_input_pos[q] + 1 < m->Ta, "render_request: prefix rope_input_pos out of range");
      }
    }
    ARG_CHECK(S / 2 + chunk <= 4096, "render_request: max_sequence_length <= 4096 (token_mask_ids of the candidates)");
    if (full) {   // the cache: the model's reserve when it holds a wave's users, else max_rows slots (RSYS_ERR_STATE when they do not fit)
      int with_hist = 0;
      for (int64_t u = 0; u < nu; ++u) with_hist += user_desc[4 * u] >= 1;
      if (m->rc_slots < std::min(RM, with_hist)) RC(model_rank_cache_reserve(m, RM));
    }
    R = render_state(m);
    R->begin();
    m->top_log = &R->forward_top;   // every trunk forward of this call notes what its last layer did (cleared by ~Render)
    keep = R->keep;
    return RSYS_OK;
  }

  int render_carve() {
    const size_t sel_cap = (size_t)RM * (full ? S : std::max(chunk, 1));   // (a candidate row of the cached path holds up to S candidates)
    hist.stride = full ? S : P;
    const size_t n_hist = (size_t)nu * hist.stride;
    t.tok.resize(RM); t.ra.resize(RM); t.nc.resize(RM);   // (the waves' host tables)
    return carve_into(R->ws, s, [&](Carve& c) {
      Q = c.take<float>((size_t)nu * D); Qs = c.take<float>((size_t)nu * D);
      pred = c.take<float>(sel_cap); rm = c.take<float>((size_t)nu * RN_MAX_RANK);
      d_sel = c.take<int>(sel_cap); d_order = c.take<int>(nu);
      cand = c.take<int32_t>((size_t)ng * RN_MAX_RANK);
      d_rows = c.take<RowDesc>(RM); d_store = c.take<RowDesc>(full ? RM : 0); d_win = c.take<Win>(ng);
      d_segs = c.take<SegDesc>((pack || pack_rank) && full ? (size_t)RM * ((S + 31) / 32) : 0);
      hist.time = c.take<double>(n_hist);
      hist.userid = c.take<int>(n_hist); hist.gender = c.take<int>(n_hist); hist.source = c.take<int>(n_hist);
      hist.matchedid = c.take<int>(n_hist); hist.status = c.take<int>(n_hist);
      hist.rating = c.take<float>(n_hist); hist.progress = c.take<float>(n_hist);
      hist.tmid = full ? nullptr : c.take<int>(n_hist); hist.rope = full ? nullptr : c.take<int>(n_hist);
    });
  }

  // ---- 1. retrieval forward: waves of <= max_rows users in user order, media mixed
  int retrieval_forward() {
    const std::vector<float> zf((size_t)RM * S, 0.f);
    const std::vector<int32_t> zi((size_t)RM * S, 0);
    for (int64_t u0 = 0; u0 < nu; u0 += RM) {
      const int nr = (int)std::min<int64_t>(RM, nu - u0);
      const size_t o = (size_t)u0 * S;
      rsys_batch b{};
      b.rows = nr;
      b.userid = rb->userid + o; b.token_mask_ids = rb->token_mask_ids + o; b.gender = rb->gender + o; b.source = rb->source + o;
      b.matchedid = rb->matchedid + o; b.status = rb->status + o; b.time = rb->time + o; b.rating = rb->rating + o; b.progress = rb->progress + o;
      b.rope_input_pos = rb->rope_input_pos + o;
      for (int k = 0; k < 6; ++k) { b.label[k] = zf.data(); b.weight[k] = zf.data(); b.position[k] = zi.data(); }
      int live = 1;   // the wave's longest live row: the last column with a user, and the query token's column
      for (int r = 0; r < nr && trim; ++r) {
        live = std::max(live, retrieval_token[u0 + r] / 2 + 1);
        if (full) live = std::max(live, user_desc[4 * (u0 + r)] + 1);   // (the store rows read n_hist columns of the kept row: all of them are copied below, whatever the caller's rows hold there)
        int j = S;
        while (j > live && b.userid[(size_t)r * S + j - 1] == 0) --j;
        live = std::max(live, j);
      }
      const int rl = row_len_for(live);
      RC(rl == S ? model_batch_upload(m, &b) : model_batch_upload_trimmed(m, &b, rl));
      R->note_forward(0, nr, rl);
      if (full) {   // the rows' history columns stay on the device: the store rows are cut from them, nothing of a history is uploaded twice
        const BatchDev& bd = m->resident.bd;   // (rows of rl columns; the kept rows keep the stride S, their columns behind rl are never read: n_hist < rl by the choice of rl above)
        auto keep_cols = [&](void* dst, const void* src, size_t esz) {
          if (rl == S) return hipMemcpyAsync(dst, src, (size_t)nr * S * esz, hipMemcpyDeviceToDevice, s);   // (full rows: one contiguous copy)
          return hipMemcpy2DAsync(dst, (size_t)S * esz, src, (size_t)rl * esz, (size_t)rl * esz, (size_t)nr, hipMemcpyDeviceToDevice, s);
        };
        HIP_CHECK(keep_cols(hist.time + o, bd.time, 8));
        const int* src_i[5] = {bd.userid, bd.gender, bd.source, bd.matchedid, bd.status};
        int* dst_i[5] = {hist.userid, hist.gender, hist.source, hist.matchedid, hist.status};
        for (int k = 0; k < 5; ++k) HIP_CHECK(keep_cols(dst_i[k] + o, src_i[k], 4));
        HIP_CHECK(keep_cols(hist.rating + o, bd.rating, 4));
        HIP_CHECK(keep_cols(hist.progress + o, bd.progress, 4));
      }
      for (int r = 0; r < nr; ++r) {
        t.tok[r] = r * 2 * rl + retrieval_token[u0 + r];
        t.ra[r] = slots ? slots[2 * group_medium[group[u0 + r]]] : -1;
      }
      HIP_CHECK(hipMemcpyAsync(d_sel, t.tok.data(), (size_t)nr * 4, hipMemcpyHostToDevice, s));
      RC(model_infer_device(m, 0, slots ? t.ra.data() : nullptr, d_sel, nr, Q + (size_t)u0 * D));
      HIP_CHECK(hipStreamSynchronize(s));   // (t.tok / t.ra are rewritten by the next wave)
      ++R->forwards[0];
    }
    if (keep) {
      std::vector<float> h((size_t)nu * D);
      HIP_CHECK(hipMemcpy(h.data(), Q, h.size() * 4, hipMemcpyDeviceToHost));
      R->put("queries", h.data(), h.size());
    }
    return RSYS_OK;
  }

  // ---- 1. (rsys_serving_pack_set) the same stage with several users per row, serve.pack_plan's layout: user u's live columns -- through
  // its query token, its last column with a userid and (full) its n_hist columns -- become a segment that starts on a 32-column boundary
  // of a row; first-fit decreasing over the users, ties in user order; forwards of <= max_rows rows at the trim length of their fullest
  // row, whatever rsys_serving_trim_set says.  A segment's userid is 1 + its place in the forward, its adapter slot goes per tile, and the
  // trunk output at every query token lands in Qs in forward order, from where one gather puts Q into user order.
  int retrieval_forward_packed() {
    const int NT = (S + 31) / 32;
    std::vector<int> n_live((size_t)nu), uid((size_t)nu, 0), order((size_t)nu);
    for (int64_t u = 0; u < nu; ++u) {
      const int32_t* id = rb->userid + (size_t)u * S;
      int live = retrieval_token[u] / 2 + 1;
      if (full) live = std::max(live, user_desc[4 * u] + 1);
      int j = S;
      while (j > live && id[j - 1] == 0) --j;
      n_live[u] = std::max(live, j);
      for (int c = 0; c < n_live[u]; ++c) {
        if (id[c] == 0) continue;
        ARG_CHECK(uid[u] == 0 || uid[u] == id[c], "render_request: a packed retrieval row holds one user (one userid beside 0)");
        uid[u] = id[c];
      }
      order[u] = (int)u;
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n_live[a] > n_live[b]; });
    struct Seg { int user, col0; };
    struct Row { int taken = 0, end = 0; std::vector<Seg> segs; };
    std::vector<Row> prow;
    for (int u : order) {
      size_t r = 0;
      while (r < prow.size() && prow[r].taken + n_live[u] > S) ++r;
      if (r == prow.size()) prow.emplace_back();
      prow[r].segs.push_back({u, prow[r].taken});
      prow[r].end = prow[r].taken + n_live[u];
      prow[r].taken += (n_live[u] + 31) / 32 * 32;
    }
    // the packed rows of one forward, host side (everything a segment does not cover stays zero)
    const size_t cap = (size_t)RM * S;
    std::vector<double> p_time(cap);
    std::vector<int32_t> p_int[7];
    std::vector<float> p_rating(cap), p_progress(cap);
    for (auto& v : p_int) v.resize(cap);
    const int32_t* src_i[7] = {rb->userid, rb->token_mask_ids, rb->gender, rb->source, rb->matchedid, rb->status, rb->rope_input_pos};
    const std::vector<float> zf(cap, 0.f);
    const std::vector<int32_t> zi(cap, 0);
    t.place.assign((size_t)nu, 0);
    int at = 0;   // users forwarded so far: the first row of Qs the forward writes
    for (size_t r0 = 0; r0 < prow.size(); r0 += RM) {
      const int nr = (int)std::min<size_t>(RM, prow.size() - r0);
      std::fill(p_time.begin(), p_time.end(), 0.0); std::fill(p_rating.begin(), p_rating.end(), 0.f); std::fill(p_progress.begin(), p_progress.end(), 0.f);
      for (auto& v : p_int) std::fill(v.begin(), v.end(), 0);
      int end = 1;
      for (int r = 0; r < nr; ++r) end = std::max(end, prow[r0 + r].end);
      const int rl = std::min(S, (end + 31) / 32 * 32);
      t.tok.clear(); t.segs.clear(); t.tiles.assign((size_t)nr * NT, -1);
      for (int r = 0; r < nr; ++r) {
        for (const Seg& sg : prow[r0 + r].segs) {
          const int u = sg.user, n = n_live[u];
          const size_t so = (size_t)u * S, po = (size_t)r * S + sg.col0;
          std::copy(rb->time + so, rb->time + so + n, p_time.begin() + po);
          for (int k = 0; k < 7; ++k) std::copy(src_i[k] + so, src_i[k] + so + n, p_int[k].begin() + po);
          std::copy(rb->rating + so, rb->rating + so + n, p_rating.begin() + po);
          std::copy(rb->progress + so, rb->progress + so + n, p_progress.begin() + po);
          const int k1 = (int)t.tok.size() + 1;
          for (int c = 0; c < n; ++c) if (p_int[0][po + c] != 0) p_int[0][po + c] = k1;
          t.place[u] = at + k1 - 1;
          t.tok.push_back(r * 2 * rl + 2 * sg.col0 + retrieval_token[u]);
          t.segs.push_back({u, r, sg.col0, n, uid[u]});
          if (slots) std::fill(t.tiles.begin() + (size_t)r * NT + sg.col0 / 32, t.tiles.begin() + (size_t)r * NT + (sg.col0 + n + 31) / 32, slots[2 * group_medium[group[u]]]);
        }
      }
      const int nseg = (int)t.tok.size();
      rsys_batch b{};
      b.rows = nr;
      b.userid = p_int[0].data(); b.token_mask_ids = p_int[1].data(); b.gender = p_int[2].data(); b.source = p_int[3].data();
      b.matchedid = p_int[4].data(); b.status = p_int[5].data(); b.rope_input_pos = p_int[6].data();
      b.time = p_time.data(); b.rating = p_rating.data(); b.progress = p_progress.data();
      for (int k = 0; k < 6; ++k) { b.label[k] = zf.data(); b.weight[k] = zf.data(); b.position[k] = zi.data(); }
      RC(rl == S ? model_batch_upload(m, &b) : model_batch_upload_trimmed(m, &b, rl));
      R->note_forward(0, nr, rl);
      if (full) {   // the users' history columns back to one kept row each, [n_users][S]: what the store rows are cut from
        HIP_CHECK(hipMemcpyAsync(d_segs, t.segs.data(), (size_t)nseg * sizeof(SegDesc), hipMemcpyHostToDevice, s));
        const BatchDev& bd = m->resident.bd;
        const SegSrc br{bd.time, bd.userid, bd.gender, bd.source, bd.matchedid, bd.status, bd.rating, bd.progress};
        tic(m, "render_unpack_rows");
        unpack_rows_kernel<<<nseg, RN_THREADS, 0, s>>>(d_segs, br, rl, hist);
        RN_LAUNCH_CHECK();
        toc(m);
      }
      HIP_CHECK(hipMemcpyAsync(d_sel, t.tok.data(), (size_t)nseg * 4, hipMemcpyHostToDevice, s));
      RC(model_infer_device(m, 0, nullptr, d_sel, nseg, Qs + (size_t)at * D, slots ? t.tiles.data() : nullptr));
      HIP_CHECK(hipStreamSynchronize(s));   // (the host tables and the packed rows are rewritten by the next forward)
      ++R->forwards[0];
      at += nseg;
    }
    HIP_CHECK(hipMemcpyAsync(d_order, t.place.data(), (size_t)nu * 4, hipMemcpyHostToDevice, s));
    RC(launch_gather_rows_plain<float>(Qs, D, d_order, 0, Q, (int)nu, D, s));   // Q[u] = Qs[place[u]]: user order, as every later stage reads it
    HIP_CHECK(hipStreamSynchronize(s));   // (Qs and d_order are the scratch of the next stage)
    if (keep) {
      std::vector<float> h((size_t)nu * D);
      HIP_CHECK(hipMemcpy(h.data(), Q, h.size() * 4, hipMemcpyDeviceToHost));
      R->put("queries", h.data(), h.size());
    }
    return RSYS_OK;
  }

  // ---- 2. + 3. retrieval per medium, then the page window of each group
  int retrieve_and_window() {
    const int V[2] = {m->V0, m->V1};
    gloc.resize(ng); total.assign(ng, 0);
    for (int g = 0; g < ng; ++g) { gloc[g] = (int)groups_m[group_medium[g]].size(); groups_m[group_medium[g]].push_back(g); }
    for (int64_t u = 0; u < nu; ++u) users_m[group_medium[group[u]]].push_back((int)u);
    std::vector<std::vector<int32_t>> kept_ids(keep ? ng : 0);
    int cand_n = 0;
    for (int mm = 0; mm < 2; ++mm) {
      const std::vector<int>& us = users_m[mm];
      const std::vector<int>& gs = groups_m[mm];
      if (gs.empty()) continue;
      const int nq = (int)us.size(), ngm = (int)gs.size(), k = std::min(V[mm], RN_CAP);
      HIP_CHECK(hipMemcpyAsync(d_order, us.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
      RC(launch_gather_rows_plain<float>(Q, D, d_order, 0, Qs, nq, D, s));
      std::vector<int32_t> lg(nq);
      for (int i = 0; i < nq; ++i) lg[i] = gloc[group[us[i]]];
      const SubCsr h(us, hist_list), sl(gs, sel_list);
      std::vector<int32_t> counts(ngm);
      std::vector<float> wu, ws;
      std::vector<int> tloc(ng, -1);
      for (int j = 0; j < ngm; ++j) tloc[gs[j]] = j;
      SubTexts st;
      Request rq;
      rq.nq = nq; rq.group = lg.data(); rq.ng = ngm; rq.hist = h.history(); rq.sel = sl.selected();
      rq.qw = {sub_weights(us, qw.user, wu), sub_sel_weights(gs, sel_list.off, qw.sel, ws)};
      rq.qt = sub_texts(qt[mm], tloc, st);
      RetrieveDev rd; rd.d_queries = Qs;
      RC(model_retrieve_request(m, mm, rq, k, nullptr, &rd, nullptr, nullptr, counts.data()));
      std::vector<Win> wins;
      for (int j = 0; j < ngm; ++j) {
        const int g = gs[j];
        total[g] = counts[j];
        if (keep) {
          kept_ids[g].resize(counts[j]);
          if (counts[j]) HIP_CHECK(hipMemcpy(kept_ids[g].data(), rd.d_ids + (size_t)j * k, (size_t)counts[j] * 4, hipMemcpyDeviceToHost));
        }
        int start, stop, sidx, eidx;
        if (!page_window(counts[j], offset[g], limit[g], &start, &stop, &sidx, &eidx)) continue;
        act_m[mm].push_back({g, cand_n, stop - start, sidx, eidx});
        wins.push_back({j * k + start, stop - start, cand_n});
        cand_n += stop - start;
      }
      if (!wins.empty()) {
        HIP_CHECK(hipMemcpyAsync(d_win, wins.data(), wins.size() * sizeof(Win), hipMemcpyHostToDevice, s));
        window_kernel<<<(unsigned)wins.size(), RN_THREADS, 0, s>>>(d_win, rd.d_ids, cand);
        RN_LAUNCH_CHECK();
        HIP_CHECK(hipStreamSynchronize(s));   // (wins is rewritten; the next medium's retrieval reuses the id rows)
      }
    }
    if (keep) {
      R->put("ret.counts", total.data(), total.size());
      R->kept["ret.ids"];
      for (int g = 0; g < ng; ++g) R->put("ret.ids", kept_ids[g].data(), kept_ids[g].size());
    }
    return RSYS_OK;
  }

  // the split row of user u (medium mm) with candidates [c0, c0 + n) of its group's window, which starts at slot `window` of the candidate list
  RowDesc make_row(int u, int mm, int window, int c0, int n) const {
    const int32_t* d = user_desc + 4 * (int64_t)u;
    RowDesc r{};
    r.user = u; r.med = mm; r.userid = d[1]; r.gender = d[2]; r.source = d[3];
    r.moff = mm ? m->V0 : 0; r.cand0 = window + c0; r.ncand = n;
    r.ncopy = r.mask0 = r.cpos = d[0];
    r.rm0 = (int)(rm_off[u] + c0); r.ts = user_ts[u];
    return r;
  }

  // ---- 4. the ranking rows of every active group, media mixed, and where their values go in r_masked
  void plan_ranking() {
    gact.assign(ng, -1); rm_off.assign(nu, 0);
    for (int mm = 0; mm < 2; ++mm) {
      for (size_t a = 0; a < act_m[mm].size(); ++a) gact[act_m[mm][a].g] = (int)a;
      rm_base[mm] = mm ? rm_n[0] : 0;
      for (int u : users_m[mm]) {
        const int a = gact[group[u]];
        if (a < 0) continue;
        const Active& A = act_m[mm][a];
        ausers_m[mm].push_back(u);
        rm_off[u] = rm_base[mm] + rm_n[mm];
        if (full && user_desc[4 * (int64_t)u] >= 1) {   // through the cache: no history columns, every token at position n_hist, mask id 0
          RowDesc q = make_row(u, mm, A.c0, 0, A.n);
          q.ncopy = 0; q.mask0 = -1; q.fill_pos = q.cpos;
          cached.push_back(q);
        } else {
          for (int c0 = 0; c0 < A.n; c0 += chunk) rows.push_back(make_row(u, mm, A.c0, c0, std::min(chunk, A.n - c0)));
        }
        rm_n[mm] += A.n;
      }
    }
  }

  // the batch of n rows from their descriptors: the resident batch, filled on the device
  // (rl: the wave's row length, row_len_for its longest row: the rows' stride in the batch and in the token indices of d_sel)
  int assemble(const char* label, const RowDesc* host, RowDesc* dev, int n, BatchDevRows* bd, int rl) {
    RC(model_batch_device_begin(m, n, bd, rl));
    HIP_CHECK(hipMemcpyAsync(dev, host, (size_t)n * sizeof(RowDesc), hipMemcpyHostToDevice, s));
    tic(m, label);
    rows_kernel<<<n, RN_THREADS, 0, s>>>(dev, hist, rl, cand, *bd, d_sel);
    RN_LAUNCH_CHECK();
    toc(m);
    return RSYS_OK;
  }

  // ---- 5. one ranking forward over the n <= max_rows rows w[0 .. n): the rating head's values at their candidates go to r_masked.
  // WAVE_CACHED: the cache's candidate pass, row r on cache slot slot[r]; WAVE_ASSEMBLED: the plain forward.  `wave` numbers the kept records.
  int rank_wave(WaveKind kind, RowDesc* w, const int32_t* slot, int n, int wave) {
    int nsel = 0, live = 1;
    for (int r = 0; r < n; ++r) {
      w[r].sel0 = nsel; nsel += w[r].ncand;
      t.nc[r] = w[r].ncand; t.ra[r] = slots ? slots[2 * w[r].med + 1] : -1;
      live = std::max(live, w[r].ncopy + w[r].ncand);
    }
    const int rl = row_len_for(live);
    BatchDevRows bd;
    RC(assemble(WAVE_KEYS[kind][0], w, d_rows, n, &bd, rl));
    R->note_forward(kind == WAVE_CACHED ? 2 : 3, n, rl);
    if (kind == WAVE_CACHED) RC(rank_cache_candidates_rows(m, slots ? t.ra.data() : nullptr, slot, t.nc.data(), t.c_tab.data(), bd.rope_pos, d_sel, nsel, pred));
    else RC(model_infer_device(m, 1, slots ? t.ra.data() : nullptr, d_sel, nsel, pred));
    tic(m, "render_rank_scatter");
    rank_scatter_kernel<<<n, RN_THREADS, 0, s>>>(d_rows, pred, rm);
    RN_LAUNCH_CHECK();
    toc(m);
    HIP_CHECK(hipStreamSynchronize(s));   // (the row tables are rewritten by the next wave)
    ++R->forwards[1];
    if (full) ++R->forwards_full[1 + kind];   // (rsys_render_request_full counts its forwards by kind: candidate rows, empty histories)
    if (keep) {
      std::vector<int> fp(n);
      for (int r = 0; r < n; ++r) fp[r] = w[r].fill_pos;
      RC(R->keep_rows(WAVE_KEYS[kind][1], bd, n, S, rl, fp));
      std::vector<int32_t> hi((size_t)std::max(nsel, 1));
      HIP_CHECK(hipMemcpy(hi.data(), d_sel, (size_t)nsel * 4, hipMemcpyDeviceToHost));
      for (int i = 0; i < nsel && rl != S; ++i) hi[i] = hi[i] / (2 * rl) * 2 * S + hi[i] % (2 * rl);   // (kept in the documented geometry r 2S + t)
      R->put(WAVE_KEYS[kind][2], hi.data(), (size_t)nsel);
      for (int r = 0; r < n; ++r) {
        const int32_t rec[7] = {w[r].user, group[w[r].user], w[r].cand0, w[r].ncand, r, wave, (int32_t)kind};   // user, group, first candidate, count, row in wave, wave (, full: kind)
        R->put("rows", rec, full ? 7 : 6);
      }
    }
    return RSYS_OK;
  }

  // ---- 4. + 5. (full) the users with a history through the K/V cache: per wave of <= max_rows users one store forward over their history
  // rows, then their candidate rows (<= S candidates each, a user's candidates may span rows) in batches of <= max_rows rows, media mixed.
  // The host tables of a wave are read by stream-ordered copies: they stay as they are until the wave's last batch has been waited for.
  int rank_cached_waves() {
    if (cached.empty()) return RSYS_OK;
    if (pack_rank) return rank_cached_waves_packed();
    t.sd.resize(RM); t.s_nh.resize(RM); t.s_slot.resize(RM); t.s_ad.resize(RM); t.s_tab.resize((size_t)3 * RM); t.c_tab.resize((size_t)3 * RM);
    int cand_forward = 0;
    for (size_t w0 = 0; w0 < cached.size(); w0 += RM) {
      const int nw = (int)std::min<size_t>(RM, cached.size() - w0);
      t.crows.clear(); t.crow_slot.clear();
      for (int r = 0; r < nw; ++r) {
        const RowDesc& cu = cached[w0 + r];
        t.sd[r] = RowDesc{};
        t.sd[r].user = cu.user; t.sd[r].ncopy = cu.cpos;
        t.s_nh[r] = cu.cpos; t.s_slot[r] = r; t.s_ad[r] = slots ? slots[2 * cu.med + 1] : -1;
        for (int c0 = 0; c0 < cu.ncand; c0 += S) {   // the user's window in rows of <= S candidates
          RowDesc q = cu;
          q.cand0 += c0; q.rm0 += c0; q.ncand = std::min(S, cu.ncand - c0);
          t.crows.push_back(q); t.crow_slot.push_back(r);
        }
      }
      int live = 1;
      for (int r = 0; r < nw; ++r) live = std::max(live, t.sd[r].ncopy);
      const int rl = row_len_for(live);
      BatchDevRows bd;
      RC(assemble("render_store_rows", t.sd.data(), d_store, nw, &bd, rl));
      R->note_forward(1, nw, rl);
      RC(rank_cache_store_rows(m, slots ? t.s_ad.data() : nullptr, t.s_nh.data(), t.s_slot.data(), t.s_tab.data()));   // (no host wait)
      ++R->forwards[1]; ++R->forwards_full[0];
      if (keep) {
        RC(R->keep_rows("store", bd, nw, S, rl, std::vector<int>(nw, 0)));
        for (int r = 0; r < nw; ++r) {
          const int32_t rec[4] = {t.sd[r].user, r, t.sd[r].ncopy, (int32_t)(w0 / RM)};   // user, slot, events, wave
          R->put("store.rows", rec, 4);
        }
      }
      for (size_t b0 = 0; b0 < t.crows.size(); b0 += RM)
        RC(rank_wave(WAVE_CACHED, t.crows.data() + b0, t.crow_slot.data() + b0, (int)std::min<size_t>(RM, t.crows.size() - b0), cand_forward++));
    }
    return RSYS_OK;
  }

  // ---- 4. + 5. (full, rsys_serving_pack_ranking_set) the same with packed store rows, serve.rank_cache_pack_plan's store stage: a wave
  // holds up to rc_slots users (slot = the user's place in the wave); its histories become segments on 32-column boundaries, first-fit
  // decreasing, ties in user order, rows in the order they were opened, forwards of <= max_rows rows at the trim length of their fullest
  // row -- if that needs fewer forwards than one history per row at its trim length, or as many and fewer tokens; otherwise one history
  // per row at column 0.  Either way the rows are cut from the kept history rows by pack_store_rows_kernel and stored through the packed
  // store body, without a host wait.  The candidate rows, their forwards and rank_scatter_kernel are rank_cached_waves'.
  // The host tables of a wave are read by stream-ordered copies: every forward has its own, kept until the wave's last batch has been waited for.
  int rank_cached_waves_packed() {
    struct Place { int k, row, col0; };                      // user k of the wave at column col0 of row `row` of its forward
    struct Fwd { int rl = 0, rows = 0; std::vector<Place> at; };
    struct Tabs { std::vector<SegDesc> desc; std::vector<int32_t> seg, ad; };
    const int W = std::max(m->rc_slots, 1);
    t.c_tab.resize((size_t)3 * RM);
    auto tokens = [](const std::vector<Fwd>& f) { long long n = 0; for (const Fwd& x : f) n += (long long)x.rl * x.rows; return n; };
    int cand_forward = 0, wave = 0;
    for (size_t w0 = 0; w0 < cached.size(); w0 += W, ++wave) {
      const int nw = (int)std::min<size_t>(W, cached.size() - w0);
      t.crows.clear(); t.crow_slot.clear();
      std::vector<int> n(nw), order(nw);
      for (int k = 0; k < nw; ++k) {
        const RowDesc& cu = cached[w0 + k];
        n[k] = cu.cpos; order[k] = k;
        for (int c0 = 0; c0 < cu.ncand; c0 += S) {   // the user's window in rows of <= S candidates
          RowDesc q = cu;
          q.cand0 += c0; q.rm0 += c0; q.ncand = std::min(S, cu.ncand - c0);
          t.crows.push_back(q); t.crow_slot.push_back(k);
        }
      }
      // the two layouts of the store stage
      std::vector<Fwd> single, packed;
      for (int k0 = 0; k0 < nw; k0 += RM) {
        Fwd f; int live = 1;
        for (int k = k0; k < std::min(nw, k0 + RM); ++k) { f.at.push_back({k, k - k0, 0}); live = std::max(live, n[k]); }
        f.rows = (int)f.at.size(); f.rl = std::min(S, (live + 31) / 32 * 32);
        single.push_back(f);
      }
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n[a] > n[b]; });
      struct Row { int taken = 0, end = 0; std::vector<Place> at; };
      std::vector<Row> prow;
      for (int k : order) {
        size_t r = 0;
        while (r < prow.size() && prow[r].taken + n[k] > S) ++r;
        if (r == prow.size()) prow.emplace_back();
        prow[r].at.push_back({k, 0, prow[r].taken});
        prow[r].end = prow[r].taken + n[k];
        prow[r].taken += (n[k] + 31) / 32 * 32;
      }
      for (size_t r0 = 0; r0 < prow.size(); r0 += RM) {
        Fwd f; int end = 1;
        f.rows = (int)std::min<size_t>(RM, prow.size() - r0);
        for (int r = 0; r < f.rows; ++r) {
          end = std::max(end, prow[r0 + r].end);
          for (Place p : prow[r0 + r].at) { p.row = r; f.at.push_back(p); }
        }
        f.rl = std::min(S, (end + 31) / 32 * 32);
        packed.push_back(f);
      }
      const bool take_packed = packed.size() < single.size() || (packed.size() == single.size() && tokens(packed) < tokens(single));
      const std::vector<Fwd>& plan = take_packed ? packed : single;
      std::vector<Tabs> tabs(plan.size());
      for (size_t fi = 0; fi < plan.size(); ++fi) {
        const Fwd& f = plan[fi];
        Tabs& tb = tabs[fi];
        for (const Place& p : f.at) {
          const RowDesc& cu = cached[w0 + p.k];
          tb.desc.push_back({cu.user, p.row, p.col0, n[p.k], (int)tb.desc.size() + 1});
          const int32_t sg[4] = {p.row, p.col0, n[p.k], p.k};
          tb.seg.insert(tb.seg.end(), sg, sg + 4);
          tb.ad.push_back(slots ? slots[2 * cu.med + 1] : -1);
        }
        const int nseg = (int)tb.desc.size();
        BatchDevRows bd;
        RC(model_batch_device_begin(m, f.rows, &bd, f.rl));
        HIP_CHECK(hipMemcpyAsync(d_segs, tb.desc.data(), (size_t)nseg * sizeof(SegDesc), hipMemcpyHostToDevice, s));
        tic(m, "render_store_rows");
        pack_store_rows_kernel<<<f.rows, RN_THREADS, 0, s>>>(d_segs, nseg, hist, f.rl, bd);
        RN_LAUNCH_CHECK();
        toc(m);
        R->note_forward(1, f.rows, f.rl);
        RC(rank_cache_store_packed_rows(m, slots ? tb.ad.data() : nullptr, nseg, tb.seg.data(), bd.rope_pos));   // (no host wait)
        ++R->forwards[1]; ++R->forwards_full[0];
        if (keep) {
          HIP_CHECK(hipStreamSynchronize(s));
          RC(R->keep_rows("store", bd, f.rows, S, f.rl, std::vector<int>(f.rows, 0)));
          for (const Place& p : f.at) {
            const int32_t rec[4] = {cached[w0 + p.k].user, p.k, n[p.k], wave};   // user, slot, events, wave
            R->put("store.rows", rec, 4);
          }
        }
      }
      for (size_t b0 = 0; b0 < t.crows.size(); b0 += RM)
        RC(rank_wave(WAVE_CACHED, t.crows.data() + b0, t.crow_slot.data() + b0, (int)std::min<size_t>(RM, t.crows.size() - b0), cand_forward++));
      HIP_CHECK(hipStreamSynchronize(s));   // (the wave's host tables go out of scope)
    }
    return RSYS_OK;
  }

  // ---- 4. + 5. the split rows: user x chunk, waves of <= max_rows rows, media mixed
  int rank_assembled_waves() {
    const size_t n_prefix = (size_t)nu * P;
    if (!rows.empty() && n_prefix) {   // the history part of the rows: uploaded once, per user
      HIP_CHECK(hipMemcpyAsync(hist.time, pb->time, n_prefix * 8, hipMemcpyHostToDevice, s));
      const int32_t* src_i[7] = {pb->userid, pb->token_mask_ids, pb->gender, pb->source, pb->matchedid, pb->status, pb->rope_input_pos};
      int* dst_i[7] = {hist.userid, hist.tmid, hist.gender, hist.source, hist.matchedid, hist.status, hist.rope};
      for (int k = 0; k < 7; ++k) HIP_CHECK(hipMemcpyAsync(dst_i[k], src_i[k], n_prefix * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(hist.rating, pb->rating, n_prefix * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(hist.progress, pb->progress, n_prefix * 4, hipMemcpyHostToDevice, s));
    }
    for (size_t r0 = 0; r0 < rows.size(); r0 += RM)
      RC(rank_wave(WAVE_ASSEMBLED, rows.data() + r0, nullptr, (int)std::min<size_t>(RM, rows.size() - r0), (int)(r0 / RM)));
    return RSYS_OK;
  }

  // ---- 6. ranking + reranking per medium; the pages come back
  int rank_and_rerank() {
    pages.resize(ng);
    for (int mm = 0; mm < 2; ++mm) {
      const std::vector<Active>& act = act_m[mm];
      if (act.empty()) continue;
      const std::vector<int>& us = ausers_m[mm];
      const int na = (int)act.size(), nq = (int)us.size();
      HIP_CHECK(hipMemcpyAsync(d_order, us.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
      RC(launch_gather_rows_plain<float>(Q, D, d_order, 0, Qs, nq, D, s));
      std::vector<int64_t> coff(na + 1, 0), poff(na);
      std::vector<int32_t> pk(na), plo(na), phi(na), lg(nq);
      std::vector<float> pen((size_t)na * 4);
      int64_t np = 0;
      for (int a = 0; a < na; ++a) {
        coff[a + 1] = coff[a] + act[a].n;
        pk[a] = act[a].eidx; plo[a] = act[a].sidx - 1; phi[a] = act[a].eidx; poff[a] = np; np += phi[a] - plo[a];
        memcpy(&pen[4 * (size_t)a], penalties + 4 * (size_t)act[a].g, 16);
      }
      for (int i = 0; i < nq; ++i) lg[i] = gact[group[us[i]]];
      const SubCsr h(us, hist_list);
      std::vector<int32_t> page(std::max<int64_t>(np, 1)), kp(keep ? coff[na] : 0);
      std::vector<float> kr(keep ? coff[na] : 0);
      RankDev rd{cand + act[0].c0, Qs, rm + rm_base[mm], plo.data(), phi.data(), poff.data(), page.data(), keep ? kr.data() : nullptr,
                 keep ? kp.data() : nullptr};
      const int have = coef_have ? coef_have[mm] : 0;
      const float* cf = coefs ? coefs + 4 * mm : nullptr;
      std::vector<float> wu;
      SubTexts st;
      Request rq;
      rq.nq = nq; rq.group = lg.data(); rq.ng = na; rq.hist = h.history();
      rq.qw.user = sub_weights(us, qw.user, wu);
      rq.qt = sub_texts(qt[mm], gact, st);   // (a text of medium mm belongs to a group of medium mm)
      RankCands rc;
      rc.cand_off = coff.data(); rc.partialk = pk.data(); rc.penalties = pen.data(); rc.n_rm = rm_n[mm];
      if (have & 1) rc.retrieval_coef = cf;
      if (have & 2) { rc.rating_coefs = cf + 1; rc.rating_mean = cf[3]; }
      RC(model_rank_request_dev(m, mm, rq, rc, &rd));
      for (int a = 0; a < na; ++a) pages[act[a].g].assign(page.begin() + poff[a], page.begin() + poff[a] + (phi[a] - plo[a]));
      if (keep) {
        std::vector<float> hrm((size_t)rm_n[mm]);
        if (rm_n[mm]) HIP_CHECK(hipMemcpy(hrm.data(), rm + rm_base[mm], hrm.size() * 4, hipMemcpyDeviceToHost));
        R->put("r_masked", hrm.data(), hrm.size());
        for (int u : us) {
          const int32_t rec[3] = {u, (int32_t)rm_off[u], act[gact[group[u]]].n};   // user, first value in "r_masked", values
          R->put("rm_users", rec, 3);
        }
        for (int a = 0; a < na; ++a) {
          const int32_t rec[6] = {act[a].g, mm, act[a].c0, act[a].n, act[a].sidx, act[a].eidx};   // group, medium, first slot in "r" / "picks", candidates, page
          R->put("groups", rec, 6);
        }
        R->put("r", kr.data(), kr.size());
        R->put("picks", kp.data(), kp.size());
      }
    }
    return RSYS_OK;
  }

  // ---- outputs, once everything has succeeded
  void write_outputs() {
    int64_t at = 0;
    for (int g = 0; g < ng; ++g) {
      ids_offsets[g] = at;
      if (!pages[g].empty()) memcpy(ids_out + at, pages[g].data(), pages[g].size() * 4);
      at += (int64_t)pages[g].size();
      total_out[g] = total[g];
    }
    ids_offsets[ng] = at;
  }

  int run_stages() {
    RC(render_carve());
    RC(pack ? retrieval_forward_packed() : retrieval_forward());
    RC(retrieve_and_window());
    plan_ranking();
    RC(rank_cached_waves());
    RC(rank_assembled_waves());
    RC(rank_and_rerank());
    if (keep) R->complete_keys(full ? 3 : 1);
    write_outputs();
    return RSYS_OK;
  }
};

}  // namespace

// The one body of rsys_render_request and rsys_render_request_full (a.full).
int model_render(Model* m, const RenderArgs& a) {
  Render c(m, a);
  RC(c.render_check());
  HIP_CHECK(hipSetDevice(m->device));
  c.s = m->stream;
  const int rc = c.run_stages();
  if (rc != RSYS_OK) (void)hipStreamSynchronize(c.s);   // (copies a failed stage has enqueued read the context's host tables)
  return rc;
}

// rsys_render_items.  Per medium: the window of render.jl:448-463 from each group's offset (the same arithmetic as page_window, before
// the total is known: the window's first rank does not depend on it), rsys_retrieve_window without queries, the windows gathered into
// one candidate list, the reranking of rsys_rank_request on zeros.  Outputs are written once both media have succeeded.
int model_render_items(Model* m, int32_t ng, const int32_t* group_medium, const int64_t* offset, const int32_t* limit, const float* penalties,
                       const SelectedList& sel, int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out,
                       const float* sel_w, const QueryTexts* qt) {
  ARG_CHECK(ng >= 1 && ng <= RN_MAXQ, "render_items: 1 <= n_groups <= 4096");
  ARG_CHECK(group_medium && offset && limit && penalties && ids_out && ids_offsets && total_out, "render_items: null argument");
  RC(check_ragged("render_items", sel, ng));
  int64_t need_ids = 0;
  std::vector<int> groups_m[2];
  for (int g = 0; g < ng; ++g) {
    ARG_CHECK(group_medium[g] == 0 || group_medium[g] == 1, "render_items: medium must be 0 or 1");
    ARG_CHECK(limit[g] >= 1 && limit[g] <= RN_MAX_RANK, "render_items: 1 <= limit <= 1024");
    ARG_CHECK(offset[g] >= 0, "render_items: offset >= 0");
    need_ids += limit[g];
    groups_m[group_medium[g]].push_back(g);
  }
  ARG_CHECK(ids_cap >= need_ids, "render_items: ids_out must hold the sum of the limits");
  for (int mm = 0; mm < 2; ++mm) {   // the tables of the reranking, before anything runs (the retrieval checks its own)
    if (groups_m[mm].empty()) continue;
    int64_t dim = 0;
    ARG_CHECK(retrieve_similarity_table(m, mm, &dim) != nullptr, "render_items: the item-similarity embeddings of the medium are not loaded");
  }
  HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  RenderState* R = render_state(m);
  int32_t* cand; Win* d_win;
  RC(carve_into(R->ws, s, [&](Carve& c) {
    cand = c.take<int32_t>((size_t)ng * RN_MAX_RANK);
    d_win = c.take<Win>(ng);
  }));
  std::vector<int32_t> total(ng, 0);
  std::vector<std::vector<int32_t>> pages(ng);
  for (int mm = 0; mm < 2; ++mm) {
    const std::vector<int>& gs = groups_m[mm];
    if (gs.empty()) continue;
    const int ngm = (int)gs.size();
    std::vector<int64_t> wstart(ngm);
    std::vector<int32_t> wlen(ngm), counts(ngm), totals(ngm);
    for (int j = 0; j < ngm; ++j) {
      const int mitr = RN_MAX_RANK - RN_MAX_RANK % limit[gs[j]];
      wstart[j] = offset[gs[j]] / mitr * mitr;
      wlen[j] = mitr;
    }
    const SubCsr sl(gs, sel);
    const RetrieveWin win{wstart.data(), wlen.data(), totals.data()};
    std::vector<float> ws;
    std::vector<int> tloc(ng, -1);
    for (int j = 0; j < ngm; ++j) tloc[gs[j]] = j;
    SubTexts st;
    Request rq;   // (no users: every group is scored by its prior and its texts)
    rq.ng = ngm; rq.sel = sl.selected();
    rq.qw.sel = sub_sel_weights(gs, sel.off, sel_w, ws);
    if (qt) rq.qt = sub_texts(qt[mm], tloc, st);
    RetrieveDev rd;
    RC(model_retrieve_request(m, mm, rq, 0, &win, &rd, nullptr, nullptr, counts.data()));
    std::vector<Win> wins;
    std::vector<int> act;
    std::vector<int64_t> coff(1, 0), poff;
    std::vector<int32_t> pk, plo, phi;
    std::vector<float> pen;
    int64_t np = 0;
    for (int j = 0; j < ngm; ++j) {
      const int g = gs[j];
      total[g] = totals[j];
      int start, stop, sidx, eidx;
      if (!page_window(totals[j], offset[g], limit[g], &start, &stop, &sidx, &eidx)) continue;
      // (start == wstart[j] and stop - start == counts[j]: the retrieval clamped the same window)
      wins.push_back({j * RN_MAX_RANK, counts[j], (int)coff.back()});
      coff.push_back(coff.back() + counts[j]);
      act.push_back(g);
      const int last = std::min(eidx, counts[j]);   // (an offset that is no multiple of the limit may end the page past the ranked slice)
      pk.push_back(eidx); plo.push_back(sidx - 1); phi.push_back(last); poff.push_back(np); np += last - (sidx - 1);
      pen.insert(pen.end(), penalties + 4 * (size_t)g, penalties + 4 * (size_t)g + 4);
    }
    if (act.empty()) continue;
    const int na = (int)act.size();
    HIP_CHECK(hipMemcpyAsync(d_win, wins.data(), wins.size() * sizeof(Win), hipMemcpyHostToDevice, s));
    window_kernel<<<(unsigned)na, RN_THREADS, 0, s>>>(d_win, rd.d_ids, cand);
    RN_LAUNCH_CHECK();
    std::vector<int32_t> page((size_t)np);
    const RankDev rk{cand, nullptr, nullptr, plo.data(), phi.data(), poff.data(), page.data(), nullptr, nullptr};
    const int rc = model_rank_items_dev(m, mm, na, coff.data(), &rk, pk.data(), pen.data());
    if (rc != RSYS_OK) { (void)hipStreamSynchronize(s); return rc; }   // (the copy of `wins` may be in flight)
    for (int a = 0; a < na; ++a) pages[act[a]].assign(page.begin() + poff[a], page.begin() + poff[a] + (phi[a] - plo[a]));
  }
  int64_t at = 0;
  for (int g = 0; g < ng; ++g) {
    ids_offsets[g] = at;
    if (!pages[g].empty()) memcpy(ids_out + at, pages[g].data(), pages[g].size() * 4);
    at += (int64_t)pages[g].size();
    total_out[g] = total[g];
  }
  ids_offsets[ng] = at;
  return RSYS_OK;
}

}  // namespace rsys
