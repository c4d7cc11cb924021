// A page from raw histories in one device pipeline (Inference/compute.jl:512-531 + render.jl:437-474): the retrieval forward, `retrieval(state)`,
// the page window, the ranking forward and `ranking` + `reranking!` chained on the device for states of both media.  In: histories (as
// inference rows and as list items), selected items, penalties, pagination.  Out: the pages' ids and the totals.  User embeddings,
// retrieved candidates and rating-head values never leave the device; the per-group counts do (they size the ranking rows).
// Stages:
//   retrieval forward   the users' rows in waves of <= max_rows (media mixed, one adapter slot per row); the trunk output at each
//                       user's query token goes to the query buffer Q [n_users][D] fp32
//   retrieval           per medium the body of rsys_retrieve_request on the medium's rows of Q (gathered in user order)
//   window              render.jl:447-465 on the host from the counts; window_kernel copies each group's slice to the candidate list
//   ranking rows        rank_rows_kernel, one workgroup per row (user x chunk of <= S - S/2 candidates): history prefix from the uploaded
//                       per-user prefix, candidate tail of all ten arrays + RoPE positions + the action-token indices, one launch per wave
//   ranking forward     rows of both media in waves of <= max_rows, rating head at the selected tokens; rank_scatter_kernel puts the
//                       values into the ragged r_masked layout of rsys_rank_request
//   ranking, reranking  per medium the body of rsys_rank_request on device candidates, queries and r_masked; the page's ids come back
// rsys_render_request_full is the same pipeline with the ranking forward on the reference's row: every user with a
// history is ranked on all of its newest S - 1 events through the per-user K/V cache of rank_cache.hip.  The history columns of the
// retrieval rows stay on the device while the retrieval waves upload them, so no prefix is uploaded:
//   store rows          store_rows_kernel, one workgroup per user of a wave of <= max_rows users with a history: columns [0, n_hist) of the
//                       user's retrieval row, without its query token; one forward with rc_mode = 1 (slot = the user's place in the wave)
//   candidate rows      cand_rows_kernel, one workgroup per row of <= S candidates of one user: the candidate tokens, the RoPE positions
//                       (2 n_hist, 2 n_hist + 1) and the action-token indices; forwards with rc_mode = 2 in batches of <= max_rows rows
//   empty histories     the assembled rows above with nh = 0, in waves of their own
#include <algorithm>
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

// one ranking row: user `user`'s history prefix (nh tokens), then candidates cand[cand0 .. cand0 + ncand) of its group
struct RowDesc {
  int user, nh, userid, gender, source;
  int moff;          // added to a candidate id: V_0 for medium 1
  int cand0, ncand;
  int sel0;          // first slot of the row's action tokens in the wave's selection (and in its rating-head output)
  int rm0;           // first slot of the row's values in r_masked
  double ts;         // the user's timestamp: `time` of every candidate token
};

// the per-user history prefixes [n_users][P], device
struct Prefix {
  const double* time;
  const int *userid, *tmid, *gender, *source, *matchedid, *status, *rope;
  const float *rating, *progress;
};

struct Win { int src, n, dst; };

// row blockIdx.x of the wave: columns [0, nh) from the user's prefix, [nh, nh + ncand) the candidate tokens (serve.build_batch's tail:
// item = candidate, time = the user's timestamp, status -1, rating = progress = 0, position nh, mask id nh + j), the rest zero; the
// per-token RoPE positions (2 p, 2 p + 1) as rsys_batch_upload derives them; the candidates' action tokens row 2S + 2 (nh + j) + 1
__global__ void __launch_bounds__(RN_THREADS) rank_rows_kernel(const RowDesc* rows, Prefix pf, int P, int S, const int32_t* cand, BatchDevRows out,
                                                               int* sel) {
  const int r = blockIdx.x;
  const RowDesc d = rows[r];
  for (int j = threadIdx.x; j < S; j += RN_THREADS) {
    const long long i = (long long)r * S + j;
    double time = 0.0;
    int userid = 0, tmid = 0, gender = 0, source = 0, matchedid = 0, status = 0, p = 0;
    float rating = 0.f, progress = 0.f;
    if (j < d.nh) {
      const long long q = (long long)d.user * P + j;
      time = pf.time[q]; userid = pf.userid[q]; tmid = pf.tmid[q]; gender = pf.gender[q]; source = pf.source[q];
      matchedid = pf.matchedid[q]; status = pf.status[q]; rating = pf.rating[q]; progress = pf.progress[q]; p = pf.rope[q];
    } else if (j < d.nh + d.ncand) {
      const int c = j - d.nh;
      time = d.ts; userid = d.userid; gender = d.gender; source = d.source;
      matchedid = cand[d.cand0 + c] + d.moff; status = -1; p = d.nh; tmid = d.nh + c;
      sel[d.sel0 + c] = r * 2 * S + 2 * j + 1;
    }
    out.time[i] = time; out.userid[i] = userid; out.tmid[i] = tmid; out.gender[i] = gender; out.source[i] = source;
    out.matchedid[i] = matchedid; out.status[i] = status; out.rating[i] = rating; out.progress[i] = progress;
    ((int2*)out.rope_pos)[i] = make_int2(2 * p, 2 * p + 1);
  }
}

// the history columns of the users' retrieval rows [n_users][S], kept on the device by the retrieval waves (rsys_render_request_full)
struct HistRows {
  double* time;
  int *userid, *gender, *source, *matchedid, *status;
  float *rating, *progress;
};

struct StoreDesc { int user, nh; };

// store row blockIdx.x of the wave: columns [0, nh) of the user's retrieval row (positions 0 .. nh - 1, mask id 0), zeros from nh on --
// the retrieval row without its query token, which history tokens would attend to (serve._fill_row(hist, nh, ranking=False))
__global__ void __launch_bounds__(RN_THREADS) store_rows_kernel(const StoreDesc* rows, HistRows h, int S, BatchDevRows out) {
  const int r = blockIdx.x;
  const StoreDesc d = rows[r];
  for (int j = threadIdx.x; j < S; j += RN_THREADS) {
    const long long i = (long long)r * S + j;
    double time = 0.0;
    int userid = 0, gender = 0, source = 0, matchedid = 0, status = 0, p = 0;
    float rating = 0.f, progress = 0.f;
    if (j < d.nh) {
      const long long q = (long long)d.user * S + j;
      time = h.time[q]; userid = h.userid[q]; gender = h.gender[q]; source = h.source[q]; matchedid = h.matchedid[q]; status = h.status[q];
      rating = h.rating[q]; progress = h.progress[q]; p = j;
    }
    out.time[i] = time; out.userid[i] = userid; out.tmid[i] = 0; out.gender[i] = gender; out.source[i] = source;
    out.matchedid[i] = matchedid; out.status[i] = status; out.rating[i] = rating; out.progress[i] = progress;
    ((int2*)out.rope_pos)[i] = make_int2(2 * p, 2 * p + 1);
  }
}

// candidate row blockIdx.x of the batch (rsys_rank_cache_candidates' row): candidate j of the row at column j (item = candidate, time = the
// user's timestamp, status -1, rating = progress = 0, mask id 0), the rest zero; every token of the row at RoPE positions (2 nh, 2 nh + 1);
// the candidates' action tokens row 2S + 2 j + 1
__global__ void __launch_bounds__(RN_THREADS) cand_rows_kernel(const RowDesc* rows, int S, const int32_t* cand, BatchDevRows out, int* sel) {
  const int r = blockIdx.x;
  const RowDesc d = rows[r];
  for (int j = threadIdx.x; j < S; j += RN_THREADS) {
    const long long i = (long long)r * S + j;
    double time = 0.0;
    int userid = 0, gender = 0, source = 0, matchedid = 0, status = 0;
    if (j < d.ncand) {
      time = d.ts; userid = d.userid; gender = d.gender; source = d.source;
      matchedid = cand[d.cand0 + j] + d.moff; status = -1;
      sel[d.sel0 + j] = r * 2 * S + 2 * j + 1;
    }
    out.time[i] = time; out.userid[i] = userid; out.tmid[i] = 0; out.gender[i] = gender; out.source[i] = source;
    out.matchedid[i] = matchedid; out.status[i] = status; out.rating[i] = 0.f; out.progress[i] = 0.f;
    ((int2*)out.rope_pos)[i] = make_int2(2 * d.nh, 2 * d.nh + 1);
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

}  // namespace

struct RenderState {
  DevScratch ws;
  bool keep = false;                                   // rsys_render_debug_keep: the next calls keep their intermediates
  int forwards[2] = {0, 0};                            // forwards of the last call: retrieval, ranking
  int forwards_full[3] = {0, 0, 0};                    // rsys_render_request_full's ranking forwards: store, candidates, empty-history chunks
  std::map<std::string, std::vector<unsigned char>> kept;
  template <typename X> void put(const char* key, const X* p, size_t n) {
    std::vector<unsigned char>& v = kept[key];
    const size_t at = v.size();
    v.resize(at + n * sizeof(X));
    if (n) memcpy(v.data() + at, p, n * sizeof(X));
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

// list items / selected items of a subset of rows of a CSR, in subset order
struct SubCsr {
  std::vector<int64_t> off;
  std::vector<int32_t> a, b, c;
};
static void sub_csr(const std::vector<int>& rows, const int64_t* off, const int32_t* a, const int32_t* b, const int32_t* c, SubCsr& out) {
  out.off.assign(1, 0);
  for (int r : rows) {
    for (int64_t j = off[r]; j < off[r + 1]; ++j) {
      out.a.push_back(a[j]); out.b.push_back(b[j]);
      if (c) out.c.push_back(c[j]);
    }
    out.off.push_back((int64_t)out.a.size());
  }
  if (out.a.empty()) { out.a.push_back(0); out.b.push_back(0); out.c.push_back(0); }   // (non-null pointers for empty lists)
  if (c == nullptr) out.c.assign(1, 0);
}

// The one body of rsys_render_request (full == false: pb / P are the ranking prefixes) and rsys_render_request_full (full == true: pb ==
// nullptr, P == 0, user_desc[u][0] = n_hist = the history columns of retrieval row u).  Stages 1-3 and 6 are shared; 4-5 differ.
static int render_run(Model* m, bool full, int32_t ng, const int32_t* group_medium, const int64_t* offset, const int32_t* limit,
                      const float* penalties, int64_t nu, const int32_t* group, const rsys_batch* rb, const int32_t* retrieval_token,
                      const rsys_batch* pb, int32_t P, const int32_t* user_desc, const double* user_ts, const int32_t* slots,
                      const int64_t* hist_off, const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                      const int64_t* sel_off, const int32_t* sel_medium, const int32_t* sel_ids, const int32_t* coef_have, const float* coefs,
                      int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out) {
  const int S = m->S, D = m->D, chunk = S - S / 2, RM = m->rows_max;
  const int V[2] = {m->V0, m->V1};
  // ---- arguments.  Checked here, before anything is enqueued: the request's shape, pagination, groups, offsets' monotonicity, adapter
  // slots, descriptors and prefixes.  Checked later, by the code that owns them: the retrieval rows (rsys_batch_upload's checks, wave by
  // wave) and the ids of list and selected items and the tables they need (the request bodies) -- by then the retrieval forward may have
  // run and the resident batch is replaced.  In every case the outputs are written only after the last stage has succeeded.
  ARG_CHECK(!m->fp8, "render_request: fp32 and bf16 models only (the adapter bank's dtypes)");
  ARG_CHECK(!m->sharded, "render_request: the row-sharded item table is not supported (replicated table only)");
  ARG_CHECK(ng >= 1 && nu >= 1 && nu <= RN_MAXQ && ng <= nu, "render_request: 1 <= n_groups <= n_users <= 4096 (every group needs a user)");
  ARG_CHECK(group_medium && offset && limit && penalties && group && rb && retrieval_token && (pb || full) && user_desc && user_ts && ids_out &&
                ids_offsets && total_out,
            "render_request: null argument");
  RC(check_ragged("render_request", LIST_HISTORY, hist_off, nu, {hist_medium, hist_ids, hist_status}));
  RC(check_ragged("render_request", LIST_SELECTED, sel_off, ng, {sel_medium, sel_ids}));
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
      ARG_CHECK(pb->rope_input_pos[q] >= 0 && 2 * pb->rope_input_pos[q] + 1 < m->T, "render_request: prefix rope_input_pos out of range");
    }
  }
  ARG_CHECK(S / 2 + chunk <= 4096, "render_request: max_sequence_length <= 4096 (token_mask_ids of the candidates)");
  if (full) {   // the cache: the model's reserve when it holds a wave's users, else max_rows slots (RSYS_ERR_STATE when they do not fit)
    int with_hist = 0;
    for (int64_t u = 0; u < nu; ++u) with_hist += user_desc[4 * u] >= 1;
    if (m->rc_slots < std::min(RM, with_hist)) RC(model_rank_cache_reserve(m, RM));
  }
  RenderState* R = render_state(m);
  R->forwards[0] = R->forwards[1] = 0;
  R->forwards_full[0] = R->forwards_full[1] = R->forwards_full[2] = 0;
  const bool keep = R->keep;
  R->kept.clear();

  // ---- host plan: users and groups by medium
  std::vector<int> users_m[2], groups_m[2], gloc(ng), uslot(nu);
  for (int g = 0; g < ng; ++g) { gloc[g] = (int)groups_m[group_medium[g]].size(); groups_m[group_medium[g]].push_back(g); }
  for (int64_t u = 0; u < nu; ++u) users_m[group_medium[group[u]]].push_back((int)u);
  const int64_t n_prefix = (int64_t)nu * P;
  const size_t sel_cap = (size_t)RM * (full ? S : std::max(chunk, 1));   // (a candidate row of the cached path holds up to S candidates)
  const size_t n_hrows = full ? (size_t)nu * S : 0;

  HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  float *Q, *Qs, *pred, *rm; int *d_sel, *d_order; int32_t* cand; RowDesc* d_rows; Win* d_win; Prefix pf; double* pf_time;
  int *pf_i[7]; float *pf_f[2];
  HistRows hr; StoreDesc* d_store;
  RC(carve_into(R->ws, s, [&](Carve& c) {
    Q = c.take<float>((size_t)nu * D); Qs = c.take<float>((size_t)nu * D);
    pred = c.take<float>(sel_cap); rm = c.take<float>((size_t)nu * RN_MAX_RANK);
    d_sel = c.take<int>(sel_cap); d_order = c.take<int>(nu);
    cand = c.take<int32_t>((size_t)ng * RN_MAX_RANK);
    d_rows = c.take<RowDesc>(RM); d_win = c.take<Win>(ng);
    pf_time = c.take<double>(n_prefix);
    for (int k = 0; k < 7; ++k) pf_i[k] = c.take<int>(n_prefix);
    for (int k = 0; k < 2; ++k) pf_f[k] = c.take<float>(n_prefix);
    hr.time = c.take<double>(n_hrows);
    hr.userid = c.take<int>(n_hrows); hr.gender = c.take<int>(n_hrows); hr.source = c.take<int>(n_hrows);
    hr.matchedid = c.take<int>(n_hrows); hr.status = c.take<int>(n_hrows);
    hr.rating = c.take<float>(n_hrows); hr.progress = c.take<float>(n_hrows);
    d_store = c.take<StoreDesc>(full ? RM : 0);
  }));
  pf.time = pf_time; pf.userid = pf_i[0]; pf.tmid = pf_i[1]; pf.gender = pf_i[2]; pf.source = pf_i[3]; pf.matchedid = pf_i[4];
  pf.status = pf_i[5]; pf.rope = pf_i[6]; pf.rating = pf_f[0]; pf.progress = pf_f[1];

  // ---- 1. retrieval forward: waves of <= max_rows users in user order, media mixed
  const std::vector<float> zf((size_t)RM * S, 0.f);
  const std::vector<int32_t> zi((size_t)RM * S, 0);
  std::vector<int32_t> tok(RM), ra(RM);
  for (int64_t u0 = 0; u0 < nu; u0 += RM) {
    const int rows = (int)std::min<int64_t>(RM, nu - u0);
    const size_t o = (size_t)u0 * S;
    rsys_batch b{};
    b.rows = rows;
    b.userid = rb->userid + o; b.token_mask_ids = rb->token_mask_ids + o; b.gender = rb->gender + o; b.source = rb->source + o;
    b.matchedid = rb->matchedid + o; b.status = rb->status + o; b.time = rb->time + o; b.rating = rb->rating + o; b.progress = rb->progress + o;
    b.rope_input_pos = rb->rope_input_pos + o;
    for (int k = 0; k < 6; ++k) { b.label[k] = zf.data(); b.weight[k] = zf.data(); b.position[k] = zi.data(); }
    RC(model_batch_upload(m, &b));
    if (full) {   // the rows' history columns stay on the device: the store rows are cut from them, nothing of a history is uploaded twice
      const size_t n = (size_t)rows * S;
      const BatchDev& bd = m->bd;
      HIP_CHECK(hipMemcpyAsync(hr.time + o, bd.time, n * 8, hipMemcpyDeviceToDevice, s));
      const int* src_i[5] = {bd.userid, bd.gender, bd.source, bd.matchedid, bd.status};
      int* dst_i[5] = {hr.userid, hr.gender, hr.source, hr.matchedid, hr.status};
      for (int k = 0; k < 5; ++k) HIP_CHECK(hipMemcpyAsync(dst_i[k] + o, src_i[k], n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(hr.rating + o, bd.rating, n * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(hr.progress + o, bd.progress, n * 4, hipMemcpyDeviceToDevice, s));
    }
    for (int r = 0; r < rows; ++r) {
      tok[r] = r * 2 * S + retrieval_token[u0 + r];
      ra[r] = slots ? slots[2 * group_medium[group[u0 + r]]] : -1;
    }
    HIP_CHECK(hipMemcpyAsync(d_sel, tok.data(), (size_t)rows * 4, hipMemcpyHostToDevice, s));
    RC(model_infer_device(m, 0, slots ? ra.data() : nullptr, d_sel, rows, Q + (size_t)u0 * D));
    HIP_CHECK(hipStreamSynchronize(s));   // (tok / ra are rewritten by the next wave)
    ++R->forwards[0];
  }
  if (keep) {
    std::vector<float> h((size_t)nu * D);
    HIP_CHECK(hipMemcpy(h.data(), Q, h.size() * 4, hipMemcpyDeviceToHost));
    R->put("queries", h.data(), h.size());
  }

  // ---- 2. + 3. retrieval per medium, then the page window of each group
  struct Active { int g, c0, n, sidx, eidx; };
  std::vector<Active> act_m[2];
  std::vector<int32_t> total(ng, 0);
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
    SubCsr h, sl;
    if (hist_off) sub_csr(us, hist_off, hist_medium, hist_ids, hist_status, h);
    if (sel_off) sub_csr(gs, sel_off, sel_medium, sel_ids, nullptr, sl);
    std::vector<int32_t> counts(ngm);
    RetrieveDev rd; rd.d_queries = Qs;
    RC(model_retrieve_request_dev(m, mm, &rd, nq, lg.data(), ngm, hist_off ? h.off.data() : nullptr, hist_off ? h.a.data() : nullptr,
                                  hist_off ? h.b.data() : nullptr, hist_off ? h.c.data() : nullptr, sel_off ? sl.off.data() : nullptr,
                                  sel_off ? sl.a.data() : nullptr, sel_off ? sl.b.data() : nullptr, k, counts.data()));
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

  // ---- 4. + 5. ranking rows of every active group: user x chunk, waves of <= max_rows rows, media mixed
  std::vector<int> gact(ng, -1);                 // group -> index in its medium's active list
  std::vector<int> ausers_m[2];                  // users of active groups, user order
  std::vector<int64_t> rm_off(nu, 0);
  int64_t rm_n[2] = {0, 0}, rm_base[2] = {0, 0};
  std::vector<RowDesc> rows;                     // the assembled rows (full: of the users with an empty history only)
  std::vector<int32_t> row_med;
  struct CachedUser { int u, mm, c0, n; };
  std::vector<CachedUser> cached;                // full: the users ranked through the cache, in r_masked order
  for (int mm = 0; mm < 2; ++mm) {
    for (size_t a = 0; a < act_m[mm].size(); ++a) gact[act_m[mm][a].g] = (int)a;
    rm_base[mm] = mm ? rm_n[0] : 0;
    for (int u : users_m[mm]) {
      const int a = gact[group[u]];
      if (a < 0) continue;
      const Active& A = act_m[mm][a];
      ausers_m[mm].push_back(u);
      rm_off[u] = rm_base[mm] + rm_n[mm];
      const int32_t* d = user_desc + 4 * (int64_t)u;
      if (full && d[0] >= 1) cached.push_back({u, mm, A.c0, A.n});
      for (int c0 = 0; c0 < A.n && !(full && d[0] >= 1); c0 += chunk) {
        RowDesc r{};
        r.user = u; r.nh = d[0]; r.userid = d[1]; r.gender = d[2]; r.source = d[3];
        r.moff = mm ? m->V0 : 0; r.cand0 = A.c0 + c0; r.ncand = std::min(chunk, A.n - c0);
        r.rm0 = (int)(rm_off[u] + c0); r.ts = user_ts[u];
        rows.push_back(r); row_med.push_back(mm);
      }
      rm_n[mm] += A.n;
    }
  }
  // (debug channel) the ten arrays of the nr device-assembled rows under "<name>.*"
  auto keep_rows = [&](const std::string& name, const BatchDevRows& bd, int nr) -> int {
    const size_t N = (size_t)nr * S;
    std::vector<int32_t> hi(2 * N);
    std::vector<double> ht(N);
    std::vector<float> hf(N);
    HIP_CHECK(hipMemcpy(ht.data(), bd.time, N * 8, hipMemcpyDeviceToHost));
    R->put((name + ".time").c_str(), ht.data(), N);
    const char* names[6] = {".userid", ".token_mask_ids", ".gender", ".source", ".matchedid", ".status"};
    const int* srcs[6] = {bd.userid, bd.tmid, bd.gender, bd.source, bd.matchedid, bd.status};
    for (int k = 0; k < 6; ++k) {
      HIP_CHECK(hipMemcpy(hi.data(), srcs[k], N * 4, hipMemcpyDeviceToHost));
      R->put((name + names[k]).c_str(), hi.data(), N);
    }
    HIP_CHECK(hipMemcpy(hf.data(), bd.rating, N * 4, hipMemcpyDeviceToHost));
    R->put((name + ".rating").c_str(), hf.data(), N);
    HIP_CHECK(hipMemcpy(hf.data(), bd.progress, N * 4, hipMemcpyDeviceToHost));
    R->put((name + ".progress").c_str(), hf.data(), N);
    HIP_CHECK(hipMemcpy(hi.data(), bd.rope_pos, 2 * N * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < N; ++i) hi[i] = hi[2 * i] / 2;   // (the per-token positions 2 p, 2 p + 1 back to rope_input_pos)
    R->put((name + ".rope_input_pos").c_str(), hi.data(), N);
    return RSYS_OK;
  };
  // ---- 4. + 5. (full) the users with a history through the K/V cache: per wave of <= max_rows users one store forward over their history
  // rows, then their candidate rows (<= S candidates each, a user's candidates may span rows) in batches of <= max_rows rows, media mixed.
  // The host tables of a wave are read by stream-ordered copies: they stay as they are until the wave's last batch has been waited for.
  if (!cached.empty()) {
    std::vector<StoreDesc> sd(RM);
    std::vector<int32_t> s_nh(RM), s_slot(RM), s_ad(RM), c_slot(RM), c_nc(RM), c_ad(RM), crow_slot, crow_med;
    std::vector<int> s_tab((size_t)3 * RM), c_tab((size_t)3 * RM);
    std::vector<RowDesc> crows;
    int cand_forward = 0;
    auto waves = [&]() -> int {
      for (size_t w0 = 0; w0 < cached.size(); w0 += RM) {
        const int nw = (int)std::min<size_t>(RM, cached.size() - w0);
        crows.clear(); crow_slot.clear(); crow_med.clear();
        for (int r = 0; r < nw; ++r) {
          const CachedUser& cu = cached[w0 + r];
          const int32_t* d = user_desc + 4 * (int64_t)cu.u;
          sd[r] = {cu.u, d[0]};
          s_nh[r] = d[0]; s_slot[r] = r; s_ad[r] = slots ? slots[2 * cu.mm + 1] : -1;
          for (int c0 = 0; c0 < cu.n; c0 += S) {
            RowDesc q{};
            q.user = cu.u; q.nh = d[0]; q.userid = d[1]; q.gender = d[2]; q.source = d[3];
            q.moff = cu.mm ? m->V0 : 0; q.cand0 = cu.c0 + c0; q.ncand = std::min(S, cu.n - c0);
            q.rm0 = (int)(rm_off[cu.u] + c0); q.ts = user_ts[cu.u];
            crows.push_back(q); crow_slot.push_back(r); crow_med.push_back(cu.mm);
          }
        }
        BatchDevRows bd;
        RC(model_batch_device_begin(m, nw, &bd));
        HIP_CHECK(hipMemcpyAsync(d_store, sd.data(), (size_t)nw * sizeof(StoreDesc), hipMemcpyHostToDevice, s));
        tic(m, "render_store_rows");
        store_rows_kernel<<<nw, RN_THREADS, 0, s>>>(d_store, hr, S, bd);
        RN_LAUNCH_CHECK();
        toc(m);
        RC(rank_cache_store_rows(m, slots ? s_ad.data() : nullptr, s_nh.data(), s_slot.data(), s_tab.data()));   // (no host wait)
        ++R->forwards[1]; ++R->forwards_full[0];
        if (keep) {
          RC(keep_rows("store", bd, nw));
          for (int r = 0; r < nw; ++r) {
            const int32_t rec[4] = {sd[r].user, r, sd[r].nh, (int32_t)(w0 / RM)};   // user, slot, events, wave
            R->put("store.rows", rec, 4);
          }
        }
        for (size_t b0 = 0; b0 < crows.size(); b0 += RM) {
          const int nb = (int)std::min<size_t>(RM, crows.size() - b0);
          int nsel = 0;
          for (int r = 0; r < nb; ++r) {
            crows[b0 + r].sel0 = nsel; nsel += crows[b0 + r].ncand;
            c_slot[r] = crow_slot[b0 + r]; c_nc[r] = crows[b0 + r].ncand;
            c_ad[r] = slots ? slots[2 * crow_med[b0 + r] + 1] : -1;
          }
          RC(model_batch_device_begin(m, nb, &bd));
          HIP_CHECK(hipMemcpyAsync(d_rows, crows.data() + b0, (size_t)nb * sizeof(RowDesc), hipMemcpyHostToDevice, s));
          tic(m, "render_cand_rows");
          cand_rows_kernel<<<nb, RN_THREADS, 0, s>>>(d_rows, S, cand, bd, d_sel);
          RN_LAUNCH_CHECK();
          toc(m);
          RC(rank_cache_candidates_rows(m, slots ? c_ad.data() : nullptr, c_slot.data(), c_nc.data(), c_tab.data(), bd.rope_pos, d_sel, nsel, pred));
          tic(m, "render_rank_scatter");
          rank_scatter_kernel<<<nb, RN_THREADS, 0, s>>>(d_rows, pred, rm);
          RN_LAUNCH_CHECK();
          toc(m);
          HIP_CHECK(hipStreamSynchronize(s));   // (the row tables are rewritten by the next batch)
          ++R->forwards[1]; ++R->forwards_full[1];
          if (keep) {
            RC(keep_rows("cand", bd, nb));
            std::vector<int32_t> hi((size_t)nsel);
            HIP_CHECK(hipMemcpy(hi.data(), d_sel, (size_t)nsel * 4, hipMemcpyDeviceToHost));
            R->put("cand.token_index", hi.data(), (size_t)nsel);
            for (int r = 0; r < nb; ++r) {
              const RowDesc& q = crows[b0 + r];
              const int32_t rec[7] = {q.user, group[q.user], q.cand0, q.ncand, r, cand_forward, 0};   // ..., row in batch, candidate forward, kind 0 = cached
              R->put("rows", rec, 7);
            }
          }
          ++cand_forward;
        }
      }
      return RSYS_OK;
    };
    const int rc = waves();
    if (rc != RSYS_OK) { (void)hipStreamSynchronize(s); return rc; }   // (copies enqueued above read this block's vectors)
  }
  if (!rows.empty() && n_prefix) {   // the history part of the rows: uploaded once, per user
    HIP_CHECK(hipMemcpyAsync(pf_time, pb->time, (size_t)n_prefix * 8, hipMemcpyHostToDevice, s));
    const int32_t* src_i[7] = {pb->userid, pb->token_mask_ids, pb->gender, pb->source, pb->matchedid, pb->status, pb->rope_input_pos};
    for (int k = 0; k < 7; ++k) HIP_CHECK(hipMemcpyAsync(pf_i[k], src_i[k], (size_t)n_prefix * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(pf_f[0], pb->rating, (size_t)n_prefix * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(pf_f[1], pb->progress, (size_t)n_prefix * 4, hipMemcpyHostToDevice, s));
  }
  for (size_t r0 = 0; r0 < rows.size(); r0 += RM) {
    const int nr = (int)std::min<size_t>(RM, rows.size() - r0);
    int nsel = 0;
    for (int r = 0; r < nr; ++r) {
      rows[r0 + r].sel0 = nsel; nsel += rows[r0 + r].ncand;
      ra[r] = slots ? slots[2 * row_med[r0 + r] + 1] : -1;
    }
    BatchDevRows bd;
    RC(model_batch_device_begin(m, nr, &bd));
    HIP_CHECK(hipMemcpyAsync(d_rows, rows.data() + r0, (size_t)nr * sizeof(RowDesc), hipMemcpyHostToDevice, s));
    tic(m, "render_rank_rows");
    rank_rows_kernel<<<nr, RN_THREADS, 0, s>>>(d_rows, pf, P, S, cand, bd, d_sel);
    RN_LAUNCH_CHECK();
    toc(m);
    RC(model_infer_device(m, 1, slots ? ra.data() : nullptr, d_sel, nsel, pred));
    tic(m, "render_rank_scatter");
    rank_scatter_kernel<<<nr, RN_THREADS, 0, s>>>(d_rows, pred, rm);
    RN_LAUNCH_CHECK();
    toc(m);
    HIP_CHECK(hipStreamSynchronize(s));   // (ra is rewritten by the next wave)
    ++R->forwards[1];
    if (full) ++R->forwards_full[2];
    if (keep) {
      std::vector<int32_t> hi((size_t)std::max(nsel, 1));
      RC(keep_rows("batch", bd, nr));
      HIP_CHECK(hipMemcpy(hi.data(), d_sel, (size_t)nsel * 4, hipMemcpyDeviceToHost));
      R->put("token_index", hi.data(), (size_t)nsel);
      for (int r = 0; r < nr; ++r) {
        const RowDesc& d = rows[r0 + r];
        const int32_t rec[7] = {d.user, group[d.user], d.cand0, d.ncand, r, (int32_t)(r0 / RM), 1};   // user, group, first candidate, count, row in wave, wave (, full: kind 1 = assembled)
        R->put("rows", rec, full ? 7 : 6);
      }
    }
  }

  // ---- 6. ranking + reranking per medium; the pages come back
  std::vector<std::vector<int32_t>> pages(ng);
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
    SubCsr h;
    if (hist_off) sub_csr(us, hist_off, hist_medium, hist_ids, hist_status, h);
    std::vector<int32_t> page(std::max<int64_t>(np, 1)), kp(keep ? coff[na] : 0);
    std::vector<float> kr(keep ? coff[na] : 0);
    RankDev rd{cand + act[0].c0, Qs, rm + rm_base[mm], plo.data(), phi.data(), poff.data(), page.data(), keep ? kr.data() : nullptr,
               keep ? kp.data() : nullptr};
    const int have = coef_have ? coef_have[mm] : 0;
    const float* cf = coefs ? coefs + 4 * mm : nullptr;
    RC(model_rank_request_dev(m, mm, na, coff.data(), &rd, pk.data(), pen.data(), nq, lg.data(), rm_n[mm], hist_off ? h.off.data() : nullptr,
                              hist_off ? h.a.data() : nullptr, hist_off ? h.b.data() : nullptr, hist_off ? h.c.data() : nullptr,
                              (have & 1) ? cf : nullptr, (have & 2) ? cf + 1 : nullptr, (have & 2) ? cf[3] : 0.f));
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
  if (keep)   // (every key is present, maybe empty)
    for (const char* k : {"rows", "groups", "rm_users", "r", "picks", "r_masked", "token_index", "batch.time", "batch.userid",
                          "batch.token_mask_ids", "batch.gender", "batch.source", "batch.matchedid", "batch.status", "batch.rating",
                          "batch.progress", "batch.rope_input_pos"})
      R->kept[k];
  if (keep && full)
    for (const char* pre : {"store", "cand"}) {
      for (const char* k : {".time", ".userid", ".token_mask_ids", ".gender", ".source", ".matchedid", ".status", ".rating", ".progress",
                            ".rope_input_pos"})
        R->kept[std::string(pre) + k];
      R->kept[std::string(pre) + (pre[0] == 's' ? ".rows" : ".token_index")];
    }
  // ---- outputs, once everything has succeeded
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

int model_render_request(Model* m, int32_t ng, const int32_t* group_medium, const int64_t* offset, const int32_t* limit, const float* penalties,
                         int64_t nu, const int32_t* group, const rsys_batch* rb, const int32_t* retrieval_token, const rsys_batch* pb,
                         int32_t P, const int32_t* user_desc, const double* user_ts, const int32_t* slots, const int64_t* hist_off,
                         const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status, const int64_t* sel_off,
                         const int32_t* sel_medium, const int32_t* sel_ids, const int32_t* coef_have, const float* coefs, int32_t* ids_out,
                         int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out) {
  return render_run(m, false, ng, group_medium, offset, limit, penalties, nu, group, rb, retrieval_token, pb, P, user_desc, user_ts, slots,
                    hist_off, hist_medium, hist_ids, hist_status, sel_off, sel_medium, sel_ids, coef_have, coefs, ids_out, ids_cap, ids_offsets,
                    total_out);
}

int model_render_request_full(Model* m, int32_t ng, const int32_t* group_medium, const int64_t* offset, const int32_t* limit,
                              const float* penalties, int64_t nu, const int32_t* group, const rsys_batch* rb, const int32_t* retrieval_token,
                              const int32_t* user_desc, const double* user_ts, const int32_t* slots, const int64_t* hist_off,
                              const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status, const int64_t* sel_off,
                              const int32_t* sel_medium, const int32_t* sel_ids, const int32_t* coef_have, const float* coefs,
                              int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out) {
  return render_run(m, true, ng, group_medium, offset, limit, penalties, nu, group, rb, retrieval_token, nullptr, 0, user_desc, user_ts, slots,
                    hist_off, hist_medium, hist_ids, hist_status, sel_off, sel_medium, sel_ids, coef_have, coefs, ids_out, ids_cap, ids_offsets,
                    total_out);
}

}  // namespace rsys
