// extern "C" surface of librsys_hip.so (declared in include/rsys.h).
#include <algorithm>
#include <dlfcn.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>

#include "comm.hpp"
#include "encoder_handle.hpp"
#include "model_internal.hpp"

namespace rsys {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace rsys

using namespace rsys;

struct rsys_model { Model* m; };
struct rsys_optimizer { Optimizer o; };

#define CHECK_HANDLE(h) do { if ((h) == nullptr) { set_error("null handle"); return RSYS_ERR_ARG; } } while (0)

namespace {
// The pending query weights (rsys_query_weights_set) and text queries (rsys_query_texts_set, both media) of a model in the hands of the
// request entry point that consumes them: moved out of the model on entry, so the model holds none again on every return path, success
// and error alike.  The texts' rows stay in the model's buffers, which only the next rsys_query_texts_set rewrites.  for_medium /
// for_page check them against the call -- texts first, then weights -- and hand the call its QueryWeights / QueryTexts.
struct PendingQueries {
  std::vector<float> user, sel;
  bool have_user, have_sel;
  struct Set { QueryTexts q; std::vector<int32_t> group, row; } t[2];
  explicit PendingQueries(Model* m) : user(std::move(m->qw_user)), sel(std::move(m->qw_sel)), have_user(m->qw_have_user), have_sel(m->qw_have_sel) {
    m->qw_user.clear(); m->qw_sel.clear();
    m->qw_have_user = m->qw_have_sel = false;
    for (int mm = 0; mm < 2; ++mm) {
      TextSet& ts = m->qtexts[mm];
      Set& o = t[mm];
      o.group = std::move(ts.group);
      o.group.resize((size_t)ts.n);
      o.row.resize((size_t)ts.n);
      for (int i = 0; i < ts.n; ++i) o.row[i] = i;
      o.q.n = ts.n; o.q.z = ts.z; o.q.lse = ts.lse; o.q.d_w = ts.d_w; o.q.ldz = ts.ldz;
      o.q.row = o.row.data(); o.q.group = o.group.data();
      ts.n = 0; ts.group.clear();
    }
  }
  // a call on one medium: a text set of the other medium is refused, every text's group must be one of the call's.  A medium or a
  // group count the call itself will refuse is left to it: no texts are handed on.
  int for_medium(const char* who, int medium, int64_t n_users, bool accept_sel, const int64_t* sel_off, int64_t ng, QueryWeights* qw,
                 QueryTexts* qt) const {
    *qt = QueryTexts{};
    if ((t[0].q.n || t[1].q.n) && (medium == 0 || medium == 1) && ng >= 1 && ng <= 4096) {
      ARG_CHECK(t[1 - medium].q.n == 0, std::string(who) + ": text queries are pending for a medium this call does not serve (rsys_query_texts_set)");
      for (int32_t g : t[medium].group) ARG_CHECK(g >= 0 && g < ng, std::string(who) + ": the group of a pending text query must be in [0, n_groups)");
      *qt = t[medium].q;
    }
    return check_weights(who, n_users, accept_sel, sel_off, ng, qw);
  }
  // a page pipeline: every text's group must be one of the call's and of the set's medium
  int for_page(const char* who, const int32_t* group_medium, int64_t n_users, const int64_t* sel_off, int64_t ng, QueryWeights* qw,
               QueryTexts qt[2]) const {
    qt[0] = qt[1] = QueryTexts{};
    if ((t[0].q.n || t[1].q.n) && group_medium != nullptr && ng >= 1 && ng <= 4096) {
      for (int mm = 0; mm < 2; ++mm)
        for (int32_t g : t[mm].group) {
          ARG_CHECK(g >= 0 && g < ng, std::string(who) + ": the group of a pending text query must be in [0, n_groups)");
          ARG_CHECK(group_medium[g] == mm, std::string(who) + ": a pending text query belongs to a group of another medium (rsys_query_texts_set)");
        }
      qt[0] = t[0].q; qt[1] = t[1].q;
    }
    return check_weights(who, n_users, true, sel_off, ng, qw);
  }

 private:
  // the counts against the call's: n_users (-1: the call accepts no user weights) and sel_off[n_groups] (accept_sel == false: the
  // call accepts no selected-item weights).  A group count the call itself will refuse is left to it: no weights are handed on.
  int check_weights(const char* who, int64_t n_users, bool accept_sel, const int64_t* sel_off, int64_t ng, QueryWeights* out) const {
    *out = QueryWeights{};
    if (have_user) {
      ARG_CHECK(n_users >= 0, std::string(who) + ": the pending query weights hold user weights, which this call does not take");
      ARG_CHECK((int64_t)user.size() == n_users, std::string(who) + ": the pending user weights do not match the call's users (rsys_query_weights_set n_users)");
      out->user = user.data();
    }
    if (have_sel) {
      ARG_CHECK(accept_sel, std::string(who) + ": the pending query weights hold selected-item weights, which this call does not take");
      if (ng < 1 || ng > 4096) { *out = QueryWeights{}; return RSYS_OK; }
      const int64_t nsel = sel_off ? sel_off[ng] : 0;
      ARG_CHECK((int64_t)sel.size() == nsel, std::string(who) + ": the pending selected-item weights do not match sel_offsets[n_groups] (rsys_query_weights_set n_sel)");
      out->sel = sel.data();
    }
    return RSYS_OK;
  }
};
}  // namespace

extern "C" {

const char* rsys_version(void) { return "recommendersystem_amd 0.1 (gfx950)"; }

size_t rsys_last_error(char* buf, size_t n) {
  if (buf && n) { strncpy(buf, g_err.c_str(), n - 1); buf[n - 1] = 0; }
  return g_err.size();
}

int32_t rsys_device_count(int32_t* n) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  if (n) *n = c;
  return RSYS_OK;
}
int32_t rsys_device_synchronize(void) { HIP_CHECK(hipDeviceSynchronize()); return RSYS_OK; }

int32_t rsys_model_create(const rsys_config* cfg, int32_t device, rsys_model** out) {
  switches_parse();
  Model* m = nullptr;
  int rc = model_create(cfg, device, &m);
  if (rc) return rc;
  *out = new rsys_model{m};
  return RSYS_OK;
}
int32_t rsys_model_destroy(rsys_model* h) { if (!h) return RSYS_OK; model_destroy(h->m); delete h; return RSYS_OK; }
int32_t rsys_model_init_random(rsys_model* h, uint64_t seed) { CHECK_HANDLE(h); return model_init_random(h->m, seed); }
int32_t rsys_model_load_metadata(rsys_model* h, const float* t, int64_t V, int64_t M) { CHECK_HANDLE(h); ARG_CHECK(t, "null table"); return model_load_metadata(h->m, t, V, M); }
int32_t rsys_model_random_metadata(rsys_model* h, uint64_t seed) { CHECK_HANDLE(h); return model_random_metadata(h->m, seed); }
int32_t rsys_model_set_rope(rsys_model* h, const float* c, const float* s, int64_t n) { CHECK_HANDLE(h); ARG_CHECK(c && s, "null table"); return model_set_rope(h->m, c, s, n); }

int32_t rsys_param_count(rsys_model* h, int32_t* n) { CHECK_HANDLE(h); *n = (int32_t)h->m->tensors.size(); return RSYS_OK; }
int32_t rsys_param_info(rsys_model* h, int32_t i, char* name, size_t cap, int64_t shape[2], int32_t* ndim, int32_t* trainable) {
  CHECK_HANDLE(h);
  ARG_CHECK(i >= 0 && i < (int)h->m->tensors.size(), "parameter index");
  const TensorInfo& t = h->m->tensors[i];
  if (name && cap) { strncpy(name, t.name.c_str(), cap - 1); name[cap - 1] = 0; }
  if (shape) { if (t.ndim == 1) { shape[0] = t.cols; shape[1] = 0; } else { shape[0] = t.rows; shape[1] = t.cols; } }
  if (ndim) *ndim = t.ndim;
  if (trainable) *trainable = t.trainable ? 1 : 0;
  return RSYS_OK;
}
int32_t rsys_param_get(rsys_model* h, const char* name, float* out, int64_t n) { CHECK_HANDLE(h); ARG_CHECK(name && out, "null"); return model_param_io(h->m, name, out, nullptr, n, 0); }
int32_t rsys_param_set(rsys_model* h, const char* name, const float* in, int64_t n) { CHECK_HANDLE(h); ARG_CHECK(name && in, "null"); return model_param_io(h->m, name, nullptr, in, n, 0); }
int32_t rsys_grad_get(rsys_model* h, const char* name, float* out, int64_t n) { CHECK_HANDLE(h); ARG_CHECK(name && out, "null"); return model_param_io(h->m, name, out, nullptr, n, 1); }
int32_t rsys_zero_grad(rsys_model* h) {
  CHECK_HANDLE(h);
  HIP_CHECK(hipSetDevice(h->m->device));
  HIP_CHECK(hipMemsetAsync(h->m->G, 0, h->m->n_total * 4, h->m->stream));
  h->m->table_grads_pending = false;
  h->m->gE_clean[0] = h->m->gE_clean[1] = true;
  return RSYS_OK;
}

int32_t rsys_batch_upload(rsys_model* h, const rsys_batch* b) { CHECK_HANDLE(h); return model_batch_upload(h->m, b); }
int32_t rsys_batch_rows(rsys_model* h, int32_t* rows_out) { CHECK_HANDLE(h); ARG_CHECK(rows_out, "null"); *rows_out = h->m->cur_rows; return RSYS_OK; }
int32_t rsys_batch_upload_trimmed(rsys_model* h, const rsys_batch* b, int32_t row_len) { CHECK_HANDLE(h); return model_batch_upload_trimmed(h->m, b, row_len); }
int32_t rsys_batch_row_length(rsys_model* h, int32_t* row_len_out) {
  CHECK_HANDLE(h); ARG_CHECK(row_len_out, "null");
  *row_len_out = h->m->cur_rows > 0 ? h->m->S : 0;
  return RSYS_OK;
}
int32_t rsys_serving_pack_set(rsys_model* h, int32_t on) { CHECK_HANDLE(h); h->m->serving_pack = on != 0; return RSYS_OK; }
int32_t rsys_serving_pack_get(rsys_model* h, int32_t* on_out) { CHECK_HANDLE(h); ARG_CHECK(on_out, "null"); *on_out = h->m->serving_pack ? 1 : 0; return RSYS_OK; }
int32_t rsys_serving_pack_ranking_set(rsys_model* h, int32_t on) { CHECK_HANDLE(h); h->m->serving_pack_ranking = on != 0; return RSYS_OK; }
int32_t rsys_serving_pack_ranking_get(rsys_model* h, int32_t* on_out) { CHECK_HANDLE(h); ARG_CHECK(on_out, "null"); *on_out = h->m->serving_pack_ranking ? 1 : 0; return RSYS_OK; }
int32_t rsys_serving_compact_top_set(rsys_model* h, int32_t on) { CHECK_HANDLE(h); h->m->serving_compact_top = on == 2 || on == 3 ? on : (on != 0 ? 1 : 0); return RSYS_OK; }   // (2 / 3: the measurement values of model.hpp)
int32_t rsys_serving_compact_top_get(rsys_model* h, int32_t* on_out) { CHECK_HANDLE(h); ARG_CHECK(on_out, "null"); *on_out = h->m->serving_compact_top; return RSYS_OK; }
int32_t rsys_serving_trim_set(rsys_model* h, int32_t on) { CHECK_HANDLE(h); h->m->serving_trim = on != 0; return RSYS_OK; }
int32_t rsys_serving_trim_get(rsys_model* h, int32_t* on_out) { CHECK_HANDLE(h); ARG_CHECK(on_out, "null"); *on_out = h->m->serving_trim ? 1 : 0; return RSYS_OK; }
int32_t rsys_batch_prefetch(rsys_model* h, const rsys_batch* b) { CHECK_HANDLE(h); return model_batch_prefetch(h->m, b); }
int32_t rsys_batch_swap(rsys_model* h) { CHECK_HANDLE(h); return model_batch_swap(h->m); }

int32_t rsys_forward_backward(rsys_model* h, int32_t evaluate, const float task_w[4], float grad_scale, uint64_t seed, uint64_t step) {
  CHECK_HANDLE(h);
  return model_forward_backward(h->m, evaluate, task_w, grad_scale, seed, step);
}

int32_t rsys_losses_get(rsys_model* h, float losses_out[12], float wsum_out[4]) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  float acc[16], st[8];
  HIP_CHECK(hipMemcpyAsync(acc, m->loss_acc, 16 * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_CHECK(hipMemcpyAsync(st, m->stats, 8 * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  for (int ti = 0; ti < 4; ++ti) {
    float ws = fmaxf(st[2 * ti], 1e-8f);  // w_sum over the selected positions, clamp(min=1e-8) (model.py:392,515)
    for (int k = 0; k < 3; ++k) losses_out[3 * ti + k] = acc[3 * ti + k] / ws;
    if (wsum_out) wsum_out[ti] = st[2 * ti + 1];
  }
  return RSYS_OK;
}

// The reference's loop adds each step's losses into device tensors and reads them once per epoch (transformer.py:245-262, 279-283):
// push parks the finished step's loss sums and weight sums in a device ring (a 96-byte copy on the model's stream, no host wait),
// drain reads every parked step back in order with the arithmetic of rsys_losses_get.
int32_t rsys_losses_push(rsys_model* h) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  if (m->loss_ring == nullptr) HIP_CHECK(hipMalloc((void**)&m->loss_ring, (size_t)Model::loss_ring_cap * 24 * 4));
  if (m->loss_ring_n >= Model::loss_ring_cap) { set_error("rsys_losses_push: ring full (rsys_losses_drain first)"); return RSYS_ERR_STATE; }
  float* slot = m->loss_ring + (size_t)m->loss_ring_n * 24;
  HIP_CHECK(hipMemcpyAsync(slot, m->loss_acc, 16 * 4, hipMemcpyDeviceToDevice, m->stream));
  HIP_CHECK(hipMemcpyAsync(slot + 16, m->stats, 8 * 4, hipMemcpyDeviceToDevice, m->stream));
  m->loss_ring_n += 1;
  return RSYS_OK;
}

int32_t rsys_losses_drain(rsys_model* h, float* losses_out, float* wsum_out, int32_t cap, int32_t* n_out) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  ARG_CHECK(losses_out && wsum_out && n_out, "rsys_losses_drain: null output");
  ARG_CHECK(cap >= m->loss_ring_n, "rsys_losses_drain: output holds fewer steps than are parked");
  HIP_CHECK(hipSetDevice(m->device));
  const int n = m->loss_ring_n;
  *n_out = n;
  if (n == 0) return RSYS_OK;
  std::vector<float> host((size_t)n * 24);
  HIP_CHECK(hipMemcpyAsync(host.data(), m->loss_ring, host.size() * 4, hipMemcpyDeviceToHost, m->stream));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  for (int s = 0; s < n; ++s) {
    const float* acc = host.data() + (size_t)s * 24; const float* st = acc + 16;
    for (int ti = 0; ti < 4; ++ti) {
      const float ws = fmaxf(st[2 * ti], 1e-8f);
      for (int k = 0; k < 3; ++k) losses_out[(size_t)s * 12 + 3 * ti + k] = acc[3 * ti + k] / ws;
      wsum_out[(size_t)s * 4 + ti] = st[2 * ti + 1];
    }
  }
  m->loss_ring_n = 0;
  return RSYS_OK;
}

int32_t rsys_head_rows_get(rsys_model* h, int32_t out[4]) {
  CHECK_HANDLE(h);
  HIP_CHECK(hipSetDevice(h->m->device));
  HIP_CHECK(hipStreamSynchronize(h->m->stream));
  HIP_CHECK(hipMemcpy(out, h->m->npos, 16, hipMemcpyDeviceToHost));
  return RSYS_OK;
}

int32_t rsys_item_table(rsys_model* h, float* out, int64_t n) { CHECK_HANDLE(h); ARG_CHECK(out, "null"); return model_item_table(h->m, out, n); }
int32_t rsys_retrieve_topk(rsys_model* h, int32_t medium, const float* queries, int64_t n_queries, const int32_t* group, int32_t n_groups,
                           const float* prior, const int64_t* excl_offsets, const int32_t* excl_ids, int32_t k, int32_t* ids_out,
                           float* scores_out, int32_t* counts_out) {
  CHECK_HANDLE(h);
  return model_retrieve_topk(h->m, medium, queries, n_queries, group, n_groups, prior, excl_offsets, excl_ids, k, ids_out, scores_out,
                             counts_out);
}
// the fp32 item-table rows of `medium` become the frozen features of an item-similarity or search handle on the model's device
static int32_t features_from_model(void* sink, rsys_model* h, int32_t medium) {
  CHECK_HANDLE(h);
  if (sink == nullptr) { set_error("null handle"); return RSYS_ERR_ARG; }
  const float* rows = nullptr; int64_t Vm = 0; int D = 0;
  RC(model_item_table_device(h->m, medium, &rows, &Vm, &D));
  return enc_features_from_device((EncoderCore*)sink, rows, Vm, D, h->m->device);
}
int32_t rsys_sim_features_from_model(void* sim, rsys_model* h, int32_t medium) { return features_from_model(sim, h, medium); }
int32_t rsys_search_features_from_model(void* search, rsys_model* h, int32_t medium) { return features_from_model(search, h, medium); }
int32_t rsys_retrieve_target_rank(rsys_model* h, int32_t medium, const float* queries, int64_t n_queries, const int32_t* targets,
                                  const int64_t* excl_offsets, const int32_t* excl_ids, int32_t* rank_out, float* logp_out) {
  CHECK_HANDLE(h);
  return model_retrieve_target_rank(h->m, medium, queries, n_queries, targets, excl_offsets, excl_ids, rank_out, logp_out);
}
int32_t rsys_retrieve_relations_set(rsys_model* h, int32_t medium, int32_t kind, int64_t n_rows, int64_t n_cols, const int64_t* colptr,
                                    const int32_t* rowval, const float* nzval) {
  CHECK_HANDLE(h);
  return model_retrieve_relations_set(h->m, medium, kind, n_rows, n_cols, colptr, rowval, nzval);
}
int32_t rsys_retrieve_similarity_set(rsys_model* h, int32_t medium, int64_t dim, const float* emb, const float* crossproject) {
  CHECK_HANDLE(h);
  return model_retrieve_similarity_set(h->m, medium, dim, emb, crossproject);
}
int32_t rsys_retrieve_released_set(rsys_model* h, int32_t medium, const uint8_t* mask) {
  CHECK_HANDLE(h);
  return model_retrieve_released_set(h->m, medium, mask);
}
int32_t rsys_query_weights_set(rsys_model* h, const float* user_w, int64_t n_users, const float* sel_w, int64_t n_sel) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  m->qw_user.clear(); m->qw_sel.clear();
  m->qw_have_user = m->qw_have_sel = false;   // (a refused call holds nothing)
  ARG_CHECK(n_users >= 0 && n_sel >= 0, "query_weights_set: counts must be >= 0");
  ARG_CHECK((user_w != nullptr) == (n_users > 0) && (sel_w != nullptr) == (n_sel > 0), "query_weights_set: an array and its count go together ((NULL, 0) = unweighted)");
  for (int64_t i = 0; i < n_users; ++i) ARG_CHECK(std::isfinite(user_w[i]), "query_weights_set: weights must be finite");
  for (int64_t i = 0; i < n_sel; ++i) ARG_CHECK(std::isfinite(sel_w[i]), "query_weights_set: weights must be finite");
  if (n_users) { m->qw_user.assign(user_w, user_w + n_users); m->qw_have_user = true; }
  if (n_sel) { m->qw_sel.assign(sel_w, sel_w + n_sel); m->qw_have_sel = true; }
  return RSYS_OK;
}
int32_t rsys_query_weights_pending(rsys_model* h, int64_t out[2]) {
  CHECK_HANDLE(h);
  ARG_CHECK(out, "query_weights_pending: null output");
  out[0] = h->m->qw_have_user ? (int64_t)h->m->qw_user.size() : 0;
  out[1] = h->m->qw_have_sel ? (int64_t)h->m->qw_sel.size() : 0;
  return RSYS_OK;
}
int32_t rsys_query_texts_set(rsys_model* h, void* search, int32_t medium, const float* x, int64_t n_texts, const int32_t* group,
                             const float* w) {
  CHECK_HANDLE(h);
  return model_query_texts_set(h->m, search, medium, x, n_texts, group, w);
}
int32_t rsys_query_texts_pending(rsys_model* h, int64_t out[2]) {
  CHECK_HANDLE(h);
  ARG_CHECK(out, "query_texts_pending: null output");
  out[0] = h->m->qtexts[0].n; out[1] = h->m->qtexts[1].n;
  return RSYS_OK;
}
int32_t rsys_retrieve_request(rsys_model* h, int32_t medium, const float* queries, int64_t n_queries, const int32_t* group, int32_t n_groups,
                              const int64_t* hist_offsets, const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                              const int64_t* sel_offsets, const int32_t* sel_medium, const int32_t* sel_ids, int32_t k, int32_t* ids_out,
                              float* scores_out, int32_t* counts_out) {
  CHECK_HANDLE(h);
  const PendingQueries pq(h->m);
  Request rq{queries, n_queries, group, n_groups, {hist_offsets, hist_medium, hist_ids, hist_status}, {sel_offsets, sel_medium, sel_ids}};
  RC(pq.for_medium("retrieve_request", medium, n_queries, true, sel_offsets, n_groups, &rq.qw, &rq.qt));
  return model_retrieve_request(h->m, medium, rq, k, nullptr, nullptr, ids_out, scores_out, counts_out);
}
int32_t rsys_retrieve_window(rsys_model* h, int32_t medium, const float* queries, int64_t n_queries, const int32_t* group, int32_t n_groups,
                             const int64_t* hist_offsets, const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                             const int64_t* sel_offsets, const int32_t* sel_medium, const int32_t* sel_ids, const int64_t* win_start,
                             const int32_t* win_len, int32_t* ids_out, float* scores_out, int32_t* counts_out, int32_t* total_out) {
  CHECK_HANDLE(h);
  const PendingQueries pq(h->m);
  Request rq{queries, n_queries, group, n_groups, {hist_offsets, hist_medium, hist_ids, hist_status}, {sel_offsets, sel_medium, sel_ids}};
  RC(pq.for_medium("retrieve_window", medium, n_queries, true, sel_offsets, n_groups, &rq.qw, &rq.qt));
  const RetrieveWin win{win_start, win_len, total_out};
  return model_retrieve_request(h->m, medium, rq, 0, &win, nullptr, ids_out, scores_out, counts_out);
}
int32_t rsys_render_items(rsys_model* h, int32_t n_groups, const int32_t* group_medium, const int64_t* offset, const int32_t* limit,
                          const float* penalties, const int64_t* sel_offsets, const int32_t* sel_medium, const int32_t* sel_ids,
                          int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out) {
  CHECK_HANDLE(h);
  const PendingQueries pq(h->m);
  QueryWeights qw;
  QueryTexts qt[2];
  RC(pq.for_page("render_items", group_medium, -1, sel_offsets, n_groups, &qw, qt));
  return model_render_items(h->m, n_groups, group_medium, offset, limit, penalties, {sel_offsets, sel_medium, sel_ids}, ids_out, ids_cap,
                            ids_offsets, total_out, qw.sel, qt);
}
int32_t rsys_rank_related_set(rsys_model* h, int32_t medium, int64_t n, const int64_t* colptr, const int32_t* rowval, const float* nzval) {
  CHECK_HANDLE(h);
  return model_rank_related_set(h->m, medium, n, colptr, rowval, nzval);
}
int32_t rsys_rank_request(rsys_model* h, int32_t medium, int32_t n_groups, const int64_t* cand_offsets, const int32_t* cand_ids,
                          const int32_t* partialk, const float* penalties, const float* queries, int64_t n_users, const int32_t* group,
                          const float* r_masked, int64_t n_r_masked, const int64_t* hist_offsets, const int32_t* hist_medium,
                          const int32_t* hist_ids, const int32_t* hist_status, const float* retrieval_coef, const float* rating_coefs,
                          float rating_mean, const float* r_in, int32_t* ids_out, float* r_out) {
  CHECK_HANDLE(h);
  const PendingQueries pq(h->m);
  Request rq{queries, n_users, group, n_groups, {hist_offsets, hist_medium, hist_ids, hist_status}, {}};
  RC(pq.for_medium("rank_request", medium, n_users, false, nullptr, n_groups, &rq.qw, &rq.qt));
  const RankCands rc{cand_offsets, cand_ids, partialk, penalties, r_masked, n_r_masked, retrieval_coef, rating_coefs, rating_mean, r_in};
  return model_rank_request(h->m, medium, rq, rc, ids_out, r_out);
}
// The one body of rsys_render_request (full == false) and rsys_render_request_full (full == true; no ranking prefixes): the C
// arguments, in their order, become a RenderArgs, and the pending weights and texts join it.
static int32_t render_page(rsys_model* h, bool full, int32_t n_groups, const int32_t* group_medium, const int64_t* offset, const int32_t* limit,
                           const float* penalties, int64_t n_users, const int32_t* group, const rsys_batch* retrieval_rows,
                           const int32_t* retrieval_token, const rsys_batch* ranking_prefix, int32_t prefix_stride, const int32_t* user_desc,
                           const double* user_ts, const int32_t* adapter_slots, const HistoryList& hist, const SelectedList& sel,
                           const int32_t* coef_have, const float* coefs, int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets,
                           int32_t* total_out) {
  CHECK_HANDLE(h);
  const PendingQueries pq(h->m);
  RenderArgs a{};
  RC(pq.for_page("render_request", group_medium, n_users, sel.off, n_groups, &a.qw, a.qt));
  a.full = full; a.ng = n_groups; a.group_medium = group_medium; a.offset = offset; a.limit = limit; a.penalties = penalties;
  a.nu = n_users; a.group = group; a.rb = retrieval_rows; a.retrieval_token = retrieval_token; a.pb = ranking_prefix; a.P = prefix_stride;
  a.user_desc = user_desc; a.user_ts = user_ts; a.slots = adapter_slots;
  a.hist_list = hist; a.sel_list = sel; a.coef_have = coef_have; a.coefs = coefs;
  a.ids_out = ids_out; a.ids_cap = ids_cap; a.ids_offsets = ids_offsets; a.total_out = total_out;
  return model_render(h->m, a);
}
int32_t rsys_render_request(rsys_model* h, int32_t n_groups, const int32_t* group_medium, const int64_t* offset, const int32_t* limit,
                            const float* penalties, int64_t n_users, const int32_t* group, const rsys_batch* retrieval_rows,
                            const int32_t* retrieval_token, const rsys_batch* ranking_prefix, int32_t prefix_stride, const int32_t* user_desc,
                            const double* user_ts, const int32_t* adapter_slots, const int64_t* hist_offsets, const int32_t* hist_medium,
                            const int32_t* hist_ids, const int32_t* hist_status, const int64_t* sel_offsets, const int32_t* sel_medium,
                            const int32_t* sel_ids, const int32_t* coef_have, const float* coefs, int32_t* ids_out, int64_t ids_cap,
                            int64_t* ids_offsets, int32_t* total_out) {
  return render_page(h, false, n_groups, group_medium, offset, limit, penalties, n_users, group, retrieval_rows, retrieval_token, ranking_prefix,
                     prefix_stride, user_desc, user_ts, adapter_slots, {hist_offsets, hist_medium, hist_ids, hist_status},
                     {sel_offsets, sel_medium, sel_ids}, coef_have, coefs, ids_out, ids_cap, ids_offsets, total_out);
}
int32_t rsys_render_request_full(rsys_model* h, int32_t n_groups, const int32_t* group_medium, const int64_t* offset, const int32_t* limit,
                                 const float* penalties, int64_t n_users, const int32_t* group, const rsys_batch* retrieval_rows,
                                 const int32_t* retrieval_token, const int32_t* user_desc, const double* user_ts, const int32_t* adapter_slots,
                                 const int64_t* hist_offsets, const int32_t* hist_medium, const int32_t* hist_ids, const int32_t* hist_status,
                                 const int64_t* sel_offsets, const int32_t* sel_medium, const int32_t* sel_ids, const int32_t* coef_have,
                                 const float* coefs, int32_t* ids_out, int64_t ids_cap, int64_t* ids_offsets, int32_t* total_out) {
  return render_page(h, true, n_groups, group_medium, offset, limit, penalties, n_users, group, retrieval_rows, retrieval_token, nullptr, 0,
                     user_desc, user_ts, adapter_slots, {hist_offsets, hist_medium, hist_ids, hist_status}, {sel_offsets, sel_medium, sel_ids},
                     coef_have, coefs, ids_out, ids_cap, ids_offsets, total_out);
}
int32_t rsys_render_debug_keep(rsys_model* h, int32_t on) { CHECK_HANDLE(h); return render_debug_keep(h->m, on); }
int32_t rsys_render_debug_get(rsys_model* h, const char* key, void* out, int64_t cap, int64_t* bytes) {
  CHECK_HANDLE(h);
  return render_debug_get(h->m, key, out, cap, bytes);
}
int32_t rsys_rank_gram_get(rsys_model* h, int32_t medium, int32_t n_groups, const int64_t* cand_offsets, const int32_t* cand_ids, float* out,
                           int64_t n_out) {
  CHECK_HANDLE(h);
  return model_rank_gram(h->m, medium, n_groups, cand_offsets, cand_ids, out, n_out);
}
int32_t rsys_model_set_deterministic(rsys_model* h, int32_t on) { CHECK_HANDLE(h); return model_set_deterministic(h->m, on); }
int32_t rsys_infer(rsys_model* h, int32_t task, float* out, int64_t n) { CHECK_HANDLE(h); ARG_CHECK(out, "null"); return model_infer(h->m, task, nullptr, 0, out, n); }
int32_t rsys_infer_select(rsys_model* h, int32_t task, const int32_t* token_index, int64_t n_tokens, float* out, int64_t n) {
  CHECK_HANDLE(h); ARG_CHECK(out && token_index && n_tokens >= 1, "null or empty selection");
  return model_infer(h->m, task, token_index, n_tokens, out, n);
}
int32_t rsys_adapter_set(rsys_model* h, int32_t slot, const char* name, const float* in, int64_t n) {
  CHECK_HANDLE(h); ARG_CHECK(name && in, "null");
  return adapter_io(h->m, slot, name, nullptr, in, n);
}
int32_t rsys_adapter_get(rsys_model* h, int32_t slot, const char* name, float* out, int64_t n) {
  CHECK_HANDLE(h); ARG_CHECK(name && out, "null");
  return adapter_io(h->m, slot, name, out, nullptr, n);
}
int32_t rsys_adapter_clear(rsys_model* h, int32_t slot) { CHECK_HANDLE(h); return adapter_clear(h->m, slot); }
int32_t rsys_adapter_slots(rsys_model* h, int32_t* mask_out) { CHECK_HANDLE(h); return adapter_slots(h->m, mask_out); }
// training through the bank: the reference's four sequential finetune jobs (Finetune/run.jl:9-13; transformer.py:591-597,
// 259-276) as one pass over a batch whose rows name their slot and task
int32_t rsys_adapter_train_enable(rsys_model* h, float dropout) { CHECK_HANDLE(h); return adapter_train_enable(h->m, dropout); }   // model.py:238
int32_t rsys_adapter_forward_backward(rsys_model* h, int32_t evaluate, const int32_t* row_slot, const int32_t* row_task, float grad_scale, uint64_t seed,
                                      uint64_t step) {   // model.py:417-435, 493-529; train.py:259-272
  CHECK_HANDLE(h);
  return adapter_forward_backward(h->m, evaluate, row_slot, row_task, grad_scale, seed, step);
}
int32_t rsys_adapter_forward_backward_packed(rsys_model* h, int32_t evaluate, const int32_t* seg, int32_t n_seg, float grad_scale, uint64_t seed,
                                             uint64_t step) {   // the same on packed rows: slot and task per segment
  CHECK_HANDLE(h);
  return adapter_forward_backward_packed(h->m, evaluate, seg, n_seg, grad_scale, seed, step);
}
int32_t rsys_adapter_grad_get(rsys_model* h, int32_t slot, const char* name, float* out, int64_t n) { CHECK_HANDLE(h); return adapter_grad_get(h->m, slot, name, out, n); }
int32_t rsys_adapter_zero_grad(rsys_model* h) { CHECK_HANDLE(h); return adapter_zero_grad(h->m); }   // train.py:275
int32_t rsys_adapter_adamw_step(rsys_model* h, float lr0, float beta1, float beta2, float eps, float wd, const float* per_slot, int32_t n_slots,
                                float* norms_out) {   // train.py:273-275, transformer.py:285-298
  CHECK_HANDLE(h);
  return adapter_adamw_step(h->m, lr0, beta1, beta2, eps, wd, per_slot, n_slots, norms_out);
}
int32_t rsys_adapter_adamw_state_get(rsys_model* h, int32_t slot, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step_out) {
  CHECK_HANDLE(h);
  ARG_CHECK(name == nullptr || (exp_avg && exp_avg_sq), "null");
  return adapter_adamw_state_io(h->m, slot, name, exp_avg, exp_avg_sq, nullptr, nullptr, n, step_out, -1);
}
int32_t rsys_adapter_adamw_state_set(rsys_model* h, int32_t slot, const char* name, const float* exp_avg, const float* exp_avg_sq, int64_t n, int32_t step) {
  CHECK_HANDLE(h);
  ARG_CHECK(name == nullptr || (exp_avg && exp_avg_sq), "null");
  return adapter_adamw_state_io(h->m, slot, name, nullptr, nullptr, exp_avg, exp_avg_sq, n, nullptr, step);
}
int32_t rsys_infer_select_adapters(rsys_model* h, int32_t task, const int32_t* row_adapter, const int32_t* token_index, int64_t n_tokens, float* out,
                                   int64_t n) {
  CHECK_HANDLE(h); ARG_CHECK(out && token_index && n_tokens >= 1, "null or empty selection");
  ARG_CHECK(row_adapter, "row_adapter is null (rsys_infer_select runs the base model)");
  return model_infer_adapters(h->m, task, row_adapter, token_index, n_tokens, out, n);
}
int32_t rsys_infer_select_tiles(rsys_model* h, int32_t task, const int32_t* tile_adapter, const int32_t* token_index, int64_t n_tokens, float* out,
                                int64_t n) {
  CHECK_HANDLE(h); ARG_CHECK(out && token_index && n_tokens >= 1, "null or empty selection");
  return model_infer_tiles(h->m, task, tile_adapter, token_index, n_tokens, out, n);
}

int32_t rsys_rank_cache_reserve(rsys_model* h, int32_t n_slots) { CHECK_HANDLE(h); return model_rank_cache_reserve(h->m, n_slots); }
int32_t rsys_rank_cache_store(rsys_model* h, const int32_t* row_adapter, const int32_t* n_hist, const int32_t* slot) {
  CHECK_HANDLE(h);
  return model_rank_cache_store(h->m, row_adapter, n_hist, slot);
}
int32_t rsys_rank_cache_candidates(rsys_model* h, const int32_t* row_adapter, const int32_t* slot, const int32_t* n_cand, float* out) {
  CHECK_HANDLE(h);
  return model_rank_cache_candidates(h->m, row_adapter, slot, n_cand, out);
}
int32_t rsys_rank_cache_store_packed(rsys_model* h, const int32_t* seg_adapter, int32_t n_seg, const int32_t* seg) {
  CHECK_HANDLE(h);
  return model_rank_cache_store_packed(h->m, seg_adapter, n_seg, seg);
}
int32_t rsys_rank_cache_candidates_packed(rsys_model* h, const int32_t* seg_adapter, int32_t n_seg, const int32_t* seg, float* out) {
  CHECK_HANDLE(h);
  return model_rank_cache_candidates_packed(h->m, seg_adapter, n_seg, seg, out);
}
int32_t rsys_rank_cache_get(rsys_model* h, int32_t layer, int32_t slot, void* out, int64_t bytes) {
  CHECK_HANDLE(h);
  return model_rank_cache_get(h->m, layer, slot, out, bytes);
}

int32_t rsys_trunk_output_get(rsys_model* h, float* out, int64_t n) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  const int64_t cnt = (int64_t)2 * m->cur_rows * m->S * m->D;
  ARG_CHECK(n == cnt, "trunk output has rows*2S*D floats");
  HIP_CHECK(hipSetDevice(m->device));
  { const int rc_ = model_materialise_trunk_output(m); if (rc_ != RSYS_OK) return rc_; }   // (a training pass computed it at the selected tokens only)
  HIP_CHECK(hipStreamSynchronize(m->stream));
  if (!m->bf16_mode) { HIP_CHECK(hipMemcpy(out, m->out, cnt * 4, hipMemcpyDeviceToHost)); return RSYS_OK; }
  std::vector<unsigned short> host(cnt);
  HIP_CHECK(hipMemcpy(host.data(), m->out, cnt * 2, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < cnt; ++i) { uint32_t u = (uint32_t)host[i] << 16; memcpy(&out[i], &u, 4); }
  return RSYS_OK;
}

// Parity read-back of the integer / index paths of the last forward (tests only; synchronises):
//   "masked.token_mask_ids" | "masked.matchedid" | "masked.status"   int32 [rows*S]   mask_tokens outputs (model.py:417-462)
//   "masked.rating" | "masked.progress"                              f32   [rows*S]
//   "masked.<m>.<watch|rating>.<label|weight|position>"              f32 / f32 / int32 [rows*S]
//   "idx.<task>"   int32 [mask_topk*rows]  flat positions chosen for task = medium*2 + metric (model.py:501-513)
//   "npos"         int32 [4]               positive-weight positions per task
//   "tokens.userid" | "tokens.token_mask_ids"   int32 [rows*2S]  interleaved per-token arrays (model.py:468-469)
//   "embed.x0"     f32 [rows*2S*D]         interleaved input embeddings (even rows: gathered item rows)
//   "table.fused"  f32 [(V+1)*D]           the fused item table the gather reads (row V = mask row)
//   "host_syncs" int32 [2]: blocking host waits inside the last rsys_forward_backward {stream drains, event waits}
//   "forward.tokens" int64 [1]: tokens the last trunk forward ran over = rows * 2 * row length of the resident batch (S here is that length)
//   "top.n" int32 [1] | "top.sel" int32 [top.cap] | "top.slot" int32 [rows*2S] | "top.cap" int32 [1]: compact top of the last training
//                  pass (model.hpp sparse_top): number of selected tokens, the sorted tokens, token -> compact row (-1: not selected)
//   "infer.top" int32 [1] | "infer.top_rows" int32 [1]: what the last inference pass did under rsys_serving_compact_top_set -- 0 dense,
//                  1 compact tail behind the dense attention, 2 compact tail behind attn_sel_kernel, 3 store stopped at K | V -- and the rows its tail ran on
int32_t rsys_debug_get(rsys_model* h, const char* key, void* out, int64_t bytes) {
  CHECK_HANDLE(h);
  ARG_CHECK(key && out, "null");
  Model* m = h->m;
  ARG_CHECK(m->cur_rows > 0, "no batch uploaded");
  HIP_CHECK(hipSetDevice(m->device));
  const int64_t N = (int64_t)m->cur_rows * m->S;
  const std::string k(key);
  const void* src = nullptr; int64_t n = 0;   // n: bytes
  const BatchDev& b = m->bd;
  if (k == "masked.token_mask_ids") { src = b.m_tmid; n = N * 4; }
  else if (k == "masked.matchedid") { src = b.m_matchedid; n = N * 4; }
  else if (k == "masked.status") { src = b.m_status; n = N * 4; }
  else if (k == "masked.rating") { src = b.m_rating; n = N * 4; }
  else if (k == "masked.progress") { src = b.m_progress; n = N * 4; }
  else if (k == "npos") { src = m->npos; n = 16; }
  else if (k == "tokens.userid") { src = m->uid_t; n = 2 * N * 4; }
  else if (k == "tokens.token_mask_ids") { src = m->tm_t; n = 2 * N * 4; }
  else if (k == "embed.x0") { src = m->x0; n = 2 * N * m->D * 4; }
  else if (k == "table.fused") { src = m->F32; n = (int64_t)m->TR * m->D * 4; }
  else if (k == "forward.tokens") { ARG_CHECK(bytes == 8, "forward.tokens: one int64"); *(int64_t*)out = m->fwd_tokens; return RSYS_OK; }
  else if (k == "host_syncs") {   // blocking host waits inside the last rsys_forward_backward: {stream drains, waits on the early-counts event}
    ARG_CHECK(bytes == 8, "host_syncs: two int32"); ((int32_t*)out)[0] = m->host_stream_syncs; ((int32_t*)out)[1] = m->host_event_waits; return RSYS_OK; }
  else if (k.compare(0, 4, "act.") == 0 && k.size() > 6) {   // act.<layer>.<x|xn|qkv|O|h|hn|ab|g>: a saved activation of the last forward (T-typed ones as stored)
    const size_t dot = k.find('.', 4);
    const int l = atoi(k.substr(4, dot - 4).c_str());
    const std::string f = dot == std::string::npos ? "" : k.substr(dot + 1);
    ARG_CHECK(l >= 0 && l < m->L, "act: layer index");
    const Model::LayerAct& a = m->la[l];
    const int64_t NT = 2 * N, e = m->esz;
    if (f == "x") { src = a.x; n = NT * m->D * 4; } else if (f == "h") { src = a.h; n = NT * m->D * 4; }
    else if (f == "xn") { src = a.xn; n = NT * m->D * e; } else if (f == "hn") { src = a.hn; n = NT * m->D * e; }
    else if (f == "qkv") { src = a.qkv; n = NT * m->Nqkv * e; } else if (f == "O") { src = a.O; n = NT * m->D * e; }
    else if (f == "ab") { src = a.ab; n = NT * 2 * m->Ip * e; } else if (f == "g") { src = a.g; n = NT * m->Ip * e; }
  }
  else if (k.compare(0, 3, "dw.") == 0 && !m->dwb.empty()) {   // dw.<layer>.<gxt|dab|dht|dqkv>: the dY operands the deferred weight gradients kept
    const size_t dot = k.find('.', 3);
    const int l = atoi(k.substr(3, dot - 3).c_str());
    const std::string f = dot == std::string::npos ? "" : k.substr(dot + 1);
    ARG_CHECK(l >= 0 && l < m->L, "dw: layer index");
    const Model::DwOperands& o = m->dwb[l];
    const int64_t NT = 2 * N;
    if (f == "gxt" && o.gxt) { src = o.gxt; n = NT * m->D * 2; } else if (f == "dab" && o.dab) { src = o.dab; n = NT * 2 * m->Ip * 2; }
    else if (f == "dht" && o.dht) { src = o.dht; n = NT * m->D * 2; } else if (f == "dqkv" && o.dqkv) { src = o.dqkv; n = NT * m->Nqkv * 2; }
  }
  else if (k.compare(0, 7, "f8keep.") == 0 && !m->f8_keep.empty()) {   // f8keep.<layer>.<0|1|2>: outputs of w13_dx, o_dx, qkv_dx (RSYS_F8_DEBUG_KEEP=1)
    const size_t dot = k.find('.', 7);
    const int l = atoi(k.substr(7, dot - 7).c_str()), j = dot == std::string::npos ? -1 : atoi(k.substr(dot + 1).c_str());
    ARG_CHECK(l >= 0 && l < m->L && j >= 0 && j < 3, "f8keep: layer / product index");
    src = m->f8_keep[(size_t)l * 3 + j]; n = 2 * N * m->D * 2;
  }
  else if (k == "f8.aamax" && m->fp8) { src = m->f8_aamax; n = (int64_t)m->L * F8_AMAX_SHARDS * F8_AMAX_SHARD * 4; }
  else if (k == "f8.wamax" && m->fp8) { src = m->f8_wamax; n = (int64_t)m->L * 8 * 4; }
  else if (k == "f8.desc" && m->fp8) { src = m->f8_desc; n = (int64_t)m->L * 8 * 32 * 4; }
  else if (k == "top.cap") { ARG_CHECK(bytes == 4, "top.cap: one int32"); *(int32_t*)out = m->top_is_sparse ? m->ctop_cap : 0; return RSYS_OK; }
  else if (k == "infer.top") { ARG_CHECK(bytes == 4, "infer.top: one int32"); *(int32_t*)out = m->infer_top; return RSYS_OK; }
  else if (k == "infer.top_rows") { ARG_CHECK(bytes == 4, "infer.top_rows: one int32"); *(int32_t*)out = m->infer_top_rows; return RSYS_OK; }
  else if (k == "top.n" && m->top_is_sparse) { src = m->c_n; n = 4; }
  else if (k == "top.sel" && m->top_is_sparse) { src = m->c_sel; n = (int64_t)m->ctop_cap * 4; }
  else if (k == "top.slot" && m->top_is_sparse) { src = m->c_slot; n = 2 * N * 4; }
  else if (k.size() == 5 && k.compare(0, 4, "idx.") == 0 && k[4] >= '0' && k[4] <= '3') { src = m->idx[k[4] - '0']; n = (int64_t)m->K * m->cur_rows * 4; }
  else if (k.compare(0, 7, "masked.") == 0 && k.size() > 9 && (k[7] == '0' || k[7] == '1') && k[8] == '.') {
    const int med = k[7] - '0';
    const std::string rest = k.substr(9);
    const size_t dot = rest.find('.');
    if (dot != std::string::npos) {
      const std::string metric = rest.substr(0, dot), field = rest.substr(dot + 1);
      const int mi = metric == "watch" ? 0 : metric == "rating" ? 1 : -1;
      if (mi >= 0) {
        const int ti = med * 2 + mi;
        if (field == "label") src = b.m_label[ti]; else if (field == "weight") src = b.m_weight[ti]; else if (field == "position") src = b.m_position[ti];
        n = N * 4;
      }
    }
  }
  if (src == nullptr) { set_error(std::string("rsys_debug_get: unknown key ") + key); return RSYS_ERR_ARG; }
  ARG_CHECK(bytes == n, "rsys_debug_get: buffer size does not match the array");
  HIP_CHECK(hipStreamSynchronize(m->stream));
  HIP_CHECK(hipMemcpy(out, src, (size_t)n, hipMemcpyDeviceToHost));
  return RSYS_OK;
}

int32_t rsys_clip_grad_norm(rsys_model* h, float max_norm, float* norm_out) { CHECK_HANDLE(h); return model_clip(h->m, max_norm, norm_out); }

// Replica-consistency words of this rank's parameters (transformer.py:678-682): the flat fp32 parameter buffer -- of a
// row-sharded model everything but its table rows, which differ between the ranks by construction -- as {fp64 sum, fp64 sum of
// squares, low and high 32 bits of a position-weighted integer sum of the bit patterns}.  Synchronises.
int32_t rsys_param_checksum(rsys_model* h, double out[4]) {
  CHECK_HANDLE(h);
  ARG_CHECK(out != nullptr, "rsys_param_checksum: out is NULL");
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  double* scratch = nullptr;
  HIP_CHECK(hipMalloc((void**)&scratch, (size_t)checksum_scratch_doubles() * 8));
  long long ranges[4] = {0, m->n_total, 0, 0};
  int nr = 1;
  if (m->sharded && m->sh_world > 1) {
    ranges[1] = m->o_E; ranges[2] = m->o_E + ((int64_t)m->TR * m->D + 7) / 8 * 8; ranges[3] = m->n_total; nr = 2;
  }
  double* out_dev = scratch + checksum_scratch_doubles() - 4;
  int rc = launch_checksum(m->P, ranges, nr, scratch, out_dev, m->stream);
  if (rc == RSYS_OK) {
    hipError_t e = hipMemcpyAsync(out, out_dev, 32, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) { set_error(std::string("rsys_param_checksum: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  }
  (void)hipFree(scratch);
  return rc;
}

int32_t rsys_adamw_create(rsys_model* h, float lr, float b1, float b2, float eps, float wd, rsys_optimizer** out) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  rsys_optimizer* o = new rsys_optimizer();
  o->o.m = m; o->o.device = m->device; o->o.lr = lr; o->o.b1 = b1; o->o.b2 = b2; o->o.eps = eps; o->o.wd = wd;
  HIP_CHECK(hipMalloc((void**)&o->o.mom, m->n_total * 4));
  HIP_CHECK(hipMalloc((void**)&o->o.var, m->n_total * 4));
  HIP_CHECK(hipMemset(o->o.mom, 0, m->n_total * 4));
  HIP_CHECK(hipMemset(o->o.var, 0, m->n_total * 4));
  *out = o;
  return RSYS_OK;
}
int32_t rsys_adamw_destroy(rsys_optimizer* o) {
  if (!o) return RSYS_OK;
  hipSetDevice(o->o.device);
  hipDeviceSynchronize();   // (not the model's stream: the model may already be gone)
  hipFree(o->o.mom); hipFree(o->o.var);
  if (o->o.z_tailbuf) hipFree(o->o.z_tailbuf);
  delete o;
  return RSYS_OK;
}
int32_t rsys_adamw_step(rsys_optimizer* o, float lr_factor, float clip, float grad_div) {
  CHECK_HANDLE(o);
  ARG_CHECK(!o->o.zero1, "this optimizer is partitioned (rsys_adamw_set_zero1): step it with rsys_adamw_step_zero1");
  return optimizer_step(&o->o, lr_factor, clip, grad_div);
}
int32_t rsys_adamw_set_zero1(rsys_optimizer* o, int32_t rank, int32_t world) { CHECK_HANDLE(o); return optimizer_set_zero1(&o->o, rank, world); }
int32_t rsys_adamw_step_zero1(rsys_optimizer* o, rsys_comm* c, float lr_factor, float clip, float grad_div) {
  CHECK_HANDLE(o); CHECK_HANDLE(c);
  Model* m = o->o.m;
  m->grad_bucket_hook = nullptr; m->reduced.clear(); m->early_reduced = 0;   // (no early buckets in this mode: the step reduces the whole gradient)
  m->gemm_flags &= ~GEMM_ONE_WG_PER_TILE;
  return optimizer_step_zero1(&o->o, c, lr_factor, clip, grad_div);
}

static int adam_state_io(rsys_optimizer* o, const char* name, float* m_out, float* v_out, const float* m_in, const float* v_in, int64_t n) {
  Model* m = o->o.m;
  auto it = m->by_name.find(name);
  if (it == m->by_name.end()) { set_error(std::string("unknown parameter: ") + name); return RSYS_ERR_ARG; }
  const TensorInfo& t = m->tensors[it->second];
  ARG_CHECK(!t.frozen_table, "frozen table has no optimizer state");
  ARG_CHECK(n == t.rows * t.cols, "element count");
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  const int64_t int_rows = (t.map == MAP_DIRECT) ? t.rows : 2 * m->Ip;
  std::vector<float> host((size_t)int_rows * t.ld);
  // ZeRO-1 (optimizer_set_zero1): this rank holds the moments of flat elements [rank * chunk, (rank + 1) * chunk) at local offset 0 and --
  // the last rank -- of the tail [chunk * world, n_opt) behind them.  A read returns the rank's part of the tensor and zeros elsewhere
  // (the parts of all ranks are disjoint: AdamW.state_dict sums them over the ranks' HostGroup); a write keeps the rank's part.
  struct Piece { int64_t g_lo, g_hi, local; };
  std::vector<Piece> pieces;
  const int64_t t_lo = t.off, t_hi = t.off + (int64_t)host.size();
  if (o->o.zero1) {
    const int64_t chunk = o->o.z_chunk, own = o->o.z_rank * chunk, tail_lo = chunk * o->o.z_world;
    pieces.push_back({own, own + chunk, 0});
    if (o->o.z_rank == o->o.z_world - 1 && o->o.z_tail > 0) pieces.push_back({tail_lo, tail_lo + o->o.z_tail, chunk});
  }
  for (int which = 0; which < 2; ++which) {
    float* zbase = which == 0 ? o->o.mom : o->o.var;
    float* base = zbase + t.off;
    float* out = which == 0 ? m_out : v_out;
    const float* in = which == 0 ? m_in : v_in;
    if (o->o.zero1) {
      std::fill(host.begin(), host.end(), 0.f);
      auto irow = [&](int64_t r) { return t.map == MAP_W1 ? (r / 16) * 32 + r % 16 : t.map == MAP_W3 ? (r / 16) * 32 + 16 + r % 16 : r; };
      if (in) for (int64_t r = 0; r < t.rows; ++r) memcpy(host.data() + irow(r) * t.ld, in + r * t.cols, t.cols * 4);
      for (const Piece& pc : pieces) {
        const int64_t a = std::max(pc.g_lo, t_lo), b = std::min(pc.g_hi, t_hi);
        if (a >= b) continue;
        if (in) {
          // (a W1 / W3 tensor shares its interleaved rows with its partner: write this tensor's rows only)
          if (t.map == MAP_DIRECT) HIP_CHECK(hipMemcpy(zbase + pc.local + (a - pc.g_lo), host.data() + (a - t_lo), (size_t)(b - a) * 4, hipMemcpyHostToDevice));
          else
            for (int64_t r = 0; r < t.rows; ++r) {
              const int64_t ra = std::max(a, t_lo + irow(r) * t.ld), rb = std::min(b, t_lo + irow(r) * t.ld + t.cols);
              if (ra < rb) HIP_CHECK(hipMemcpy(zbase + pc.local + (ra - pc.g_lo), host.data() + (ra - t_lo), (size_t)(rb - ra) * 4, hipMemcpyHostToDevice));
            }
        } else {
          HIP_CHECK(hipMemcpy(host.data() + (a - t_lo), zbase + pc.local + (a - pc.g_lo), (size_t)(b - a) * 4, hipMemcpyDeviceToHost));
        }
      }
      if (out) for (int64_t r = 0; r < t.rows; ++r) memcpy(out + r * t.cols, host.data() + irow(r) * t.ld, t.cols * 4);
      continue;
    }
    HIP_CHECK(hipMemcpy(host.data(), base, host.size() * 4, hipMemcpyDeviceToHost));
    auto irow = [&](int64_t r) { return t.map == MAP_W1 ? (r / 16) * 32 + r % 16 : t.map == MAP_W3 ? (r / 16) * 32 + 16 + r % 16 : r; };
    if (out) for (int64_t r = 0; r < t.rows; ++r) memcpy(out + r * t.cols, host.data() + irow(r) * t.ld, t.cols * 4);
    if (in) {
      for (int64_t r = 0; r < t.rows; ++r) memcpy(host.data() + irow(r) * t.ld, in + r * t.cols, t.cols * 4);
      HIP_CHECK(hipMemcpy(base, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    }
  }
  return RSYS_OK;
}
int32_t rsys_adamw_state_get(rsys_optimizer* o, const char* name, float* m_out, float* v_out, int64_t n, int32_t* step) {
  CHECK_HANDLE(o);
  if (step) *step = o->o.step;
  if (name == nullptr) return RSYS_OK;
  return adam_state_io(o, name, m_out, v_out, nullptr, nullptr, n);
}
int32_t rsys_adamw_state_set(rsys_optimizer* o, const char* name, const float* m_in, const float* v_in, int64_t n, int32_t step) {
  CHECK_HANDLE(o);
  if (step >= 0) o->o.step = step;
  if (name == nullptr) return RSYS_OK;
  return adam_state_io(o, name, nullptr, nullptr, m_in, v_in, n);
}

// ---------------------------------------------------------------- communicator
int32_t rsys_comm_unique_id(uint8_t id_buf[128]) { return comm_unique_id(id_buf); }
int32_t rsys_comm_init(const uint8_t id_buf[128], int32_t rank, int32_t world, int32_t device, rsys_comm** out) {
  switches_parse();
  ARG_CHECK(id_buf && out, "null");
  return comm_init_rccl(id_buf, rank, world, device, out);
}
int32_t rsys_comm_destroy(rsys_comm* c) { return comm_destroy(c); }
int32_t rsys_comm_debug_delay(rsys_comm* c, int32_t microseconds) { CHECK_HANDLE(c); return comm_debug_delay(c, microseconds); }

// in-process rank group (tests of the multi-rank partition arithmetic on one GPU): `world` ranks of THIS process on one
// device, each driven by its own host thread; rsys_comm_init_local gives rank r its communicator
int32_t rsys_local_group_create(int32_t world, int32_t device, void** out) {
  ARG_CHECK(out && world >= 1 && world <= 16, "in-process group: 1..16 ranks");
  LocalGroup* g = new LocalGroup();
  g->world = world; g->device = device; g->slot.resize(world);
  *out = g;
  return RSYS_OK;
}
int32_t rsys_local_group_destroy(void* group) {
  if (!group) return RSYS_OK;
  LocalGroup* g = (LocalGroup*)group;
  { std::lock_guard<std::mutex> lk(g->mu); if (g->refs > 0) { set_error("in-process group: close its communicators first (rsys_comm_destroy)"); return RSYS_ERR_STATE; } }
  delete g;
  return RSYS_OK;
}
int32_t rsys_comm_init_local(void* group, int32_t rank, rsys_comm** out) {
  switches_parse();
  ARG_CHECK(group && out, "null");
  return comm_init_local((LocalGroup*)group, rank, out);
}

// DDP's bucketed gradient all-reduce (train.py:678-682, 272) on the communicator's own stream.
//
// rsys_set_grad_sync(model, comm) before the backward of the last micro-step arms the early buckets: the trunk backward
// hands over each >= 25 MB run of finished per-layer weight gradients (reverse layer order), and its all-reduce is
// enqueued behind an event while the backward of the lower layers is still running.  rsys_allreduce_grads then reduces
// whatever is left (heads, small tensors, the item table and the metadata projection, final only after the token
// scatter) and makes the compute stream wait for the last bucket before the optimizer reads the gradients.
static int reduce_range(Model* m, rsys_comm* c, int64_t lo, int64_t hi) {
  const int64_t bucket = 16 * 1024 * 1024;  // floats
  for (int64_t o = lo; o < hi; o += bucket) {
    const int64_t n = std::min(bucket, hi - o);
    RC(comm_all_reduce_f32(c, m->G + o, (size_t)n, COMM_SUM, c->stream));
  }
  if (hi > lo) m->bucket_log.push_back({lo, hi, m->bucket_phase});
  return RSYS_OK;
}

int32_t rsys_set_grad_sync(rsys_model* h, rsys_comm* c) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  m->reduced.clear();
  m->bucket_log.clear(); m->bucket_phase = 0;
  m->grad_bucket_hook = nullptr;
  m->table_head_hook = nullptr;
  m->gemm_flags &= ~GEMM_ONE_WG_PER_TILE;
  if (!comm_active(c) || m->cfg.finetune) return RSYS_OK;
  if (m->split_table && m->bf16_mode && !m->sharded) {
    // the head part of the item table's gradient, complete when heads() returns: summed over the ranks into tbl_R while the trunk
    // backward runs (G[E] itself keeps the local gradient: the token scatter and the metadata-projection gradient still need it)
    m->table_head_hook = [m, c]() -> int {
      // first on the communicator's stream, a whole trunk backward before the tail needs it on the host: the ranks' maximum of the
      // distinct ids of their resident batches = the rows per rank the tail's gathers will carry
      RC(model_split_table_arm(m, c));
      HIP_CHECK(hipEventRecord(c->ev_ready, m->stream));
      HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_ready, 0));
      const int64_t n = (int64_t)m->TR * m->D, bucket = 16 * 1024 * 1024;
      for (int64_t o = 0; o < n; o += bucket)
        RC(comm_all_reduce_f32_to(c, m->G + m->o_E + o, m->tbl_R + o, (size_t)std::min(bucket, n - o), c->stream));
      // The collective READS G[E] on the communicator's stream; the trunk backward WRITES G[E] on the model's stream (the token rows,
      // model.hip backward_trunk).  That write waits for this event: free when the reduce is done by then, and otherwise what keeps a
      // slow link from folding some ranks' token rows into tbl_R, which the tail would then add a second time.
      HIP_CHECK(hipEventRecord(c->ev_head, c->stream));
      m->bucket_log.push_back({m->o_E, m->o_E + n, 3});
      m->split_head_event = c->ev_head;
      m->split_head_reduced = true;
      return RSYS_OK;
    };
  }
  m->grad_bucket_hook = [m, c](int64_t lo, int64_t hi) -> int {
    hi = std::min(hi, m->n_opt);
    if (lo >= hi) return RSYS_OK;
    HIP_CHECK(hipEventRecord(c->ev_ready, m->stream));
    HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_ready, 0));
    int rc = reduce_range(m, c, lo, hi);
    if (rc) return rc;
    m->reduced.emplace_back(lo, hi);
    return RSYS_OK;
  };
  return RSYS_OK;
}

int32_t rsys_model_set_split_table_reduce(rsys_model* h, int32_t on) {
  CHECK_HANDLE(h);
  return model_split_table_enable(h->m, on);
}

int32_t rsys_model_set_shard_comm(rsys_model* h, rsys_comm* c) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  ARG_CHECK(m->sharded, "the model's item table is replicated (rsys_config.table_shard_world == 0)");
  ARG_CHECK((c == nullptr && m->sh_world == 1) || (c != nullptr && c->world == m->sh_world && c->rank == m->sh_rank),
            "the communicator's rank / world must equal the model's table_shard_rank / table_shard_world");
  m->shard_comm = c;
  return RSYS_OK;
}
int32_t rsys_table_rows(rsys_model* h, int64_t* lo, int64_t* hi) {
  CHECK_HANDLE(h);
  if (lo) *lo = h->m->row_lo;
  if (hi) *hi = h->m->row_lo + h->m->TR;
  return RSYS_OK;
}

int32_t rsys_allreduce_grads(rsys_model* h, rsys_comm* c) {
  CHECK_HANDLE(h); CHECK_HANDLE(c);
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  if (m->grad_bucket_hook == nullptr && m->table_head_hook == nullptr) m->bucket_log.clear();   // (not armed: nothing of this step is in the log yet)
  m->grad_bucket_hook = nullptr;   // one backward per arming
  m->table_head_hook = nullptr;
  const bool split = m->split_head_reduced && comm_active(c) && model_finalize_splittable(m);   // (else: G[E] holds the whole local gradient, the dense path is right)
  m->split_head_reduced = false;
  m->split_head_event = nullptr;   // (everything below is ordered behind the head reduce on the communicator's stream itself)
  m->gemm_flags &= ~GEMM_ONE_WG_PER_TILE;   // the optimizer waits for the reduction: nothing after this call overlaps with it
  m->early_reduced = 0;
  for (auto& r : m->reduced) m->early_reduced += r.second - r.first;
  if (!comm_active(c)) { m->reduced.clear(); return model_finalize_grads(m); }
  // what the early buckets have not covered, ascending
  std::vector<std::pair<int64_t, int64_t>> done = m->reduced, rem;
  m->reduced.clear();
  // row-sharded table: a rank's table rows already hold the gradient of EVERY rank's loss (vocabulary-parallel head, row
  // exchange of the token gradients): they are not part of the dense all-reduce
  if (m->sharded) done.emplace_back(m->o_E, m->o_E + (int64_t)m->TR * m->D);
  if (split) {   // split table reduce: tbl_R + the ranks' token rows instead
    done.emplace_back(m->o_E, m->o_E + (int64_t)m->TR * m->D);
    m->early_reduced += (int64_t)m->TR * m->D;
  }
  std::sort(done.begin(), done.end());
  int64_t at = 0;
  for (auto& r : done) { if (r.first > at) rem.emplace_back(at, r.first); at = std::max(at, r.second); }
  if (at < m->n_opt) rem.emplace_back(at, m->n_opt);
  auto reduce_rest = [&](int64_t lo, int64_t hi) -> int {
    for (auto& r : rem) {
      const int64_t a = std::max(r.first, lo), b = std::min(r.second, hi);
      if (a < b) { int rc = reduce_range(m, c, a, b); if (rc) return rc; }
    }
    return RSYS_OK;
  };
  if (model_finalize_splittable(m)) {
    // The last piece of the backward -- the metadata-projection gradient dWp = dF^T Meta, a ~2 ms GEMM on a bf16 copy
    // of dF -- runs on the model's stream while the communication stream already reduces everything else (80 % of the
    // bytes are dF itself, final since the token scatter); dWp follows when the GEMM is done.
    int64_t wo = 0, wn = 0;
    int rc = model_finalize_stage(m, 1, &wo, &wn);
    if (rc) return rc;
    HIP_CHECK(hipEventRecord(c->ev_ready, m->stream));
    HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_ready, 0));
    m->bucket_phase = 1;
    if (split) {   // nothing reads the local G[E] any more (stage 1 made the operand copy and the bias gradient): it becomes the sum
      int64_t tail_rows = 0;
      rc = model_split_table_tail(m, c, c->stream, &tail_rows);
      if (rc) return rc;
      m->bucket_log.push_back({0, (int64_t)c->world * tail_rows * (m->D + 1), 4});
    }
    rc = reduce_rest(0, std::min(wo, m->n_opt));
    if (rc) return rc;
    rc = reduce_rest(std::min(wo + wn, m->n_opt), m->n_opt);
    if (rc) return rc;
    rc = model_finalize_stage(m, 2, nullptr, nullptr);
    if (rc) return rc;
    HIP_CHECK(hipEventRecord(c->ev_ready, m->stream));
    HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_ready, 0));
    m->bucket_phase = 2;
    rc = reduce_rest(wo, std::min(wo + wn, m->n_opt));
    if (rc) return rc;
  } else {
    m->bucket_phase = 1;
    int rc = model_finalize_grads(m);
    if (rc) return rc;
    HIP_CHECK(hipEventRecord(c->ev_ready, m->stream));
    HIP_CHECK(hipStreamWaitEvent(c->stream, c->ev_ready, 0));
    rc = reduce_rest(0, m->n_opt);
    if (rc) return rc;
  }
  HIP_CHECK(hipEventRecord(c->ev_done, c->stream));
  HIP_CHECK(hipStreamWaitEvent(m->stream, c->ev_done, 0));
  return RSYS_OK;
}
int32_t rsys_grad_sync_early(rsys_model* h, int64_t* n) { CHECK_HANDLE(h); ARG_CHECK(n, "null"); *n = h->m->early_reduced; return RSYS_OK; }
int32_t rsys_grad_sync_schedule(rsys_model* h, int64_t* out, int32_t cap, int32_t* n_out) {
  CHECK_HANDLE(h); ARG_CHECK(out && n_out && cap >= 0, "null");
  const auto& log = h->m->bucket_log;
  const int n = (int)std::min<size_t>(log.size(), (size_t)cap);
  for (int i = 0; i < n; ++i) { out[3 * i] = log[i].lo; out[3 * i + 1] = log[i].hi; out[3 * i + 2] = log[i].phase; }
  *n_out = (int32_t)log.size();
  return RSYS_OK;
}
int32_t rsys_comm_info(rsys_comm* c, int32_t out[4]) {
  CHECK_HANDLE(c); ARG_CHECK(out, "null");
  out[0] = c->rank; out[1] = c->world;
  out[2] = c->lg ? 2 : (c->comm ? 1 : 0);     // transport: 1 = RCCL, 2 = in-process rank group (tests)
  out[3] = c->comm ? comm_rccl_version() : 0;
  return RSYS_OK;
}
int32_t rsys_allreduce_f64(rsys_comm* c, double* x, int32_t n) {
  CHECK_HANDLE(c);
  ARG_CHECK(n >= 1 && n <= 64 && x, "n in [1,64]");
  if (!comm_active(c)) return RSYS_OK;
  HIP_CHECK(hipSetDevice(c->device));
  HIP_CHECK(hipMemcpyAsync(c->scratch, x, n * 8, hipMemcpyHostToDevice, c->stream));
  RC(comm_all_reduce_f64(c, c->scratch, (size_t)n, c->stream));
  HIP_CHECK(hipMemcpyAsync(x, c->scratch, n * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  return RSYS_OK;
}
int32_t rsys_self_test(rsys_comm* c) {  // hardware_check.py:8-12
  CHECK_HANDLE(c);
  double one = 1.0;
  int rc = rsys_allreduce_f64(c, &one, 1);
  if (rc) return rc;
  if (one != (double)c->world) { set_error("all-reduce self test: sum of ones != world size"); return RSYS_ERR_COMM; }
  return RSYS_OK;
}

int32_t rsys_grad_buffer(rsys_model* h, void** p, int64_t* n) {
  CHECK_HANDLE(h);
  int rc = model_finalize_grads(h->m);
  if (rc) return rc;
  *p = h->m->G; *n = h->m->n_opt;
  return RSYS_OK;
}
int32_t rsys_param_buffer(rsys_model* h, void** p, int64_t* n) { CHECK_HANDLE(h); *p = h->m->P; *n = h->m->n_total; return RSYS_OK; }
int32_t rsys_refresh_shadow(rsys_model* h) { CHECK_HANDLE(h); return model_refresh_shadow(h->m); }

// ---------------------------------------------------------------- raw device helpers + per-op entry points (tests)
int32_t rsys_dev_alloc(void** p, size_t bytes) { HIP_CHECK(hipMalloc(p, bytes ? bytes : 16)); HIP_CHECK(hipMemset(*p, 0, bytes ? bytes : 16)); return RSYS_OK; }
int32_t rsys_dev_free(void* p) { HIP_CHECK(hipFree(p)); return RSYS_OK; }
int32_t rsys_dev_h2d(void* d, const void* s, size_t n) { HIP_CHECK(hipMemcpy(d, s, n, hipMemcpyHostToDevice)); return RSYS_OK; }
int32_t rsys_dev_d2h(void* d, const void* s, size_t n) { HIP_CHECK(hipDeviceSynchronize()); HIP_CHECK(hipMemcpy(d, s, n, hipMemcpyDeviceToHost)); return RSYS_OK; }
int32_t rsys_dev_memset(void* d, int v, size_t n) { HIP_CHECK(hipMemset(d, v, n)); return RSYS_OK; }

int32_t rsys_op_gemm(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                     int64_t ldb, int64_t ldc, int32_t a_km, int32_t b_km, int32_t a_f32, int32_t c_f32, int32_t splitk) {
  switches_parse();
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32; p.splitk = splitk < 1 ? 1 : splitk; p.alpha = 1.f;
  p.epi = p.splitk > 1 ? EPI_ATOMIC : EPI_STORE;
  if (sw().debug_epi >= 0) p.epi = sw().debug_epi;   // timing experiments only (e.g. 99 = no epilogue)
  int rc = dtype == RSYS_DTYPE_BF16 ? launch_gemm<bf16>(p, a_f32 != 0, false, a_km != 0, b_km != 0, nullptr)
                                    : launch_gemm<float>(p, false, false, a_km != 0, b_km != 0, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_gemm_rows(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                          int64_t ldb, int64_t ldc, int32_t b_km, int32_t c_f32, const int32_t* rows_dev) {
  switches_parse();
  ARG_CHECK(rows_dev != nullptr, "rsys_op_gemm_rows: rows_dev is null");
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32 != 0; p.splitk = 1; p.alpha = 1.f; p.epi = EPI_STORE; p.m_dev = rows_dev;
  if (c_f32 == 3) { p.epi = EPI_ATOMIC; p.splitk = 8; }   // the head's dEw form: fp32 C accumulated by split-K atomics
  int rc = dtype == RSYS_DTYPE_BF16 ? launch_gemm<bf16>(p, false, false, false, b_km != 0, nullptr)
                                    : launch_gemm<float>(p, false, false, false, b_km != 0, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_gemm_klimit(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                            int64_t ldb, int64_t ldc, int32_t accumulate, const int32_t* k_dev) {
  switches_parse();
  ARG_CHECK(k_dev != nullptr, "rsys_op_gemm_klimit: k_dev is null");
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = 1; p.splitk = 1; p.alpha = 1.f; p.epi = accumulate ? EPI_ACCUM : EPI_STORE; p.k_dev = k_dev;
  int rc = dtype == RSYS_DTYPE_BF16 ? launch_gemm<bf16>(p, false, false, true, true, nullptr)
                                    : launch_gemm<float>(p, false, false, true, true, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_gemm_epi(int32_t dtype, const void* A, const void* B, void* C, int32_t M, int32_t N, int32_t K, int64_t lda,
                         int64_t ldb, int64_t ldc, int32_t b_km, int32_t c_f32, int32_t epi, float alpha, int32_t accum,
                         const float* bias, const float* resid, int64_t ldr, void* C2, int64_t ldc2, const float* E,
                         const float* rope_cos, const float* rope_sin, const float* rope_cs, const int32_t* rope_pos, int32_t T,
                         int32_t hd, int32_t n_q, int32_t n_k, const int32_t* m_dev, char* tag, int32_t tag_bytes, int32_t* half) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_gemm_epi: dtype is fp32 or bf16");
  ARG_CHECK(A != nullptr && B != nullptr && C != nullptr, "rsys_op_gemm_epi: null operand");
  ARG_CHECK(tag != nullptr && tag_bytes >= 4 && half != nullptr, "rsys_op_gemm_epi: null output");
  ARG_CHECK(epi >= EPI_STORE && epi <= EPI_SWIGLU_BWD && epi != EPI_ATOMIC, "rsys_op_gemm_epi: epilogue is one of GemmEpi without EPI_ATOMIC");
  // the operands an epilogue dereferences (the launchers take them on trust)
  if (epi == EPI_BIAS || epi == EPI_TABLE || epi == EPI_GELU) ARG_CHECK(bias != nullptr, "rsys_op_gemm_epi: this epilogue reads bias");
  if (epi == EPI_RESIDUAL) ARG_CHECK(resid != nullptr, "rsys_op_gemm_epi: EPI_RESIDUAL reads resid");
  if (epi == EPI_TABLE) ARG_CHECK(E != nullptr, "rsys_op_gemm_epi: EPI_TABLE reads E");
  if (epi == EPI_SWIGLU || epi == EPI_TABLE || epi == EPI_GELU || epi == EPI_SWIGLU_BWD) ARG_CHECK(C2 != nullptr, "rsys_op_gemm_epi: this epilogue needs C2");
  if (epi == EPI_QKV_ROPE) ARG_CHECK(rope_cos != nullptr && rope_sin != nullptr, "rsys_op_gemm_epi: EPI_QKV_ROPE reads rope_cos / rope_sin");
  GemmParams p{};
  p.A = A; p.B = B; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32 != 0; p.splitk = 1; p.epi = epi; p.alpha = alpha; p.accum = accum != 0;
  p.bias = bias; p.resid = resid; p.ldr = ldr; p.C2 = C2; p.ldc2 = ldc2; p.E = E;
  p.rope_cos = rope_cos; p.rope_sin = rope_sin; p.rope_cs = rope_cs; p.rope_pos = rope_pos; p.T = T; p.hd = hd; p.n_q = n_q; p.n_k = n_k;
  p.m_dev = m_dev;
  const bool bf = dtype == RSYS_DTYPE_BF16;
  int rc = bf ? launch_gemm<bf16>(p, false, false, false, b_km != 0, nullptr) : launch_gemm<float>(p, false, false, false, b_km != 0, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  // what launch_gemm just decided, from the same parameters and switches
  const GemmRoute r = bf ? gemm_route<bf16>(p, false, false, false, b_km != 0, cu_count()) : gemm_route<float>(p, false, false, false, b_km != 0, cu_count());
  snprintf(tag, tag_bytes, "%s", gemm_kernel_tags[r.kernel]);
  *half = r.kernel == GK_8C && gemm8c_uses_half(p, cu_count()) ? 1 : 0;
  return RSYS_OK;
}

// the routing of launch_gemm, on the host only: a GemmParams from the fields the route reads (pointer fields only as set / unset)
int32_t rsys_debug_gemm_route(int32_t dtype, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t a_km,
                              int32_t b_km, int32_t a_f32, int32_t c_f32, int32_t epi, int32_t splitk, int32_t flags, float alpha,
                              int32_t accum, int32_t set, int32_t m_expect, int32_t cus, char* tag, int32_t tag_bytes, int32_t* splits) {
  ARG_CHECK(tag != nullptr && tag_bytes >= 4 && splits != nullptr, "rsys_debug_gemm_route: null output");
  static int dummy[4];   // (never dereferenced: the route only tests these for null)
  GemmParams p{};
  p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc; p.ldc2 = ldc; p.ldr = ldc;
  p.c_f32 = c_f32; p.epi = epi; p.splitk = splitk; p.flags = flags; p.alpha = alpha; p.accum = accum; p.m_expect = m_expect;
  if (set & 1) p.m_dev = dummy;
  if (set & 2) p.k_dev = dummy;
  if (set & 4) p.slab = (float*)dummy;
  if (set & 8) p.rope_cs = (const float*)dummy;
  if (set & 16) p.rope_pos = dummy;
  if (set & 32) p.C2 = dummy;
  const GemmRoute r = dtype == RSYS_DTYPE_BF16 ? gemm_route<bf16>(p, a_f32 != 0, false, a_km != 0, b_km != 0, cus)
                                                : gemm_route<float>(p, false, false, a_km != 0, b_km != 0, cus);
  snprintf(tag, tag_bytes, "%s", gemm_kernel_tags[r.kernel]);
  *splits = r.splitk;
  return RSYS_OK;
}

int32_t rsys_op_f8_quantize(const void* src, int64_t ld_src, int32_t rows, int32_t cols, int32_t fmt, int32_t layout, int32_t seg_cols,
                            int32_t seg_rep, void* dst, int64_t ld_dst, float* amax_dev, float* desc_dev, const float* wamax_dev,
                            int32_t n_w, int32_t w_rep, int32_t desc_mode) {
  switches_parse();
  ARG_CHECK(src && dst && amax_dev, "rsys_op_f8_quantize: null buffer");
  F8Cast c{};
  c.src = src; c.ld_src = ld_src; c.rows = rows; c.cols = cols; c.fmt = fmt; c.layout = layout; c.seg_cols = seg_cols; c.seg_rep = seg_rep < 1 ? 1 : seg_rep;
  c.amax = amax_dev; c.dst = (unsigned char*)dst; c.ld_dst = ld_dst; c.desc = desc_dev; c.wamax = wamax_dev; c.n_w = n_w; c.w_rep = w_rep < 1 ? 1 : w_rep;
  c.desc_mode = desc_mode;
  HIP_CHECK(hipMemsetAsync(amax_dev, 0, (size_t)F8_AMAX_SHARDS * F8_AMAX_SHARD * 4, nullptr));
  int rc = launch_f8_amax(c, nullptr);
  if (!rc) rc = launch_f8_cast(c, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_f8_weights(const float* src, int64_t ld, int32_t rows, int32_t cols, int32_t layout, int32_t seg_rows, int32_t seg_rep,
                           float* amax_dev, void* dst, void* dst_t, int64_t ld_t) {
  switches_parse();
  ARG_CHECK(src && dst && amax_dev, "rsys_op_f8_weights: null buffer");
  ARG_CHECK(cols % 4 == 0 && rows % 16 == 0, "rsys_op_f8_weights: rows % 16, cols % 4");
  F8WeightJob j{};
  j.src = src; j.ld = ld; j.rows = rows; j.cols = cols; j.layout = layout; j.seg_rows = seg_rows; j.seg_rep = seg_rep < 1 ? 1 : seg_rep; j.amax = amax_dev;
  j.dst = (unsigned char*)dst; j.dst_t = (unsigned char*)dst_t; j.ld_t = ld_t;
  const int ntiles = ((rows + 63) / 64) * ((cols + 63) / 64);
  std::vector<int> tj(ntiles, 0); int first = 0;
  void* dev = nullptr;
  HIP_CHECK(hipMalloc(&dev, sizeof(F8WeightJob) + 256 + (size_t)ntiles * 4 + 64));
  F8WeightJob* dj = (F8WeightJob*)dev; int* dfirst = (int*)((char*)dev + ((sizeof(F8WeightJob) + 63) / 64) * 64); int* dtj = dfirst + 16;
  bool ok = hipMemcpy(dj, &j, sizeof(j), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dfirst, &first, 4, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dtj, tj.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(amax_dev, 0, 16) == hipSuccess;
  int rc = ok ? launch_f8_weights(dj, dtj, dfirst, ntiles, nullptr) : RSYS_ERR_HIP;
  hipError_t e2 = hipDeviceSynchronize();
  hipFree(dev);
  if (rc) { if (!ok) set_error("rsys_op_f8_weights: job upload failed"); return rc; }
  HIP_CHECK(e2);
  return RSYS_OK;
}

int32_t rsys_op_gemm_f8(const void* A8, const void* B8, void* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc,
                        int32_t a_fmt, int32_t c_f32, const float* desc_dev, int32_t seg_cols, int32_t alt, int32_t kb0, int32_t kb1,
                        int32_t kb2) {
  switches_parse();
  GemmParams p{};
  p.A = A8; p.B = B8; p.C = C; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.c_f32 = c_f32; p.splitk = 1; p.alpha = 1.f; p.epi = EPI_STORE;
  p.f8 = a_fmt == F8_E5M2 ? 2 : 1; p.f8_desc = desc_dev; p.f8_seg_cols = seg_cols; p.f8_alt = alt; p.f8_kb[0] = kb0; p.f8_kb[1] = kb1; p.f8_kb[2] = kb2;
  int rc = launch_gemm8p_f8(p, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_attention(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv,
                          const int32_t* uid, const int32_t* tm, void* O, float* lse, const void* dO, void* dqkv,
                          const float* rope_cos, const float* rope_sin) {
  return rsys_op_attention_ex(dtype, B, T, H, KV, hd, qkv, uid, tm, O, lse, dO, dqkv, rope_cos, rope_sin, nullptr, T, nullptr, nullptr, nullptr);
}

int32_t rsys_op_attention_ex(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv,
                             const int32_t* uid, const int32_t* tm, void* O, float* lse, const void* dO, void* dqkv,
                             const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows,
                             const int32_t* q_active, float* amax_fwd, float* amax_bwd) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_attention: dtype fp32 or bf16");
  ARG_CHECK(B >= 1 && T >= 1 && H >= 1 && KV >= 1 && qkv && uid && tm && O && lse, "rsys_op_attention: null or empty");
  ARG_CHECK(!dO || (dqkv && rope_cos && rope_sin), "rsys_op_attention: the backward needs dqkv and the rope tables");
  if (dO && rope_pos) {   // every explicit position inside the tables (one copy back)
    std::vector<int32_t> pos((size_t)B * T);
    HIP_CHECK(hipMemcpy(pos.data(), rope_pos, pos.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t v : pos) ARG_CHECK(v >= 0 && v < rope_rows, "rsys_op_attention: rope_pos outside the tables");
  } else if (dO) {
    ARG_CHECK(rope_rows >= T, "rsys_op_attention: rope tables shorter than T");
  }
  const size_t e = dtype == RSYS_DTYPE_BF16 ? 2 : 4;
  const int nt = (T + 63) / 64;
  AttnParams p{};
  p.B = B; p.T = T; p.H = H; p.KV = KV; p.hd = hd; p.is_bf16 = dtype == RSYS_DTYPE_BF16;
  p.q = qkv; p.k = (const unsigned char*)qkv + (size_t)H * hd * e; p.v = (const unsigned char*)qkv + (size_t)(H + KV) * hd * e;
  p.ld = (long long)(H + 2 * KV) * hd;
  p.o = O; p.ldo = (long long)H * hd; p.lse = lse; p.uid = uid; p.tm = tm;
  unsigned int* maps = nullptr; float* delta = nullptr;
  unsigned long long* pairbits = nullptr;
  const size_t mw = (size_t)attn_map_words(T) * B * nt;   // words of one [B][nt] map
  HIP_CHECK(hipMalloc((void**)&maps, sizeof(unsigned int) * (12 * mw + (size_t)B * (H + KV) * nt)));
  HIP_CHECK(hipMalloc((void**)&pairbits, sizeof(unsigned long long) * 2 * (size_t)B * nt * nt * 64));
  HIP_CHECK(hipMalloc((void**)&delta, sizeof(float) * B * H * T));
  p.qmap = maps; p.kmap = maps + mw; p.qmap_full = maps + 2 * mw; p.kmap_full = maps + 3 * mw; p.delta = delta;
  p.qmap16 = maps + 4 * mw; p.kmap16 = maps + 8 * mw;
  p.order_q = (int*)(maps + 12 * mw); p.order_k = p.order_q + (size_t)B * H * nt;
  p.qbits = pairbits; p.kbits = pairbits + (size_t)B * nt * nt * 64;
  p.dO = dO; p.dq = dqkv; p.dk = (unsigned char*)dqkv + (size_t)H * hd * e;
  p.dv = (unsigned char*)dqkv + (size_t)(H + KV) * hd * e; p.ldg = p.ld;
  p.rope_cos = rope_cos; p.rope_sin = rope_sin; p.rope_pos = rope_pos; p.q_active = q_active;
  // (delta of the query tiles beyond q_active is never written: NaN there, so that a dK/dV kernel that reads it shows)
  if (q_active) HIP_CHECK(hipMemsetAsync(delta, 0xFF, sizeof(float) * B * H * T, nullptr));
  int rc = launch_attn_tilemap(p, nullptr);
  p.f8_amax = amax_fwd;
  if (!rc) rc = dtype == RSYS_DTYPE_BF16 ? launch_attn_fwd<bf16>(p, nullptr) : launch_attn_fwd<float>(p, nullptr);
  p.f8_amax = amax_bwd;
  if (!rc && dO) {
    rc = dtype == RSYS_DTYPE_BF16 ? launch_attn_bwd<bf16>(p, nullptr) : launch_attn_bwd<float>(p, nullptr);
  }
  hipError_t e2 = hipDeviceSynchronize();
  hipFree(maps); hipFree(delta); hipFree(pairbits);
  if (rc) return rc;
  HIP_CHECK(e2);
  return RSYS_OK;
}

// attn_sel_kernel alone: the tile maps are built here, as rsys_op_attention_ex builds them; sel is checked on the host
int32_t rsys_op_attention_selected(int32_t dtype, int32_t B, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const int32_t* uid,
                                   const int32_t* tm, int32_t n_sel, const int32_t* sel, void* O) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_attention_selected: dtype fp32 or bf16");
  ARG_CHECK(B >= 1 && T >= 1 && H >= 1 && KV >= 1 && n_sel >= 1 && qkv && uid && tm && sel && O, "rsys_op_attention_selected: null or empty");
  ARG_CHECK((long long)B * T < (1ll << 31), "rsys_op_attention_selected: B * T must stay below 2^31");
  {
    std::vector<int32_t> hs((size_t)n_sel);
    HIP_CHECK(hipMemcpy(hs.data(), sel, hs.size() * 4, hipMemcpyDeviceToHost));
    for (int32_t v : hs) ARG_CHECK(v >= 0 && v < B * T, "rsys_op_attention_selected: a selected token outside [0, B * T)");
  }
  const size_t e = dtype == RSYS_DTYPE_BF16 ? 2 : 4;
  const int nt = (T + 63) / 64;
  AttnParams p{};
  p.B = B; p.T = T; p.H = H; p.KV = KV; p.hd = hd; p.is_bf16 = dtype == RSYS_DTYPE_BF16;
  p.q = qkv; p.k = (const unsigned char*)qkv + (size_t)H * hd * e; p.v = (const unsigned char*)qkv + (size_t)(H + KV) * hd * e;
  p.ld = (long long)(H + 2 * KV) * hd; p.uid = uid; p.tm = tm;
  unsigned int* maps = nullptr; unsigned long long* pairbits = nullptr;
  const size_t mw = (size_t)attn_map_words(T) * B * nt;   // words of one [B][nt] map
  HIP_CHECK(hipMalloc((void**)&maps, sizeof(unsigned int) * 12 * mw));
  if (hipMalloc((void**)&pairbits, sizeof(unsigned long long) * 2 * (size_t)B * nt * nt * 64) != hipSuccess) { (void)hipGetLastError(); hipFree(maps); set_error("rsys_op_attention_selected: no memory for the pair bits"); return RSYS_ERR_HIP; }
  p.qmap = maps; p.kmap = maps + mw; p.qmap_full = maps + 2 * mw; p.kmap_full = maps + 3 * mw;
  p.qmap16 = maps + 4 * mw; p.kmap16 = maps + 8 * mw;
  p.qbits = pairbits; p.kbits = pairbits + (size_t)B * nt * nt * 64;
  int rc = launch_attn_tilemap(p, nullptr);
  if (!rc) rc = dtype == RSYS_DTYPE_BF16 ? launch_attn_sel<bf16>(p, sel, n_sel, O, (long long)H * hd, nullptr) : launch_attn_sel<float>(p, sel, n_sel, O, (long long)H * hd, nullptr);
  hipError_t e2 = hipDeviceSynchronize();
  hipFree(maps); hipFree(pairbits);
  if (rc) return rc;
  HIP_CHECK(e2);
  return RSYS_OK;
}

int32_t rsys_op_attention_cached(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const void* cache,
                                 int32_t n_slots, const int32_t* slot, const int32_t* n_hist, const int32_t* n_cand, void* O) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "dtype: fp32 or bf16");
  ARG_CHECK(qkv && cache && slot && n_hist && n_cand && O && KV >= 1 && H >= 1, "null or empty");
  CandAttnParams p{};
  p.rows = rows; p.T = T; p.H = H; p.KV = KV; p.hd = hd;
  p.qkv = qkv; p.ld = (long long)(H + 2 * KV) * hd; p.cache = cache; p.n_slots = n_slots;
  p.slot = slot; p.n_hist = n_hist; p.n_cand = n_cand; p.o = O; p.ldo = (long long)H * hd;
  const int rc = dtype == RSYS_DTYPE_BF16 ? launch_attn_cand<bf16>(p, nullptr) : launch_attn_cand<float>(p, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

// attn_cand_tiles_kernel alone: the host's segments (row, first_tile, n_cand, slot, n_hist) are checked (inside their rows, no tile twice, slots
// and counts in range) and become the kernel's two device tables for the length of the call
int32_t rsys_op_attention_cached_tiles(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, const void* cache,
                                       int32_t n_slots, int32_t Tc, int32_t n_seg, const int32_t* seg, void* O) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "dtype: fp32 or bf16");
  ARG_CHECK(qkv && cache && seg && O && KV >= 1 && H >= 1 && rows >= 1 && T >= 8 && n_slots >= 1, "null or empty");
  if (Tc == 0) Tc = T;
  TileOwners tiles(rows, T / 2);   // (a row of T tokens holds T / 2 interaction columns; ceil(T / 64) tiles)
  ARG_CHECK(n_seg >= 1 && n_seg <= rows * tiles.nt, "1 <= n_seg <= rows x ceil(T / 64)");
  std::vector<int> tab((size_t)4 * n_seg, -1);
  for (int i = 0; i < n_seg; ++i) {
    const int r = seg[5 * i], ft = seg[5 * i + 1], nc = seg[5 * i + 2], sl = seg[5 * i + 3], nh = seg[5 * i + 4];
    ARG_CHECK(ft >= 0 && ft < tiles.nt && nc >= 1, "segment outside its row");
    ARG_CHECK(sl >= 0 && sl < n_slots && nh >= 0 && 2 * nh <= Tc, "segment's slot or n_hist out of range");
    RC(tiles.place("rsys_op_attention_cached_tiles", r, 32 * ft, nc, i));
    tab[4 * i] = sl; tab[4 * i + 1] = nh; tab[4 * i + 2] = ft; tab[4 * i + 3] = nc;
  }
  tab.insert(tab.end(), tiles.owner.begin(), tiles.owner.end());
  int* d_tab = nullptr;
  HIP_CHECK(hipMalloc((void**)&d_tab, tab.size() * 4));
  hipError_t e = hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
  int rc = RSYS_OK;
  if (e == hipSuccess) {
    CandAttnParams p{};
    p.rows = rows; p.T = T; p.Tc = Tc; p.H = H; p.KV = KV; p.hd = hd;
    p.qkv = qkv; p.ld = (long long)(H + 2 * KV) * hd; p.cache = cache; p.n_slots = n_slots;
    p.seg = d_tab; p.tile_seg = d_tab + 4 * n_seg; p.n_seg = n_seg; p.o = O; p.ldo = (long long)H * hd;
    rc = dtype == RSYS_DTYPE_BF16 ? launch_attn_cand<bf16>(p, nullptr) : launch_attn_cand<float>(p, nullptr);
    e = hipDeviceSynchronize();
  }
  (void)hipFree(d_tab);
  if (rc) return rc;
  HIP_CHECK(e);
  return RSYS_OK;
}

// rank_cache_copy_segments_kernel alone: the host's descriptors (row, first column, n_hist, slot) are checked against the rows and the cache
int32_t rsys_op_rank_cache_copy_segments(int32_t dtype, int32_t rows, int32_t T, int32_t H, int32_t KV, int32_t hd, const void* qkv, void* cache,
                                         int32_t n_slots, int32_t Tc, int32_t n_seg, const int32_t* seg) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "dtype: fp32 or bf16");
  ARG_CHECK(qkv && cache && seg && KV >= 1 && H >= 1 && hd >= 1 && rows >= 1 && T >= 2 && n_slots >= 1 && n_seg >= 1 && n_seg <= 65535, "null or empty");
  if (Tc == 0) Tc = T;
  for (int i = 0; i < n_seg; ++i) {
    const int r = seg[4 * i], c0 = seg[4 * i + 1], nh = seg[4 * i + 2], sl = seg[4 * i + 3];
    ARG_CHECK(r >= 0 && r < rows && c0 >= 0 && nh >= 0 && 2 * ((long long)c0 + nh) <= T && 2 * (long long)nh <= Tc, "segment outside its row or longer than a slot");
    ARG_CHECK(sl >= 0 && sl < n_slots, "slot outside the cache");
  }
  int* d_seg = nullptr;
  HIP_CHECK(hipMalloc((void**)&d_seg, (size_t)4 * n_seg * 4));
  hipError_t e = hipMemcpy(d_seg, seg, (size_t)4 * n_seg * 4, hipMemcpyHostToDevice);
  int rc = RSYS_OK;
  if (e == hipSuccess) {
    const long long ld = (long long)(H + 2 * KV) * hd;
    rc = dtype == RSYS_DTYPE_BF16
             ? launch_rank_cache_copy_segments<bf16>((const bf16*)qkv, ld, H * hd, 2 * KV * hd, T, Tc, rows, d_seg, n_seg, n_slots, (bf16*)cache, nullptr)
             : launch_rank_cache_copy_segments<float>((const float*)qkv, ld, H * hd, 2 * KV * hd, T, Tc, rows, d_seg, n_seg, n_slots, (float*)cache, nullptr);
    e = hipDeviceSynchronize();
  }
  (void)hipFree(d_seg);
  if (rc) return rc;
  HIP_CHECK(e);
  return RSYS_OK;
}

// the backward's embedding scatter on caller-provided device buffers: gE[id'] += sum_n gx0[n * ldx ..+D) over the tokens whose
// masked id (m_matchedid, -1 -> row V) is id'; the token index is built from the raw ids (matchedid) as at batch upload.
// atomic != 0 runs the float-atomic form instead (A/B reference).
int32_t rsys_op_topk(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, int32_t* ids, float* vals, int32_t* counts) {
  switches_parse();
  return op_topk(scores, ld, rows, V, k, ids, vals, counts);
}
int32_t rsys_op_topk_window(const float* scores, int64_t ld, int32_t rows, int32_t V, const int64_t* start, const int32_t* len,
                            int32_t* ids, float* vals, int32_t* counts, int32_t* totals, int32_t* bounds) {
  switches_parse();
  return op_topk_window(scores, ld, rows, V, start, len, ids, vals, counts, totals, bounds);
}
int32_t rsys_op_lse(const float* z, int64_t ldz, int32_t rows, int32_t V, float* lse) {
  switches_parse();
  return op_lse(z, ldz, rows, V, lse);
}
int32_t rsys_op_query_weights(const float* z, int64_t ldz, const float* lse, const int32_t* members, const int32_t* ranges, int32_t q0,
                              const float* user_w, int32_t n_groups, const float* src, float* dst, int32_t V, int32_t last,
                              const int64_t* cand_offsets, const int32_t* cand, const float* r_masked, const int64_t* rm_offsets,
                              const float* retrieval_coef, const float* rating_coefs, float rating_mean, int32_t first, float* sc,
                              const int64_t* sel_offsets, const int32_t* sel_medium, const int32_t* sel_ids, int32_t medium, const float* emb_m,
                              const float* X, int32_t dim, const float* sel_w, float* S) {
  switches_parse();
  ARG_CHECK(dst || sc || S, "rsys_op_query_weights: no section asked for (dst, sc and S are all NULL)");
  if (dst) RC(op_combine_weighted(src, dst, n_groups, V, last, z, ldz, lse, members, ranges, q0, user_w));
  if (sc) RC(op_rank_score_weighted(n_groups, cand_offsets, cand, z, ldz, lse, members, ranges, q0, r_masked, rm_offsets, retrieval_coef,
                                    rating_coefs, rating_mean, first, user_w, sc));
  if (S) RC(op_selected_sum_weighted(n_groups, sel_offsets, sel_medium, sel_ids, medium, emb_m, X, dim, sel_w, S));
  return RSYS_OK;
}
int32_t rsys_op_target_rank(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* targets, int32_t* rank_out) {
  switches_parse();
  return op_target_rank(scores, ld, rows, V, targets, rank_out);
}
int32_t rsys_op_pair_ranks(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* self, const int64_t* tgt_offsets,
                           const int32_t* tgt_ids, int32_t* ranks_out) {
  switches_parse();
  return op_pair_ranks(scores, ld, rows, V, self, tgt_offsets, tgt_ids, ranks_out);
}
int32_t rsys_op_rerank(int32_t n, int32_t partialk, const float* pen, const float* r, const float* gram, const int32_t* ss_bits,
                       const int32_t* related_bits, int32_t* picks) {
  switches_parse();
  return op_rerank(n, partialk, pen, r, gram, ss_bits, related_bits, picks);
}
int32_t rsys_op_embedding_scatter(const float* gx0, int64_t ldx, const int32_t* matchedid, const int32_t* m_matchedid, int32_t N,
                                  int32_t V, int32_t D, float* gE, int32_t atomic) {
  switches_parse();
  ARG_CHECK(gx0 && matchedid && m_matchedid && gE && N >= 1 && ldx >= D, "rsys_op_embedding_scatter: arguments");
  if (atomic) {
    ARG_CHECK(ldx == 2LL * D, "the atomic form reads the interleaved layout (row stride 2 D)");
    BatchDev b{}; b.N = N; b.m_matchedid = const_cast<int*>(m_matchedid);
    int rc = launch_embedding_scatter_add(gx0, b, V, D, gE, nullptr);
    if (rc) return rc;
    HIP_CHECK(hipDeviceSynchronize());
    return RSYS_OK;
  }
  unsigned long long* keys = nullptr; int *skey = nullptr, *sidx = nullptr; float* slab = nullptr;
  HIP_CHECK(hipMalloc((void**)&keys, (size_t)token_index_capacity(N) * 8));
  HIP_CHECK(hipMalloc((void**)&skey, (size_t)N * 4));
  HIP_CHECK(hipMalloc((void**)&sidx, (size_t)N * 4));
  HIP_CHECK(hipMalloc((void**)&slab, seg_scatter_slab_floats(N, D) * 4));
  int rc = launch_token_index_build(matchedid, N, V, keys, skey, sidx, nullptr);
  if (!rc) rc = launch_embedding_scatter_segmented(gx0, ldx, m_matchedid, skey, sidx, N, V, D, gE, slab, nullptr);
  hipError_t e = hipDeviceSynchronize();
  hipFree(keys); hipFree(skey); hipFree(sidx); hipFree(slab);
  if (rc) return rc;
  HIP_CHECK(e);
  return RSYS_OK;
}

// ---------------------------------------------------------------- row kernels and the optimiser on caller-provided buffers (tests)
// Deterministic-mode scratch of one hook call: installed in g_det for that call only (as DetScope does for a model), freed afterwards.
// check() fails unless the launch took the partial-sum branch with no launch falling back to atomics for want of scratch.
struct HookDet {
  DetScratch saved;
  float *part = nullptr, *tmp = nullptr;
  bool on;
  explicit HookDet(bool on_) : saved(g_det), on(on_) { g_det = DetScratch(); }
  ~HookDet() { hipDeviceSynchronize(); g_det = saved; if (part) hipFree(part); if (tmp) hipFree(tmp); }
  // part_floats for the launch's partial rows; the two-stage reduction needs ceil(partial rows / 32) * row length floats
  int alloc(long long part_floats, long long tmp_floats) {
    if (!on) return RSYS_OK;
    part_floats = std::max(part_floats, 1LL); tmp_floats = std::max(tmp_floats, 1LL);
    HIP_CHECK(hipMalloc((void**)&part, (size_t)part_floats * 4));
    HIP_CHECK(hipMalloc((void**)&tmp, (size_t)tmp_floats * 4));
    g_det.part = part; g_det.cap = part_floats; g_det.tmp = tmp; g_det.tmp_cap = tmp_floats;
    return RSYS_OK;
  }
  int check(const char* who) {
    if (!on) return RSYS_OK;
    if (g_det.part_used < 1 || g_det.part_short != 0) {
      set_error(std::string(who) + ": the deterministic partial-sum branch did not run");
      return RSYS_ERR_STATE;
    }
    return RSYS_OK;
  }
};
static long long ceil32(long long n) { return (n + 31) / 32; }

int32_t rsys_op_rmsnorm_fwd(int32_t dtype, const float* x, const float* scale, void* y, float* rstd, int64_t rows, int32_t D,
                            const int32_t* rows_dev, const int32_t* in_rows, float* amax) {
  switches_parse();
  ARG_CHECK(x && scale && y && rows >= 1, "rsys_op_rmsnorm_fwd: arguments");
  int rc = dtype == RSYS_DTYPE_BF16 ? launch_rmsnorm_fwd<bf16>(x, scale, (bf16*)y, rstd, rows, D, nullptr, rows_dev, in_rows, amax)
                                    : launch_rmsnorm_fwd<float>(x, scale, (float*)y, rstd, rows, D, nullptr, rows_dev, in_rows, amax);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_rmsnorm_bwd(int32_t dtype, int32_t g_f32, const void* g, const float* x, const float* scale, const float* rstd,
                            const float* resid, const int32_t* resid_slot, const int32_t* io_rows, const int32_t* rows_dev,
                            float* dx, void* dx_t, float* dscale, int64_t rows, int32_t D, float* amax, int32_t deterministic) {
  switches_parse();
  ARG_CHECK(g && x && scale && rstd && dx && dscale && rows >= 0, "rsys_op_rmsnorm_bwd: arguments");
  ARG_CHECK(!g_f32 || (resid_slot == nullptr && io_rows == nullptr), "rsys_op_rmsnorm_bwd: the f32-gradient form takes no resid_slot / io_rows");
  HookDet det(deterministic != 0);
  const long long wgs = std::max<long long>(1, std::min<long long>(rows, 4LL * std::max(1, sw().debug_norm_bwd_grid)));   // >= the launch's grid
  RC(det.alloc(wgs * D, ceil32(wgs) * D));
  const bool bf = dtype == RSYS_DTYPE_BF16;
  int rc;
  if (g_f32) rc = bf ? launch_rmsnorm_bwd_f32<bf16>((const float*)g, x, scale, rstd, resid, dx, (bf16*)dx_t, dscale, rows, D, nullptr, rows_dev, amax)
                     : launch_rmsnorm_bwd_f32<float>((const float*)g, x, scale, rstd, resid, dx, (float*)dx_t, dscale, rows, D, nullptr, rows_dev, amax);
  else rc = bf ? launch_rmsnorm_bwd<bf16>((const bf16*)g, x, scale, rstd, resid, dx, (bf16*)dx_t, dscale, rows, D, nullptr, rows_dev, resid_slot, io_rows, amax)
               : launch_rmsnorm_bwd<float>((const float*)g, x, scale, rstd, resid, dx, (float*)dx_t, dscale, rows, D, nullptr, rows_dev, resid_slot, io_rows, amax);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return det.check("rsys_op_rmsnorm_bwd");
}

int32_t rsys_op_ce(int32_t dtype, void* logits, int64_t ldl, int32_t n, int32_t V, const int32_t* idx, const float* label,
                   const float* weight, const int32_t* position, const float* stats, const int32_t* npos, float task_w, float* loss,
                   int32_t deterministic) {
  switches_parse();
  ARG_CHECK(logits && idx && label && weight && position && stats && loss && n >= 0 && V >= 1, "rsys_op_ce: arguments");
  HookDet det(deterministic != 0 && n > 0);
  RC(det.alloc(n, ceil32(n)));
  int rc = dtype == RSYS_DTYPE_BF16 ? launch_ce_fwd_bwd<bf16>((bf16*)logits, ldl, n, V, idx, label, weight, position, stats, npos, task_w, loss, nullptr)
                                    : launch_ce_fwd_bwd<float>((float*)logits, ldl, n, V, idx, label, weight, position, stats, npos, task_w, loss, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return det.check("rsys_op_ce");
}

int32_t rsys_op_rating_tail(int32_t dtype, void* z, const void* hact, int32_t n, int32_t D, const float* w2, const float* b2,
                            const int32_t* idx, const float* label, const float* weight, const float* stats, float rating_mean,
                            float task_w, int32_t evaluate, float* loss, float* dw2, float* db2, float* db0, const int32_t* npos,
                            int32_t deterministic) {
  switches_parse();
  ARG_CHECK(z && hact && w2 && b2 && idx && label && weight && stats && loss && dw2 && db2 && db0 && n >= 0, "rsys_op_rating_tail: arguments");
  HookDet det(deterministic != 0 && n > 0);
  const long long grid = std::min<long long>((n + 3) / 4, 512);   // the launcher's grid
  RC(det.alloc(grid * (2LL * D + 4), ceil32(grid) * D));
  int rc = dtype == RSYS_DTYPE_BF16
               ? launch_rating_tail<bf16>((bf16*)z, (const bf16*)hact, n, D, w2, b2, idx, label, weight, stats, rating_mean, task_w, evaluate, loss,
                                          dw2, db2, db0, nullptr, npos)
               : launch_rating_tail<float>((float*)z, (const float*)hact, n, D, w2, b2, idx, label, weight, stats, rating_mean, task_w, evaluate, loss,
                                           dw2, db2, db0, nullptr, npos);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return det.check("rsys_op_rating_tail");
}

int32_t rsys_op_sumsq(const float* g, int64_t n, float* out) {
  ARG_CHECK(g && out, "rsys_op_sumsq: arguments");
  float* part = nullptr;
  HIP_CHECK(hipMalloc((void**)&part, (size_t)sumsq_parts() * 4));
  int rc = launch_sumsq(g, n, out, part, nullptr, true);
  hipError_t e = hipDeviceSynchronize();
  hipFree(part);
  if (rc) return rc;
  HIP_CHECK(e);
  return RSYS_OK;
}

int32_t rsys_op_clip_adamw(int32_t dtype, float* p, float* g, float* m, float* v, void* shadow, int64_t n_decay, int64_t n_total,
                           float lr, float b1, float b2, float eps, float wd, int32_t step, float max_norm, float grad_div,
                           int32_t zero_grad, int64_t sh_skip_lo, int64_t sh_skip_hi, int32_t fused, float* sumsq) {
  switches_parse();
  ARG_CHECK(p && g && m && v && sumsq && n_total >= 4 && step >= 1, "rsys_op_clip_adamw: arguments");
  float* part = nullptr;
  HIP_CHECK(hipMalloc((void**)&part, (size_t)sumsq_parts() * 4));
  const bool bf = dtype == RSYS_DTYPE_BF16;
  int rc = launch_sumsq(g, n_total, sumsq, part, nullptr, true);
  if (fused) {   // optimizer_step: the clip coefficient and the 1 / grad_div inside AdamW
    const float* ss = max_norm > 0.f ? sumsq : nullptr;
    if (!rc) rc = bf ? launch_adamw<bf16>(p, g, m, v, (bf16*)shadow, n_decay, n_total, lr, b1, b2, eps, wd, step, ss, grad_div, max_norm, zero_grad, nullptr,
                                          sh_skip_lo, sh_skip_hi)
                     : launch_adamw<float>(p, g, m, v, nullptr, n_decay, n_total, lr, b1, b2, eps, wd, step, ss, grad_div, max_norm, zero_grad, nullptr);
  } else {       // clip_grad_norm_ (model_clip: a scale pass over the gradients), then AdamW with no clip
    if (!rc) rc = launch_scale(g, n_total, sumsq, grad_div, max_norm, nullptr);
    if (!rc) rc = bf ? launch_adamw<bf16>(p, g, m, v, (bf16*)shadow, n_decay, n_total, lr, b1, b2, eps, wd, step, nullptr, 1.f, 0.f, zero_grad, nullptr,
                                          sh_skip_lo, sh_skip_hi)
                     : launch_adamw<float>(p, g, m, v, nullptr, n_decay, n_total, lr, b1, b2, eps, wd, step, nullptr, 1.f, 0.f, zero_grad, nullptr);
  }
  hipError_t e = hipDeviceSynchronize();
  hipFree(part);
  if (rc) return rc;
  HIP_CHECK(e);
  return RSYS_OK;
}

// the adapter bank's kernels on caller-provided buffers (adapter_bank.hip: the launch routines the model path calls)
int32_t rsys_op_adapter_bank(int32_t dtype, int32_t stages, int32_t train, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd,
                             int32_t L, int32_t layer, float p, uint64_t seed, int64_t stream, const int32_t* row_slot, const void* bankA,
                             const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv, void* dLa, void* dxn, float* partA, float* partB,
                             float* gA, float* gB, const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows) {
  switches_parse();
  return adapter_bank_op(dtype, stages, train, rows, Ttok, D, H, KV, hd, L, layer, p, seed, stream, row_slot, bankA, bankB, xn, La, qkv, dqkv, dLa, dxn,
                         partA, partB, gA, gB, rope_cos, rope_sin, rope_pos, rope_rows);
}

int32_t rsys_op_adapter_bank_tiles(int32_t dtype, int32_t stages, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd, int32_t L,
                                   int32_t layer, const int32_t* tile_slot, const void* bankA, const void* bankB, const void* xn, void* La, void* qkv,
                                   const float* rope_cos, const float* rope_sin, const int32_t* rope_pos, int32_t rope_rows) {
  switches_parse();
  return adapter_bank_op(dtype, stages, 0, rows, Ttok, D, H, KV, hd, L, layer, 0.f, 0, 0, tile_slot, bankA, bankB, xn, La, qkv, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, rope_cos, rope_sin, rope_pos, rope_rows, 1);
}

int32_t rsys_op_adapter_bank_segments(int32_t dtype, int32_t stages, int32_t train, int32_t rows, int32_t Ttok, int32_t D, int32_t H, int32_t KV, int32_t hd,
                                      int32_t L, int32_t layer, float p, uint64_t seed, int64_t stream, const int32_t* segs, int32_t n_seg, const void* bankA,
                                      const void* bankB, const void* xn, void* La, void* qkv, const void* dqkv, void* dLa, void* dxn, float* partA,
                                      float* partB, float* gA, float* gB, const float* rope_cos, const float* rope_sin, const int32_t* rope_pos,
                                      int32_t rope_rows) {
  switches_parse();
  return adapter_bank_op(dtype, stages, train, rows, Ttok, D, H, KV, hd, L, layer, p, seed, stream, segs, bankA, bankB, xn, La, qkv, dqkv, dLa, dxn, partA,
                         partB, gA, gB, rope_cos, rope_sin, rope_pos, rope_rows, 2, n_seg);
}

int32_t rsys_op_adapter_bank_adamw(int32_t dtype, float* A32, float* B32, float* gA, float* gB, float* mA, float* vA, float* mB, float* vB, void* A,
                                   void* B, int64_t nA, int64_t nB, const float* per_slot, float b1, float b2, float eps, float wd, float* norms) {
  switches_parse();
  return adapter_bank_adamw_op(dtype, A32, B32, gA, gB, mA, vA, mB, vB, A, B, nA, nB, per_slot, b1, b2, eps, wd, norms);
}

int32_t rsys_op_dropout(int32_t dtype, const void* src, void* dst, int64_t n, float p, uint64_t seed, int64_t stream, int32_t accumulate) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_dropout: dtype fp32 or bf16");
  ARG_CHECK(src && dst && n >= 1 && p >= 0.f && p < 1.f && stream >= 0 && stream <= 0xFFFFFFFFLL, "rsys_op_dropout: arguments");
  int rc = dtype == RSYS_DTYPE_BF16 ? launch_dropout<bf16>((const bf16*)src, (bf16*)dst, n, p, seed, (unsigned int)stream, accumulate, nullptr)
                                    : launch_dropout<float>((const float*)src, (float*)dst, n, p, seed, (unsigned int)stream, accumulate, nullptr);
  if (rc) return rc;
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

// ---------------------------------------------------------------- the sharded-table kernels on caller-provided buffers (shard.hip)
// Each stage calls the launch routine the model path calls, unchanged, on the null stream.  No collective and no GEMM: the caller stands
// in for both.  Index arrays that address caller buffers are copied back once and checked before anything is launched.
namespace {
int hook_ints(const int32_t* dev, long long n, std::vector<int>& out) {
  out.resize((size_t)std::max(n, 0LL));
  if (n > 0) HIP_CHECK(hipMemcpy(out.data(), dev, (size_t)n * 4, hipMemcpyDeviceToHost));
  return RSYS_OK;
}
// a launch of a launcher with an ordered branch: in deterministic mode it must have counted itself in g_det.part_used
struct DetTook {
  const HookDet& det; int before;
  explicit DetTook(const HookDet& d) : det(d), before(g_det.part_used) {}
  int check(const char* who) const {
    if (!det.on || (g_det.part_used > before && g_det.part_short == 0)) return RSYS_OK;
    set_error(std::string(who) + ": the ordered (deterministic) branch did not run");
    return RSYS_ERR_STATE;
  }
};
}  // namespace

int32_t rsys_op_vp_ce(int32_t dtype, int32_t stages, int32_t deterministic, const int32_t* idx, const float* label, const float* weight,
                      const int32_t* position, const float* stats, const int32_t* npos, float task_w, int32_t KB, int32_t KBmax, float* own,
                      const void* EwAll, const float* metaAll, int32_t W, int32_t D, void* EwC, float* metaC, int32_t* nlive, int32_t* pre,
                      void* logits, int64_t ldl, int32_t Vloc, int32_t col0, float* lmax, const float* gmax, float* sums, int32_t cap,
                      int32_t rank, float* loss, int32_t rows, int32_t rows_finish) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_vp_ce: dtype fp32 or bf16");
  ARG_CHECK(stages > 0 && stages < 32, "rsys_op_vp_ce: stages is a mask of 1, 2, 4, 8, 16");
  const bool bf = dtype == RSYS_DTYPE_BF16;
  const int E = bf ? 8 : 4;
  if (stages & 1) ARG_CHECK(idx && label && weight && position && stats && npos && own && KB >= 0 && KB <= KBmax && KBmax >= 1, "rsys_op_vp_ce: meta arguments");
  if (stages & 2) ARG_CHECK(EwAll && metaAll && EwC && metaC && nlive && pre && W >= 1 && W <= 47 && KBmax >= 1 && D >= E && D % E == 0, "rsys_op_vp_ce: compact arguments");
  if (stages & (4 | 16)) ARG_CHECK(cap >= 1 && metaC && nlive && sums && Vloc >= 0 && ldl >= 0 && ldl % 8 == 0 && Vloc <= ldl, "rsys_op_vp_ce: cap >= 1, Vloc <= ldl, ldl a multiple of 8");
  if (stages & 4) ARG_CHECK(lmax && rows >= 0 && rows <= cap && (Vloc == 0 || logits), "rsys_op_vp_ce: stats arguments (rows <= cap)");
  if (stages & 8) ARG_CHECK(lmax && gmax && sums && rows >= 0, "rsys_op_vp_ce: rebase arguments");
  if (stages & 16) ARG_CHECK(gmax && pre && loss && rank >= 0 && rank < 47 && rows_finish >= 0 && rows_finish <= cap && (ldl == 0 || logits), "rsys_op_vp_ce: finish arguments (rows_finish <= cap)");
  HookDet det(deterministic != 0 && (stages & 16) && rows_finish > 0);
  RC(det.alloc(rows_finish, ceil32(rows_finish)));
  if (stages & 1) RC(launch_vp_meta(idx, label, weight, position, stats, npos, task_w, KB, KBmax, own, nullptr));
  if (stages & 2) RC(bf ? launch_vp_compact<bf16>((const bf16*)EwAll, metaAll, W, KBmax, D, (bf16*)EwC, metaC, nlive, pre, nullptr)
                        : launch_vp_compact<float>((const float*)EwAll, metaAll, W, KBmax, D, (float*)EwC, metaC, nlive, pre, nullptr));
  if ((stages & 4) && rows > 0) RC(bf ? launch_vp_stats<bf16>((const bf16*)logits, ldl, Vloc, col0, metaC, nlive, lmax, sums, cap, rows, nullptr)
                                      : launch_vp_stats<float>((const float*)logits, ldl, Vloc, col0, metaC, nlive, lmax, sums, cap, rows, nullptr));
  if ((stages & 8) && rows > 0) RC(launch_vp_rebase(lmax, gmax, sums, rows, nullptr));
  if ((stages & 16) && rows_finish > 0) {
    DetTook took(det);
    RC(bf ? launch_vp_finish<bf16>((bf16*)logits, ldl, Vloc, col0, metaC, gmax, sums, cap, nlive, pre, rank, loss, rows_finish, nullptr)
          : launch_vp_finish<float>((float*)logits, ldl, Vloc, col0, metaC, gmax, sums, cap, nlive, pre, rank, loss, rows_finish, nullptr));
    RC(took.check("rsys_op_vp_ce"));
  }
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_ss(int32_t dtype, int32_t stages, int32_t deterministic, int32_t len, int32_t n_s, int32_t n_tot, int32_t col0, uint64_t seed,
                   int64_t stream, int32_t* cols, int32_t* bitmap, int32_t* tlist, int32_t* tcount, const float* metaC, const int32_t* nlive,
                   const int32_t* pre, int32_t rank, int32_t cap_rows, int32_t rows, int32_t rows_finish, const void* EwC, const void* Floc,
                   int32_t D, void* logits, int64_t ldl, float* lmax, float* lsum, float* tl, float* gmax, float* loss, float* dt,
                   float* gE_loc, float* dEwC, const int32_t* ridx, int32_t rbase, int64_t rld, int32_t rn, int32_t rtable_rows,
                   const void* gsrc, void* gdst, const float* asrc, float* adst) {
  switches_parse();
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_ss: dtype fp32 or bf16");
  ARG_CHECK(stages > 0 && stages < 2048, "rsys_op_ss: stages is a mask of 1 .. 1024");
  const bool bf = dtype == RSYS_DTYPE_BF16;
  const int E = bf ? 8 : 4;
  ARG_CHECK(len >= 0 && n_s >= 0 && n_tot >= n_s, "rsys_op_ss: len >= 0, 0 <= n_s <= n_tot");
  if (stages & 1) ARG_CHECK(cols && stream >= 0 && stream <= 0xFFFFFFFFLL, "rsys_op_ss: sample arguments");
  if (stages & 2) ARG_CHECK(metaC && nlive && bitmap && tlist && tcount && cap_rows >= 1 && len >= 1, "rsys_op_ss: targets arguments");
  if (stages & 4) ARG_CHECK(cols && bitmap && n_s >= 1, "rsys_op_ss: drop_hits arguments");
  if (stages & (8 | 512)) ARG_CHECK(ridx && rn >= 1 && rtable_rows >= 1 && D >= 4 && rld >= D, "rsys_op_ss: plain row copy arguments");
  if (stages & 8) ARG_CHECK(gsrc && gdst && D % E == 0 && rld % E == 0, "rsys_op_ss: gather_rows_plain arguments");
  if (stages & 512) ARG_CHECK(asrc && adst && D % 4 == 0 && rld % 4 == 0, "rsys_op_ss: add_rows_plain arguments");
  if (stages & (16 | 32 | 64 | 128 | 256 | 1024)) ARG_CHECK(rows >= 0, "rsys_op_ss: rows");
  if (stages & (16 | 1024)) ARG_CHECK(EwC && Floc && metaC && nlive && D >= 1 && len >= 1, "rsys_op_ss: target row arguments");
  if (stages & 16) ARG_CHECK(tl, "rsys_op_ss: target_logit arguments");
  if (stages & (32 | 256)) ARG_CHECK(metaC && nlive && (n_tot == 0 || (logits && cols)) && ldl >= n_tot && len >= n_s, "rsys_op_ss: logits arguments (ldl >= n_tot)");
  if (stages & 32) ARG_CHECK(lmax && lsum, "rsys_op_ss: stats arguments");
  if (stages & 64) ARG_CHECK(lmax && tl && gmax, "rsys_op_ss: max_with_target arguments");
  if (stages & 128) ARG_CHECK(lmax && gmax && lsum, "rsys_op_ss: rebase arguments");
  if (stages & 256) ARG_CHECK(logits && ldl >= 1 && gmax && lsum && tl && pre && loss && dt && rank >= 0 && rank < 47 && rows_finish >= 0, "rsys_op_ss: finish arguments");
  if (stages & 1024) ARG_CHECK(dt && gE_loc && dEwC, "rsys_op_ss: target_grad arguments");
  std::vector<int> h;
  if ((stages & 4) && !(stages & 1)) {   // drop_hits reads the bitmap at cols[j]
    RC(hook_ints(cols, n_s, h));
    for (int c : h) ARG_CHECK(c >= 0 && c < len, "rsys_op_ss: drop_hits takes columns in [0, len)");
  }
  if (stages & (8 | 512)) {
    RC(hook_ints(ridx, rn, h));
    for (int c : h) ARG_CHECK(c < 0 || ((long long)rbase + c >= 0 && (long long)rbase + c < rtable_rows), "rsys_op_ss: a row index outside the table");
  }
  const bool det_stage = ((stages & 256) && rows_finish > 0) || ((stages & 1024) && rows > 0);
  HookDet det(deterministic != 0 && det_stage);
  RC(det.alloc(rows_finish, ceil32(rows_finish)));
  const unsigned int st = (unsigned int)stream;
  if (stages & 1) RC(launch_ss_sample(len, n_s, seed, st, cols, nullptr));
  if (stages & 2) RC(launch_ss_targets(metaC, nlive, cap_rows, len, col0, (unsigned int*)bitmap, tlist, tcount, nullptr));
  if (stages & 4) RC(launch_ss_drop_hits(cols, n_s, (const unsigned int*)bitmap, nullptr));
  if (stages & 8) RC(bf ? launch_gather_rows_plain<bf16>((const bf16*)gsrc, rld, ridx, rbase, (bf16*)gdst, rn, D, nullptr)
                        : launch_gather_rows_plain<float>((const float*)gsrc, rld, ridx, rbase, (float*)gdst, rn, D, nullptr));
  if ((stages & 16) && rows > 0) RC(bf ? launch_ss_target_logit<bf16>((const bf16*)EwC, (const bf16*)Floc, D, len, col0, metaC, nlive, tl, rows, nullptr)
                                       : launch_ss_target_logit<float>((const float*)EwC, (const float*)Floc, D, len, col0, metaC, nlive, tl, rows, nullptr));
  if ((stages & 32) && rows > 0) RC(bf ? launch_ss_stats<bf16>((const bf16*)logits, ldl, n_s, n_tot, len, col0, cols, metaC, nlive, lmax, lsum, rows, nullptr)
                                       : launch_ss_stats<float>((const float*)logits, ldl, n_s, n_tot, len, col0, cols, metaC, nlive, lmax, lsum, rows, nullptr));
  if ((stages & 64) && rows > 0) RC(launch_ss_max_with_target(lmax, tl, gmax, rows, nullptr));
  if ((stages & 128) && rows > 0) RC(launch_ss_rebase(lmax, gmax, lsum, rows, nullptr));
  if ((stages & 256) && rows_finish > 0) {
    DetTook took(det);
    RC(bf ? launch_ss_finish<bf16>((bf16*)logits, ldl, n_s, n_tot, len, col0, cols, metaC, gmax, lsum, tl, nlive, pre, rank, loss, dt, rows_finish, nullptr)
          : launch_ss_finish<float>((float*)logits, ldl, n_s, n_tot, len, col0, cols, metaC, gmax, lsum, tl, nlive, pre, rank, loss, dt, rows_finish, nullptr));
    RC(took.check("rsys_op_ss (finish)"));
  }
  if (stages & 512) RC(launch_add_rows_plain(asrc, ridx, rbase, adst, rld, rn, D, nullptr));
  if ((stages & 1024) && rows > 0) {
    DetTook took(det);
    RC(bf ? launch_ss_target_grad<bf16>((const bf16*)EwC, (const bf16*)Floc, D, len, col0, metaC, dt, nlive, gE_loc, dEwC, rows, nullptr)
          : launch_ss_target_grad<float>((const float*)EwC, (const float*)Floc, D, len, col0, metaC, dt, nlive, gE_loc, dEwC, rows, nullptr));
    RC(took.check("rsys_op_ss (target_grad)"));
  }
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_shard_rows(int32_t stages, const int32_t* skey, const int32_t* sidx, int32_t N, int32_t V, int32_t* slot, int32_t* uniq,
                           int32_t* tok2u, int32_t* plan, const int32_t* bound, int32_t nb, int32_t* off, float* table, int64_t ld,
                           int32_t table_rows, const int32_t* ids, int32_t sub, float* packed, int32_t n, int32_t D, const int32_t* count,
                           const int32_t* m_matchedid, const int32_t* userid, const int32_t* m_tmid, int32_t Ntok, const float* Frem,
                           int32_t frem_rows, float* x0, int32_t* uid_t, int32_t* tm_t) {
  ARG_CHECK(stages > 0 && stages < 64, "rsys_op_shard_rows: stages is a mask of 1 .. 32");
  const int row_stages = stages & (4 | 8 | 16);
  ARG_CHECK((row_stages & (row_stages - 1)) == 0, "rsys_op_shard_rows: one of the three rows-by-id stages per call");
  std::vector<int> h, h2;
  if (stages & 1) {
    ARG_CHECK(skey && sidx && slot && uniq && tok2u && plan && N >= 1 && N <= (1 << 20) && V >= 0, "rsys_op_shard_rows: plan_unique arguments");
    RC(hook_ints(skey, N, h)); RC(hook_ints(sidx, N, h2));
    for (int p = 0; p < N; ++p) {
      ARG_CHECK(h[p] >= 0 && h[p] <= V && (p == 0 || h[p - 1] <= h[p]), "rsys_op_shard_rows: skey ascending in [0, V]");
      ARG_CHECK(h2[p] >= 0 && h2[p] < N, "rsys_op_shard_rows: sidx in [0, N)");
    }
  }
  if (stages & 2) {
    ARG_CHECK(uniq && plan && bound && off && nb >= 2 && nb <= 64, "rsys_op_shard_rows: plan_offsets arguments");
    if (!(stages & 1)) { RC(hook_ints(plan, 2, h)); ARG_CHECK(h[0] >= 0 && h[0] <= (1 << 20) + 1, "rsys_op_shard_rows: plan[0] = the number of unique slots"); }
  }
  if (row_stages) {
    ARG_CHECK(table && ids && packed && n >= 0 && D >= 4 && D % 4 == 0 && ld >= D && ld % 4 == 0 && table_rows >= 1, "rsys_op_shard_rows: rows-by-id arguments");
    long long live = n, lo = sub;
    if (row_stages == 16) {
      ARG_CHECK(count, "rsys_op_shard_rows: the counted form takes a device count");
      RC(hook_ints(count, 1, h));
      ARG_CHECK(h[0] >= 0, "rsys_op_shard_rows: *count >= 0");
      live = std::min<long long>(n, h[0]); lo = 0;
    }
    RC(hook_ints(ids, live, h));
    for (int id : h) ARG_CHECK(id >= lo && id - lo < table_rows, "rsys_op_shard_rows: an id outside the table");
  }
  if (stages & 32) {
    ARG_CHECK(m_matchedid && userid && m_tmid && Frem && tok2u && plan && x0 && uid_t && tm_t && Ntok >= 1 && D >= 4 && D % 4 == 0 && frem_rows >= 1,
              "rsys_op_shard_rows: gather_items_remote arguments");
    if (!(stages & 1)) {
      RC(hook_ints(tok2u, Ntok, h)); RC(hook_ints(plan, 2, h2));
      for (int u : h) ARG_CHECK(u >= 0 && u < frem_rows, "rsys_op_shard_rows: tok2u outside the fetched rows");
      ARG_CHECK(h2[1] >= 0 && h2[1] < frem_rows, "rsys_op_shard_rows: plan[1] outside the fetched rows");
    } else
      ARG_CHECK(Ntok == N && frem_rows >= N + 1, "rsys_op_shard_rows: with plan_unique, Ntok == N and frem_rows >= N + 1");
  }
  if (stages & 1) RC(launch_plan_unique(skey, sidx, N, V, slot, uniq, tok2u, plan, nullptr));
  if (stages & 2) RC(launch_plan_offsets(uniq, plan, bound, nb, off, nullptr));
  if (stages & 4) RC(launch_gather_rows_by_id(table, ld, ids, sub, packed, n, D, nullptr));
  if (stages & 8) RC(launch_add_rows_by_id(packed, ids, sub, table, ld, n, D, nullptr));
  if (stages & 16) RC(launch_add_rows_by_id_counted(packed, ids, count, table, ld, n, D, nullptr));
  if (stages & 32) {
    BatchDev b{};   // the kernel reads N, m_matchedid, userid and m_tmid
    b.N = Ntok; b.m_matchedid = const_cast<int*>(m_matchedid); b.userid = userid; b.m_tmid = const_cast<int*>(m_tmid);
    RC(launch_gather_items_remote(b, Frem, tok2u, plan, D, x0, uid_t, tm_t, nullptr));
  }
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

// ---------------------------------------------------------------- the index and compaction kernels on caller-provided buffers
// (compact.hip, the position selection, row movers and column sums of elementwise.hip, the batched transpose of optim.hip).  Each call
// runs the production launcher unchanged on the null stream and synchronises; index arrays that address a caller buffer are copied back
// once and checked before anything is launched.
namespace {
struct HookScratch {   // device scratch of one hook call, freed on every return path
  void* p = nullptr;
  ~HookScratch() { if (p) hipFree(p); }
};
}  // namespace

int32_t rsys_op_select_positions(int32_t form, int32_t ntask, const float* w, int32_t N, int32_t topk, int32_t* idx, float* stats,
                                 int32_t* npos) {
  switches_parse();
  ARG_CHECK(form == 0 || form == 1, "rsys_op_select_positions: form 0 (one workgroup per task) or 1 (chunked)");
  ARG_CHECK(w && idx && stats && npos && ntask >= 1 && ntask <= 4 && N >= 1 && N <= (1 << 24) && topk >= 1 && topk <= N,
            "rsys_op_select_positions: 1..4 tasks, 1 <= topk <= N <= 2^24");
  const float* ws[4]; int* is[4]; float* sts[4]; int* nps[4];
  for (int i = 0; i < ntask; ++i) { ws[i] = w + (long long)i * N; is[i] = idx + (long long)i * topk; sts[i] = stats + 2 * i; nps[i] = npos + i; }
  HookScratch scratch;
  if (form == 1) {
    HIP_CHECK(hipMalloc(&scratch.p, 3 * 4 * 32 * 4));   // 3 arrays of 4 tasks x 32 chunks (launch_select_positions_chunked)
    RC(launch_select_positions_chunked(ntask, ws, N, topk, is, sts, nps, scratch.p, nullptr));
  } else {
    RC(launch_select_positions_batch(ntask, ws, N, topk, is, sts, nps, nullptr));
  }
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_token_union(int32_t ntask, const int32_t* idx, int32_t cap, const int32_t* npos, int32_t null_mask, int32_t NT, int32_t* bits,
                            int32_t* pre, int32_t* nsel) {
  switches_parse();
  ARG_CHECK(idx && npos && bits && pre && nsel && ntask >= 1 && ntask <= 4 && cap >= 1 && NT >= 1 && null_mask >= 0 && null_mask < 16,
            "rsys_op_token_union: arguments");
  std::vector<int> hn, hi;
  RC(hook_ints(npos, ntask, hn));
  const int* ips[4]; const int* nps[4];
  for (int ti = 0; ti < ntask; ++ti) {
    const bool null_task = (null_mask >> ti) & 1;
    ips[ti] = null_task ? nullptr : idx + (long long)ti * cap; nps[ti] = npos + ti;
    if (null_task) continue;
    ARG_CHECK(hn[ti] >= 0 && hn[ti] <= cap, "rsys_op_token_union: 0 <= npos <= cap");
    RC(hook_ints(idx + (long long)ti * cap, hn[ti], hi));
    for (int i : hi) ARG_CHECK(i >= 0 && 2LL * i + 1 < NT, "rsys_op_token_union: a live position outside [0, NT / 2)");
  }
  RC(launch_token_union(ips, nps, ntask, NT, (unsigned int*)bits, pre, nsel, nullptr));
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_selected_first(const int32_t* bits, const int32_t* pre, int32_t B, int32_t T, const int32_t* uid, const int32_t* tm,
                               const int32_t* rope_pos, int32_t* slot, int32_t* sel, int32_t sel_cap, int32_t* perm, int32_t* uid_p,
                               int32_t* tm_p, int32_t* pos_p, int32_t* slot_p, int32_t* sel_p, int32_t* q_active) {
  switches_parse();
  ARG_CHECK(bits && pre && uid && tm && slot && sel && perm && uid_p && tm_p && pos_p && slot_p && sel_p && q_active && B >= 1 && T >= 1 &&
                T <= 4096 && sel_cap >= 0 && (long long)B * T <= (1 << 19),
            "rsys_op_selected_first: arguments (T <= 4096, B T <= 2^19)");
  const long long nw = ((long long)B * T + 31) / 32;
  std::vector<int> hb, hp;
  RC(hook_ints(bits, nw, hb)); RC(hook_ints(pre, nw, hp));
  long long run = 0;   // sel / sel_p are addressed by pre[w] + a count inside word w
  for (long long w = 0; w < nw; ++w) {
    ARG_CHECK(hp[(size_t)w] == run, "rsys_op_selected_first: pre is not the exclusive prefix count of bits");
    run += __builtin_popcount((unsigned)hb[(size_t)w]);
  }
  ARG_CHECK(run <= sel_cap, "rsys_op_selected_first: more selected tokens than sel_cap");
  RC(launch_selected_first((const unsigned int*)bits, pre, slot, sel, uid, tm, rope_pos, B, T, perm, uid_p, tm_p, pos_p, slot_p, sel_p, q_active, nullptr));
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_rows(int32_t kind, int32_t dtype, const void* src, int64_t src_rows, void* dst, int64_t dst_rows, int64_t ld, int32_t n, int32_t D,
                     const int32_t* map, int64_t map_len, const int32_t* idx, int32_t parity, const int32_t* count, int32_t Tseq) {
  switches_parse();
  ARG_CHECK(kind >= 0 && kind <= 6, "rsys_op_rows: kind 0 .. 6");
  ARG_CHECK(dtype == RSYS_DTYPE_BF16 || dtype == RSYS_DTYPE_FP32, "rsys_op_rows: dtype fp32 or bf16");
  const bool bf = dtype == RSYS_DTYPE_BF16;
  ARG_CHECK(!bf || (kind != 4 && kind != 6), "rsys_op_rows: the adding movers are fp32 only");
  const int E = bf ? 8 : 4;
  ARG_CHECK(src && dst && src_rows >= 1 && dst_rows >= 1 && dst_rows <= (1 << 24) && src_rows <= (1 << 24) && D >= E && D % E == 0,
            "rsys_op_rows: buffers, at most 2^24 rows each, D a multiple of 16 bytes");
  const bool strided = kind == 0 || kind == 1 || kind == 2 || kind == 5 || kind == 6;
  if (strided) ARG_CHECK(ld >= D && ld % E == 0, "rsys_op_rows: ld >= D, a multiple of 16 bytes");
  ARG_CHECK(parity == 0 || parity == 1, "rsys_op_rows: parity 0 or 1");
  std::vector<int> hm, hi, hc;
  long long live = n;
  if (kind != 0) ARG_CHECK(n >= 1, "rsys_op_rows: n >= 1");
  if (kind == 0) {   // gather_rows_sel: cap = dst_rows
    ARG_CHECK(map && count && map_len >= 0, "rsys_op_rows: gather_rows_sel takes sel and a device count");
    RC(hook_ints(count, 1, hc));
    ARG_CHECK(hc[0] >= 0 && hc[0] <= dst_rows && hc[0] <= map_len, "rsys_op_rows: 0 <= *count <= min(cap, map_len)");
    RC(hook_ints(map, hc[0], hm));
    for (int r : hm) ARG_CHECK(r >= 0 && r < src_rows, "rsys_op_rows: sel outside the source");
  } else if (kind == 1) {   // scatter_rows_fill: n = B batch rows of Tseq places
    ARG_CHECK(map && count && Tseq >= 1 && (long long)n * Tseq == dst_rows && map_len == dst_rows, "rsys_op_rows: scatter_rows_fill takes slot_p [n Tseq] and q_active [n]");
    RC(hook_ints(count, n, hc)); RC(hook_ints(map, map_len, hm));
    for (int b = 0; b < n; ++b) {
      ARG_CHECK(hc[b] >= 0 && hc[b] <= (1 << 20), "rsys_op_rows: q_active >= 0");
      for (long long p = 0; p < std::min<long long>(Tseq, 64LL * hc[b]); ++p) {
        const int s = hm[(size_t)((long long)b * Tseq + p)];
        ARG_CHECK(s >= -1 && s < src_rows, "rsys_op_rows: slot_p outside the compact rows");
      }
    }
  } else if (kind == 2) {   // scatter_rows_map
    ARG_CHECK(map && map_len >= n && src_rows >= n, "rsys_op_rows: scatter_rows_map takes map [n]");
    RC(hook_ints(map, n, hm));
    std::vector<char> seen((size_t)dst_rows, 0);
    for (int r : hm) {
      ARG_CHECK(r >= 0 && r < dst_rows && !seen[(size_t)r], "rsys_op_rows: map outside the destination or not distinct");
      seen[(size_t)r] = 1;
    }
  } else {   // 3 .. 6: head rows, token 2 idx[r] + parity
    ARG_CHECK(idx, "rsys_op_rows: idx");
    const bool via_slot = kind == 3 || kind == 4, adds = kind == 4 || kind == 6;
    if (via_slot) ARG_CHECK(map && map_len >= 1, "rsys_op_rows: the slot forms take slot [map_len]");
    if (kind == 4) ARG_CHECK(count, "rsys_op_rows: scatter_rows_add_slot takes a device count");
    if (adds && count) { RC(hook_ints(count, 1, hc)); ARG_CHECK(hc[0] >= 0, "rsys_op_rows: *count >= 0"); live = std::min<long long>(n, hc[0]); }
    if (adds) ARG_CHECK(src_rows >= n, "rsys_op_rows: src holds n rows");
    else ARG_CHECK(dst_rows >= n, "rsys_op_rows: dst holds n rows");
    RC(hook_ints(idx, live, hi));
    if (via_slot) RC(hook_ints(map, map_len, hm));
    const long long tokens = via_slot ? map_len : (adds ? dst_rows : src_rows), table = adds ? dst_rows : src_rows;
    std::vector<char> seen(adds ? (size_t)table : 0, 0);
    for (int i : hi) {
      const long long tok = 2LL * i + parity;
      ARG_CHECK(i >= 0 && tok < tokens, "rsys_op_rows: a position outside the token range");
      long long row = tok;
      if (via_slot) { row = hm[(size_t)tok]; ARG_CHECK(row >= -1 && row < table, "rsys_op_rows: slot outside the compact rows"); }
      if (adds && row >= 0) { ARG_CHECK(!seen[(size_t)row], "rsys_op_rows: two live rows add to one destination row"); seen[(size_t)row] = 1; }
    }
  }
  const int cap = (int)dst_rows;
  switch (kind) {
    case 0: RC(bf ? launch_gather_rows_sel<bf16>((const bf16*)src, ld, map, count, cap, (bf16*)dst, D, nullptr)
                  : launch_gather_rows_sel<float>((const float*)src, ld, map, count, cap, (float*)dst, D, nullptr)); break;
    case 1: RC(bf ? launch_scatter_rows_fill<bf16>((const bf16*)src, map, count, n, Tseq, (bf16*)dst, ld, D, nullptr)
                  : launch_scatter_rows_fill<float>((const float*)src, map, count, n, Tseq, (float*)dst, ld, D, nullptr)); break;
    case 2: RC(bf ? launch_scatter_rows_map<bf16>((const bf16*)src, map, n, (bf16*)dst, ld, D, nullptr)
                  : launch_scatter_rows_map<float>((const float*)src, map, n, (float*)dst, ld, D, nullptr)); break;
    case 3: RC(bf ? launch_gather_rows_slot<bf16>((const bf16*)src, map, idx, parity, (bf16*)dst, n, D, nullptr)
                  : launch_gather_rows_slot<float>((const float*)src, map, idx, parity, (float*)dst, n, D, nullptr)); break;
    case 4: RC(launch_scatter_rows_add_slot((const float*)src, map, idx, parity, count, (float*)dst, n, D, nullptr)); break;
    case 5: RC(bf ? launch_gather_rows<bf16>((const bf16*)src, ld, idx, parity, (bf16*)dst, n, D, nullptr)
                  : launch_gather_rows<float>((const float*)src, ld, idx, parity, (float*)dst, n, D, nullptr)); break;
    default: RC(launch_scatter_rows_add((const float*)src, idx, parity, (float*)dst, ld, n, D, nullptr, count)); break;
  }
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

int32_t rsys_op_colsum(int32_t kind, int32_t deterministic, const float* src, int64_t ld, int64_t rows, int32_t D, float* colsum, void* dst,
                       int64_t ldt) {
  switches_parse();
  ARG_CHECK(kind >= 0 && kind <= 2, "rsys_op_colsum: kind 0 colsum_add, 1 cast_colsum, 2 cast_transpose_colsum");
  ARG_CHECK(src && colsum && rows >= 1 && rows <= (1LL << 24) && D >= 1, "rsys_op_colsum: 1 <= rows <= 2^24");
  if (kind == 0) ARG_CHECK(ld >= D, "rsys_op_colsum: ld >= cols");
  else ARG_CHECK(dst && ld == D, "rsys_op_colsum: the cast forms read a dense source (ld == D) and take dst");
  long long parts;   // the launcher's own grid formula (elementwise.hip)
  if (kind == 0) { const long long rpb = std::max<long long>(64, (rows + 511) / 512); parts = (rows + rpb - 1) / rpb; }
  else if (kind == 1) { const long long rpb = std::max<long long>(32, (rows + 511) / 512); parts = (rows + rpb - 1) / rpb; }
  else { const long long chunks = (rows + 63) / 64, cpb = std::max<long long>(1, (chunks + 2047) / 2048); parts = (chunks + cpb - 1) / cpb; }
  HookDet det(deterministic != 0);
  RC(det.alloc(parts * D, ceil32(parts) * D));
  if (kind == 0) RC(launch_colsum_add(src, ld, rows, D, colsum, nullptr));
  else if (kind == 1) RC(launch_cast_colsum(src, (bf16*)dst, rows, D, colsum, nullptr));
  else RC(launch_cast_transpose_colsum(src, (bf16*)dst, rows, D, ldt, colsum, nullptr));
  HIP_CHECK(hipDeviceSynchronize());
  return det.check("rsys_op_colsum");
}

int32_t rsys_op_transpose_bf16(int32_t n_jobs, const void* const* src, void* const* dst, const int32_t* rows, const int32_t* cols,
                               const int64_t* ld_src, const int64_t* ld_dst) {
  switches_parse();
  ARG_CHECK(src && dst && rows && cols && ld_src && ld_dst && n_jobs >= 1 && n_jobs <= 64, "rsys_op_transpose_bf16: 1 .. 64 jobs");
  TransposeBatch b{};
  for (int i = 0; i < n_jobs; ++i) {
    ARG_CHECK(src[i] && dst[i] && ((uintptr_t)src[i] & 15) == 0 && ((uintptr_t)dst[i] & 15) == 0, "rsys_op_transpose_bf16: 16-byte aligned matrices");
    ARG_CHECK(rows[i] >= 1 && cols[i] >= 1 && rows[i] <= (1 << 21) && cols[i] <= (1 << 21), "rsys_op_transpose_bf16: 1 <= rows, cols <= 2^21");
    ARG_CHECK(ld_src[i] >= cols[i] && ld_dst[i] >= rows[i] && ld_src[i] % 8 == 0 && ld_dst[i] % 8 == 0,
              "rsys_op_transpose_bf16: ld_src >= cols, ld_dst >= rows, both multiples of 8 (16-byte row strides)");
    b.job[i] = TransposeJob{src[i], dst[i], rows[i], cols[i], ld_src[i], ld_dst[i]};
  }
  b.n = n_jobs;
  RC(launch_transpose_bf16(b, nullptr));
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

// step boundaries on the model's stream: rsys_step_mark records an event, rsys_step_marks_get returns the elapsed time
// between consecutive marks (ms) and clears them -- the per-step time distribution without a host sync per step
int32_t rsys_step_mark(rsys_model* h) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  hipEvent_t e;
  HIP_CHECK(hipEventCreate(&e));
  HIP_CHECK(hipEventRecord(e, m->stream));
  m->step_marks.push_back(e);
  return RSYS_OK;
}
int32_t rsys_step_marks_get(rsys_model* h, float* ms_out, int32_t cap, int32_t* n_out) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  int n = 0;
  for (size_t i = 1; i < m->step_marks.size() && n < cap; ++i, ++n) {
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, m->step_marks[i - 1], m->step_marks[i]));
    if (ms_out) ms_out[n] = ms;
  }
  for (hipEvent_t e : m->step_marks) hipEventDestroy(e);
  m->step_marks.clear();
  if (n_out) *n_out = n;
  return RSYS_OK;
}

int32_t rsys_switches_reload(void) { switches_parse(); return RSYS_OK; }

int32_t rsys_switches_describe(char* buf, int32_t cap) { return switches_describe(buf, cap); }

int32_t rsys_op_timing(rsys_model* h, int32_t enable) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  if (enable == 3) { m->timer.enabled = false; return RSYS_OK; }   // pause: stop recording, keep what was recorded, no host wait (read it later with rsys_timing_get)
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  m->timer.enabled = enable != 0;   // (2 is accepted and means 1)
  m->timer.marks.clear(); m->timer.acc_ms.clear(); m->timer.used = 0; m->timer.open.clear();
  if (!enable) m->timer.filter.clear();
  return RSYS_OK;
}

int32_t rsys_op_timing_filter(rsys_model* h, const char* substr) {
  CHECK_HANDLE(h);
  h->m->timer.filter = substr ? substr : "";
  return RSYS_OK;
}

// "name ms count flops\n" per timed span since rsys_op_timing(1); nested spans are supported
int32_t rsys_timing_get(rsys_model* h, char* buf, size_t cap) {
  CHECK_HANDLE(h);
  Model* m = h->m;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  PhaseTimer& t = m->timer;
  std::map<std::string, std::pair<double, long>> agg;
  std::vector<size_t> stack;
  for (size_t i = 0; i < t.marks.size(); ++i) {
    if (!t.marks[i].first.empty()) { stack.push_back(i); continue; }
    if (stack.empty()) continue;
    size_t b = stack.back(); stack.pop_back();
    float ms = 0.f;
    hipEventElapsedTime(&ms, t.marks[b].second, t.marks[i].second);
    auto& a = agg[t.marks[b].first];
    a.first += ms; a.second += 1;
  }
  std::ostringstream os;
  for (auto& kv : agg) {
    double fl = 0.0;
    auto it = t.acc_ms.find(std::string("#flops:") + kv.first);
    if (it != t.acc_ms.end()) fl = it->second;
    os << kv.first << " " << kv.second.first << " " << kv.second.second << " " << fl << "\n";
  }
  std::string s = os.str();
  if (buf && cap) { strncpy(buf, s.c_str(), cap - 1); buf[cap - 1] = 0; }
  t.marks.clear(); t.acc_ms.clear(); t.used = 0; t.open.clear();
  return (int32_t)RSYS_OK;
}

}  // extern "C"
