// extern "C" surface of librsys_hip.so that takes a handle (include/rsys.h, and the handle-taking hooks of include/rsys_debug.h); the
// handle-free test hooks are in capi_ops.hip.
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
  const BatchDev& b = m->resident.bd;
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
