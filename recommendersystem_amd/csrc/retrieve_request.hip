// A whole retrieval request on the device (Inference/render.jl:240-331, `retrieval(state)`): the item-similarity prior, the relation masks
// and the released-item filter from serving tables loaded once onto the model, then the scoring and top-k of retrieve.hip.  A request
// carries its users' query embeddings and list items and its selected items; only k ids and k scores per group come back.
// The kernels fill the group score rows sc [n_groups][V_m] that retrieve.hip's combine pass starts from:
//   selected   x_a = C_am E_am[id] for the selected items of the other medium (a dim x dim mat-vec over 16 waves per 64 rows, fixed
//              order), then s_g = sum over the group's selected items, in list order, of x_a (E_m[id] for an item of medium m), fp32
//   prior      sc[g][i] = s_g . E_m[i], fp32 operands and accumulation, every lane's slice summed in column order, then a fixed
//              butterfly over the wave: one read of E_m per tile of RR_GT groups, no atomics
//   static     item 0, items not in the released set, the group's selected items of medium m -> NaN
//   relations  per user (in slices of users), six bit planes over [0, V_m): W_m itself and the reachability sets Adapt W_o, Dep W_m,
//              Recap W_m, Dep C_m, Dep K_m, by OR-scatter along the CSC columns of the user's list items (order-free, so independent of
//              scheduling); then one pass per user writes NaN wherever a mask rule holds.  The list's last-status rule runs on the host.
// NaN becomes key 0 in the combine pass, so the rest of the pipeline is retrieve.hip's, unchanged.
#include <cmath>

#include "model_internal.hpp"

namespace rsys {

namespace {

constexpr int RR_THREADS = 256;
constexpr int RR_MAXDIM = 2048;      // the prior's LDS tile holds RR_GT x dim fp32 values (64 KiB at the limit)
constexpr int RR_GT = 8;             // groups per prior workgroup (largest tile)
constexpr int RR_ROWS = 4;           // items a wave scores at once (reuses each LDS read of s_g four times)
constexpr int RR_PLANES = 6;
enum { PL_W = 0, PL_ADAPT, PL_DEP_W, PL_RECAP, PL_DEP_C, PL_DEP_K };
enum { F_WM = 1, F_WO = 2, F_CM = 4, F_KM = 8 };   // the sets a (deduplicated) list item is in
// render.jl:13-23
constexpr int ST_WONT_WATCH = 1, ST_DROPPED = 2, ST_DELETED = 3, ST_PLANNED = 5, ST_WATCHING = 6, ST_COMPLETED = 7;

struct Csc {
  int64_t* colptr = nullptr;   // [cols + 1], device
  int32_t* rowval = nullptr;   // [nnz], device (explicit zeros dropped at load)
  int64_t rows = 0, cols = 0, nnz = 0;
};

struct MediumTables {
  Csc rel[3];                    // dependencies, recaps, adaptations
  unsigned* dep_rows = nullptr;  // bitset over [0, V_m): row i of `dependencies` holds an entry
  float* emb = nullptr;          // [V_m][dim]
  float* cross = nullptr;        // [dim][dim] column-major: crossproject of this medium (into the other one)
  int64_t dim = 0;
  unsigned* released = nullptr;  // bitset over [0, V_m), or null: every item released
};

__device__ __forceinline__ bool bit(const unsigned* b, long long i) { return (b[i >> 5] >> (i & 31)) & 1u; }
__device__ __forceinline__ float qnan() { return __int_as_float(0x7fc00000); }

// X[a] = C_am E_am[id] for every selected item a of the other medium (blockIdx.y = a; others return): rows blockIdx.x * 64 + lane,
// wave w sums columns [dim w / 16, dim (w + 1) / 16) in column order, then the 16 partials are added in wave order (fixed order)
__global__ void __launch_bounds__(1024) cross_kernel(const int32_t* sel_med, const int32_t* sel_ids, int m, const float* emb0,
                                                     const float* emb1, const float* cross0, const float* cross1, int dim, float* X) {
  const long long a = blockIdx.y;
  const int am = sel_med[a];
  if (am == m) return;
  const float* e = (am == 0 ? emb0 : emb1) + (long long)sel_ids[a] * dim;
  const float* C = am == 0 ? cross0 : cross1;
  const int w = threadIdx.x >> 6, r = blockIdx.x * 64 + lane_id();
  const int c0 = dim * w / 16, c1 = dim * (w + 1) / 16;
  float acc = 0.f;
  if (r < dim) {
#pragma unroll 8
    for (int c = c0; c < c1; ++c) acc = fmaf(C[(long long)c * dim + r], e[c], acc);
  }
  __shared__ float part[16][64];
  part[w][lane_id()] = acc;
  __syncthreads();
  if (w == 0 && r < dim) {
    float t = part[0][lane_id()];
    for (int v = 1; v < 16; ++v) t += part[v][lane_id()];
    X[a * dim + r] = t;
  }
}

// s_g (the rows of S [ng][dim]) = sum over the group's selected items in list order of x_a: E_m[id] for an item of medium m, X[a] else
__global__ void __launch_bounds__(RR_THREADS) selected_sum_kernel(const int64_t* sel_off, const int32_t* sel_med, const int32_t* sel_ids,
                                                                  int m, const float* emb_m, const float* X, int dim, float* S) {
  const int g = blockIdx.y, r = blockIdx.x * RR_THREADS + threadIdx.x;
  if (r >= dim) return;
  float s = 0.f;
  for (long long a = sel_off[g]; a < sel_off[g + 1]; ++a)
    s += sel_med[a] == m ? emb_m[(long long)sel_ids[a] * dim + r] : X[a * dim + r];
  S[(long long)g * dim + r] = s;
}
// the weighted form (rsys_query_weights_set): s_g = sum of w[a] * x_a, w indexed by selected-item position as sel_ids is; the product
// and the sum rounded on their own, a weight of +-0.0 skips the item
__global__ void __launch_bounds__(RR_THREADS) selected_sum_w_kernel(const int64_t* sel_off, const int32_t* sel_med, const int32_t* sel_ids,
                                                                    int m, const float* emb_m, const float* X, int dim, const float* w,
                                                                    float* S) {
  const int g = blockIdx.y, r = blockIdx.x * RR_THREADS + threadIdx.x;
  if (r >= dim) return;
  float s = 0.f;
  for (long long a = sel_off[g]; a < sel_off[g + 1]; ++a)
    s = weighted_add(s, w[a], sel_med[a] == m ? emb_m[(long long)sel_ids[a] * dim + r] : X[a * dim + r]);
  S[(long long)g * dim + r] = s;
}

// sc[g][i] = s_g . E[i] for the GT groups g0 + [0, GT) of this workgroup's tile and RR_ROWS items per wave step.  blockIdx.x = group
// tile, blockIdx.y = item block: the tiles of one item block run side by side and read its rows of E from HBM once.  Lane l sums columns
// 4l + 256j (j ascending) of each product, then a butterfly over the 64 lanes adds the partials: a fixed order, no atomics.
template <int GT>
__global__ void __launch_bounds__(RR_THREADS) prior_kernel(const float* S, int ng, const float* E, int V, int dim, int rows_per_block,
                                                           float* sc, long long ldsc) {
  extern __shared__ float4 s4[];   // [GT][dim / 4]
  const int g0 = blockIdx.x * GT, d4 = dim >> 2;
  for (int t = threadIdx.x; t < GT * d4; t += RR_THREADS) {
    const int gg = t / d4, c = t - gg * d4;
    s4[t] = g0 + gg < ng ? ((const float4*)(S + (long long)(g0 + gg) * dim))[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = lane_id();
  const long long rb = (long long)blockIdx.y * rows_per_block;
  const long long rend = rb + rows_per_block < V ? rb + rows_per_block : V;
  for (long long r0 = rb + w * RR_ROWS; r0 < rend; r0 += (RR_THREADS / 64) * RR_ROWS) {
    float acc[RR_ROWS][GT];
#pragma unroll
    for (int r = 0; r < RR_ROWS; ++r)
#pragma unroll
      for (int gg = 0; gg < GT; ++gg) acc[r][gg] = 0.f;
    const float4* er[RR_ROWS];
#pragma unroll
    for (int r = 0; r < RR_ROWS; ++r) er[r] = (const float4*)(E + (r0 + r < V ? r0 + r : V - 1) * dim);
    for (int c = lane; c < d4; c += 64) {
      float4 e[RR_ROWS];
#pragma unroll
      for (int r = 0; r < RR_ROWS; ++r) e[r] = er[r][c];
#pragma unroll
      for (int gg = 0; gg < GT; ++gg) {
        const float4 s = s4[gg * d4 + c];
#pragma unroll
        for (int r = 0; r < RR_ROWS; ++r) {
          float a = acc[r][gg];
          a = fmaf(e[r].x, s.x, a); a = fmaf(e[r].y, s.y, a); a = fmaf(e[r].z, s.z, a); a = fmaf(e[r].w, s.w, a);
          acc[r][gg] = a;
        }
      }
    }
    float out = 0.f;
#pragma unroll
    for (int r = 0; r < RR_ROWS; ++r)
#pragma unroll
      for (int gg = 0; gg < GT; ++gg) {
        float v = acc[r][gg];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == r * GT + gg) out = v;
      }
    const int r = lane / GT, gg = lane - r * GT;
    if (r < RR_ROWS && r0 + r < rend && g0 + gg < ng) sc[(long long)(g0 + gg) * ldsc + r0 + r] = out;
  }
}

// item 0 and the items outside the released set (released == nullptr: all released) of every group
__global__ void __launch_bounds__(RR_THREADS) static_mask_kernel(float* sc, int V, const unsigned* released) {
  const long long i = (long long)blockIdx.x * RR_THREADS + threadIdx.x;
  if (i >= V) return;
  if (i == 0 || (released && !bit(released, i))) sc[(long long)blockIdx.y * V + i] = qnan();
}

// the group's selected items of medium m
__global__ void __launch_bounds__(RR_THREADS) selected_mask_kernel(float* sc, int V, int m, const int64_t* sel_off, const int32_t* sel_med,
                                                                   const int32_t* sel_ids) {
  const int g = blockIdx.x;
  for (long long a = sel_off[g] + threadIdx.x; a < sel_off[g + 1]; a += RR_THREADS)
    if (sel_med[a] == m) sc[(long long)g * V + sel_ids[a]] = qnan();
}

__device__ __forceinline__ void or_column(unsigned* plane, const Csc& A, int col) {
  for (int64_t j = A.colptr[col]; j < A.colptr[col + 1]; ++j) {
    const int row = A.rowval[j];
    atomicOr(&plane[row >> 5], 1u << (row & 31));
  }
}

// OR-scatter of list entries [e0, e1) (host-deduplicated: one per (medium, id) and user, with the sets it is in) into the bit planes of
// users [u0, u0 + slice): planes [user - u0][RR_PLANES][W]
__global__ void __launch_bounds__(RR_THREADS) relation_scatter_kernel(const int32_t* ent_q, const int32_t* ent_id, const int32_t* ent_f,
                                                                      long long e0, long long e1, int u0, Csc dep, Csc recap, Csc adapt,
                                                                      unsigned* planes, long long W) {
  const long long e = e0 + (long long)blockIdx.x * RR_THREADS + threadIdx.x;
  if (e >= e1) return;
  const int id = ent_id[e], f = ent_f[e];
  unsigned* P = planes + (long long)(ent_q[e] - u0) * RR_PLANES * W;
  if (f & F_WO) or_column(P + PL_ADAPT * W, adapt, id);
  if (f & F_WM) {
    atomicOr(&P[PL_W * W + (id >> 5)], 1u << (id & 31));
    or_column(P + PL_DEP_W * W, dep, id);
    or_column(P + PL_RECAP * W, recap, id);
  }
  if (f & F_CM) or_column(P + PL_DEP_C * W, dep, id);
  if (f & F_KM) or_column(P + PL_DEP_K * W, dep, id);
}

// render.jl:257-323 for user u0 + blockIdx.y: NaN into its group's row wherever one of the user's rules masks the item
__global__ void __launch_bounds__(RR_THREADS) relation_mask_kernel(float* sc, int V, const int32_t* qgroup, int u0, const unsigned* planes,
                                                                   long long W, const unsigned* dep_rows) {
  const long long i = (long long)blockIdx.x * RR_THREADS + threadIdx.x;
  if (i >= V) return;
  const unsigned* P = planes + (long long)blockIdx.y * RR_PLANES * W;
  const long long wi = i >> 5;
  const unsigned sh = (unsigned)(i & 31);
  const bool w = (P[PL_W * W + wi] >> sh) & 1u, a = (P[PL_ADAPT * W + wi] >> sh) & 1u, dw = (P[PL_DEP_W * W + wi] >> sh) & 1u,
             rc = (P[PL_RECAP * W + wi] >> sh) & 1u, dc = (P[PL_DEP_C * W + wi] >> sh) & 1u, dk = (P[PL_DEP_K * W + wi] >> sh) & 1u;
  const bool masked = w || (a && !dw) || rc || (bit(dep_rows, i) && !dc) || dk;
  if (masked) sc[(long long)qgroup[u0 + blockIdx.y] * V + i] = qnan();
}

#define RR_LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

}  // namespace

struct RetrievalTables {
  MediumTables t[2];
  DevScratch ws;        // the request's device workspace
  std::vector<uint32_t> mark;    // host: last-status rule over [0, V0 + V1) (stamps; status)
  std::vector<int32_t> status;
  uint32_t tick = 0;
};

static RetrievalTables* tables(Model* m) {
  if (!m->rtab) m->rtab = new RetrievalTables();
  return m->rtab;
}

void retrieve_tables_free(Model* m) {
  RetrievalTables* R = m->rtab;
  if (!R) return;
  for (MediumTables& t : R->t) {
    for (Csc& c : t.rel) { dfree(c.colptr); dfree(c.rowval); }
    dfree(t.dep_rows); dfree(t.emb); dfree(t.cross); dfree(t.released);
  }
  R->ws.release();
  delete R;
  m->rtab = nullptr;
}

static std::vector<unsigned> bitset_of(int64_t n) { return std::vector<unsigned>((size_t)((n + 31) / 32), 0u); }

int model_retrieve_relations_set(Model* m, int medium, int kind, int64_t n_rows, int64_t n_cols, const int64_t* colptr, const int32_t* rowval,
                                 const float* nzval) {
  ARG_CHECK(medium == 0 || medium == 1, "retrieve_relations_set: medium must be 0 or 1");
  ARG_CHECK(kind >= 0 && kind <= 2, "retrieve_relations_set: kind must be 0 (dependencies), 1 (recaps) or 2 (adaptations)");
  const int64_t Vm = medium == 0 ? m->V0 : m->V1, Vo = medium == 0 ? m->V1 : m->V0;
  std::vector<int64_t> cp;
  std::vector<int32_t> rv;
  if (colptr) {
    ARG_CHECK(rowval && nzval, "retrieve_relations_set: rowval and nzval are required with colptr");
    ARG_CHECK(n_rows == Vm, "retrieve_relations_set: n_rows must be V_m");
    ARG_CHECK(n_cols == (kind == 2 ? Vo : Vm), "retrieve_relations_set: n_cols must be V_m (dependencies, recaps) or V_{1-m} (adaptations)");
    RC(csc_nonzero_pattern("retrieve_relations_set", "[0, n_rows)", n_rows, n_cols, colptr, rowval, nzval, cp, rv));
  }
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));   // (a request in flight may read the old table)
  MediumTables& t = tables(m)->t[medium];
  Csc& c = t.rel[kind];
  dfree(c.colptr); dfree(c.rowval);
  c.rows = c.cols = c.nnz = 0;
  if (kind == 0) dfree(t.dep_rows);
  if (!colptr) return RSYS_OK;
  RC(upload((void**)&c.colptr, cp.data(), cp.size() * 8));
  RC(upload((void**)&c.rowval, rv.data(), rv.size() * 4));
  c.rows = n_rows; c.cols = n_cols; c.nnz = (int64_t)rv.size();
  if (kind == 0) {
    std::vector<unsigned> b = bitset_of(Vm);
    for (int32_t r : rv) b[r >> 5] |= 1u << (r & 31);
    RC(upload((void**)&t.dep_rows, b.data(), b.size() * 4));
  }
  return RSYS_OK;
}

const float* retrieve_similarity_table(Model* m, int medium, int64_t* dim) {
  const MediumTables& t = tables(m)->t[medium];
  *dim = t.dim;
  return t.emb;
}

int model_retrieve_similarity_set(Model* m, int medium, int64_t dim, const float* emb, const float* crossproject) {
  ARG_CHECK(medium == 0 || medium == 1, "retrieve_similarity_set: medium must be 0 or 1");
  if (emb) ARG_CHECK(dim >= 4 && dim <= RR_MAXDIM && dim % 4 == 0, "retrieve_similarity_set: dim must be a multiple of 4 in [4, 2048]");
  const int64_t Vm = medium == 0 ? m->V0 : m->V1;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  MediumTables& t = tables(m)->t[medium];
  dfree(t.emb); dfree(t.cross);
  t.dim = 0;
  if (!emb) return RSYS_OK;
  RC(upload((void**)&t.emb, emb, (size_t)Vm * dim * 4));
  if (crossproject) RC(upload((void**)&t.cross, crossproject, (size_t)dim * dim * 4));
  t.dim = dim;
  return RSYS_OK;
}

int model_retrieve_released_set(Model* m, int medium, const uint8_t* mask) {
  ARG_CHECK(medium == 0 || medium == 1, "retrieve_released_set: medium must be 0 or 1");
  const int64_t Vm = medium == 0 ? m->V0 : m->V1;
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  MediumTables& t = tables(m)->t[medium];
  dfree(t.released);
  if (!mask) return RSYS_OK;
  std::vector<unsigned> b = bitset_of(Vm);
  for (int64_t i = 0; i < Vm; ++i)
    if (mask[i]) b[i >> 5] |= 1u << (i & 31);
  return upload((void**)&t.released, b.data(), b.size() * 4);
}

// rsys_retrieve_request, rsys_retrieve_window and the retrieval stages of rsys_render_request / rsys_render_items (model.hpp):
// dev == nullptr takes the queries from, and returns the result to, the host; else both stay on the device (RetrieveDev) and only the
// counts come back.  win != nullptr: a window of each group's ordering instead of its top k (RetrieveWin); groups may then have no
// queries -- such a group is scored by its prior alone and has no relation masks -- and nq may be 0, which needs no relation table.
int model_retrieve_request(Model* m, int medium, const Request& rq, int32_t k, const RetrieveWin* win, RetrieveDev* dev, int32_t* ids_out,
                           float* scores_out, int32_t* counts_out) {
  const int64_t nq = rq.nq;
  const int32_t ng = rq.ng;
  const int32_t* group = rq.group;
  const HistoryList& hist = rq.hist;
  const SelectedList& sel = rq.sel;
  const QueryWeights& qw = rq.qw;
  const QueryTexts& qt = rq.qt;
  const char* who = win ? "retrieve_window" : "retrieve_request";
  auto msg = [who](const char* text) { return std::string(who) + ": " + text; };
  // the limits of rsys_retrieve_topk (model_retrieve_topk)
  ARG_CHECK(medium == 0 || medium == 1, msg("medium must be 0 or 1"));
  ARG_CHECK(!m->sharded, msg("the row-sharded item table is not supported (replicated table only)"));
  ARG_CHECK((nq == 0 || (dev ? dev->d_queries != nullptr : rq.queries != nullptr)) && counts_out && (dev || (ids_out && scores_out)), msg("null buffer"));
  const int Vm = medium == 0 ? m->V0 : m->V1;
  const int V[2] = {m->V0, m->V1};
  if (win) {
    ARG_CHECK(win->start && win->len && win->total_out, msg("null buffer"));
    ARG_CHECK(nq >= 0 && nq <= 4096, msg("0 <= n_queries <= 4096"));
    ARG_CHECK(ng >= 1 && ng <= 4096, msg("1 <= n_groups <= 4096"));
    ARG_CHECK(group != nullptr || ng == nq || nq == 0, msg("without `group`, n_groups must equal n_queries"));
    for (int g = 0; g < ng; ++g) {
      ARG_CHECK(win->len[g] >= 1 && win->len[g] <= 1024, msg("1 <= win_len <= 1024"));
      ARG_CHECK(win->start[g] >= 0, msg("win_start >= 0"));
    }
  } else {
    ARG_CHECK(nq >= 1 && nq <= 4096, msg("1 <= n_queries <= 4096"));
    ARG_CHECK(ng >= 1 && ng <= nq, msg("1 <= n_groups <= n_queries (every group needs a query)"));
    ARG_CHECK(group != nullptr || ng == nq, msg("without `group`, n_groups must equal n_queries"));
    ARG_CHECK(k >= 1 && k <= std::min(Vm, 8192), msg("1 <= k <= min(V_m, 8192)"));
  }
  ARG_CHECK(Vm <= 65535 * 64, msg("V_m <= 4194240 (item blocks of the prior)"));
  std::vector<int32_t> qgroup((size_t)nq);
  for (int64_t q = 0; q < nq; ++q) {
    qgroup[q] = group ? group[q] : (int32_t)q;
    ARG_CHECK(qgroup[q] >= 0 && qgroup[q] < ng, msg("group ids must be in [0, n_groups)"));
  }
  // text queries (rsys_query_texts_set): their rows per group in text order
  std::vector<int32_t> tmem, trng;
  if (qt.n) text_plan(qt, ng, tmem, trng);
  RetrievalTables* R = tables(m);
  const MediumTables& T = R->t[medium];
  for (int kind = 0; kind < 3 && nq > 0; ++kind)
    ARG_CHECK(T.rel[kind].colptr != nullptr, msg("the dependencies, recaps and adaptations of the medium must be loaded"));
  RC(check_ragged(who, hist, nq));
  RC(check_ragged(who, sel, ng));
  // selected items: ranges, ids, the similarity tables they need
  int64_t nsel = 0;
  if (sel.off) {
    nsel = sel.off[ng];
    ARG_CHECK(nsel <= 65535, msg("at most 65535 selected items per call"));
    RC(check_list_items(who, sel, ng, V));
    for (int64_t a = 0; a < nsel; ++a) {
      const int am = sel.medium[a];
      ARG_CHECK(R->t[am].emb != nullptr, msg("the item-similarity embeddings of a selected item's medium are not loaded"));
      if (am != medium)
        ARG_CHECK(R->t[am].cross != nullptr, msg("the crossproject of a selected item's medium is not loaded"));
    }
    if (nsel) {
      ARG_CHECK(T.emb != nullptr, msg("the item-similarity embeddings of the request medium are not loaded"));
      for (int64_t a = 0; a < nsel; ++a)
        ARG_CHECK(R->t[sel.medium[a]].dim == T.dim, msg("the item-similarity tables of the two media differ in width"));
    }
  }
  // list items: the last status of each (medium, id) per user (render.jl's `statuses` dict), turned into the sets it is in
  std::vector<int32_t> ent_q, ent_id, ent_f;
  std::vector<int64_t> ent_off((size_t)nq + 1, 0);
  if (hist.off) {
    RC(check_list_items(who, hist, nq, V));
    const size_t nkeys = (size_t)m->V0 + m->V1;
    if (R->mark.size() != nkeys || R->tick > 0xfffffff0u) { R->mark.assign(nkeys, 0u); R->status.assign(nkeys, 0); R->tick = 0; }
    for (int64_t q = 0; q < nq; ++q) {
      const uint32_t seen = R->tick + 1, emitted = R->tick + 2;
      R->tick += 2;
      for (int64_t j = hist.off[q]; j < hist.off[q + 1]; ++j) {
        const size_t key = (size_t)(hist.medium[j] ? m->V0 : 0) + hist.ids[j];
        R->mark[key] = seen;
        R->status[key] = hist.status[j];
      }
      for (int64_t j = hist.off[q]; j < hist.off[q + 1]; ++j) {
        const size_t key = (size_t)(hist.medium[j] ? m->V0 : 0) + hist.ids[j];
        if (R->mark[key] != seen) continue;
        R->mark[key] = emitted;
        const int s = R->status[key];
        const bool watched = s != ST_DELETED && s != ST_PLANNED;
        int f = 0;
        if (hist.medium[j] == medium) {
          if (watched) f |= F_WM;
          if (s >= ST_COMPLETED) f |= F_CM;
          if (s == ST_WATCHING || s == ST_DROPPED || s == ST_WONT_WATCH) f |= F_KM;
        } else if (watched) {
          f |= F_WO;
        }
        if (!f) continue;
        ent_q.push_back((int32_t)q); ent_id.push_back(hist.ids[j]); ent_f.push_back(f);
      }
      ent_off[(size_t)q + 1] = (int64_t)ent_q.size();
    }
  }
  const int64_t nent = (int64_t)ent_q.size();
  // users per slice of the bit planes: their RR_PLANES x V_m bits stay within the [n_groups][V_m] fp32 score slab
  const long long W = (Vm + 31) / 32;
  const int slice = (int)std::min<int64_t>(nq, std::max(1, 32 * ng / RR_PLANES));
  const int dim = (int)T.dim;

  HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  float *S, *X, *d_sw; int64_t* d_soff; int32_t *d_smed, *d_sids, *d_eq, *d_eid, *d_ef, *d_qg, *d_tmem, *d_trng; unsigned* planes;
  RC(carve_into(R->ws, s, [&](Carve& c) {
    S = c.take<float>(nsel ? (size_t)ng * dim : 0);
    X = c.take<float>(nsel ? (size_t)nsel * dim : 0);
    d_soff = c.take<int64_t>((size_t)ng + 1);
    d_smed = c.take<int32_t>(nsel);
    d_sids = c.take<int32_t>(nsel);
    d_sw = c.take<float>(qw.sel ? nsel : 0);
    d_eq = c.take<int32_t>(nent);
    d_eid = c.take<int32_t>(nent);
    d_ef = c.take<int32_t>(nent);
    d_qg = c.take<int32_t>((size_t)nq);
    d_tmem = c.take<int32_t>(tmem.size());
    d_trng = c.take<int32_t>(trng.size());
    planes = c.take<unsigned>((size_t)slice * RR_PLANES * W);
  }));
  std::vector<int64_t> soff(sel.off ? sel.off : nullptr, sel.off ? sel.off + ng + 1 : nullptr);
  if (!sel.off) soff.assign((size_t)ng + 1, 0);
  // (synchronous copies from pageable memory: the host vectors above outlive them)
  HIP_CHECK(hipMemcpyAsync(d_soff, soff.data(), soff.size() * 8, hipMemcpyHostToDevice, s));
  if (nsel) {
    HIP_CHECK(hipMemcpyAsync(d_smed, sel.medium, (size_t)nsel * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_sids, sel.ids, (size_t)nsel * 4, hipMemcpyHostToDevice, s));
    if (qw.sel) HIP_CHECK(hipMemcpyAsync(d_sw, qw.sel, (size_t)nsel * 4, hipMemcpyHostToDevice, s));
  }
  if (nent) {
    HIP_CHECK(hipMemcpyAsync(d_eq, ent_q.data(), (size_t)nent * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_eid, ent_id.data(), (size_t)nent * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_ef, ent_f.data(), (size_t)nent * 4, hipMemcpyHostToDevice, s));
  }
  if (nq) HIP_CHECK(hipMemcpyAsync(d_qg, qgroup.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
  if (qt.n) {
    HIP_CHECK(hipMemcpyAsync(d_tmem, tmem.data(), tmem.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_trng, trng.data(), trng.size() * 4, hipMemcpyHostToDevice, s));
  }

  const MediumTables& T0 = R->t[0];
  const MediumTables& T1 = R->t[1];
  auto init = [&](float* sc, hipStream_t st) -> int {
    const unsigned nbv = (unsigned)((Vm + RR_THREADS - 1) / RR_THREADS);
    tic(m, "retrieve_request_prior");
    if (nsel) {
      cross_kernel<<<dim3((unsigned)((dim + 63) / 64), (unsigned)nsel), 1024, 0, st>>>(d_smed, d_sids, medium, T0.emb, T1.emb, T0.cross,
                                                                                      T1.cross, dim, X);
      RR_LAUNCH_CHECK();
      const dim3 sgrid((unsigned)((dim + RR_THREADS - 1) / RR_THREADS), ng);
      if (qw.sel) selected_sum_w_kernel<<<sgrid, RR_THREADS, 0, st>>>(d_soff, d_smed, d_sids, medium, T.emb, X, dim, d_sw, S);
      else selected_sum_kernel<<<sgrid, RR_THREADS, 0, st>>>(d_soff, d_smed, d_sids, medium, T.emb, X, dim, S);
      RR_LAUNCH_CHECK();
      const int gt = ng == 1 ? 1 : (ng <= 4 ? 4 : RR_GT);
      const int rows_per_block = 64;
      const dim3 grid((unsigned)((ng + gt - 1) / gt), (unsigned)((Vm + rows_per_block - 1) / rows_per_block));
      const size_t lds = (size_t)gt * dim * 4;
      if (gt == 1) prior_kernel<1><<<grid, RR_THREADS, lds, st>>>(S, ng, T.emb, Vm, dim, rows_per_block, sc, Vm);
      else if (gt == 4) prior_kernel<4><<<grid, RR_THREADS, lds, st>>>(S, ng, T.emb, Vm, dim, rows_per_block, sc, Vm);
      else prior_kernel<RR_GT><<<grid, RR_THREADS, lds, st>>>(S, ng, T.emb, Vm, dim, rows_per_block, sc, Vm);
      RR_LAUNCH_CHECK();
    } else {
      HIP_CHECK(hipMemsetAsync(sc, 0, (size_t)ng * Vm * 4, st));
    }
    toc(m);
    if (qt.n) {   // the text terms join the prior, before the masks
      tic(m, "retrieve_request_texts");
      RC(retrieve_text_terms(sc, ng, Vm, qt, d_tmem, d_trng, st));
      toc(m);
    }
    tic(m, "retrieve_request_masks");
    static_mask_kernel<<<dim3(nbv, ng), RR_THREADS, 0, st>>>(sc, Vm, T.released);
    RR_LAUNCH_CHECK();
    if (nsel) {
      selected_mask_kernel<<<ng, RR_THREADS, 0, st>>>(sc, Vm, medium, d_soff, d_smed, d_sids);
      RR_LAUNCH_CHECK();
    }
    for (int u0 = 0; u0 < nq; u0 += slice) {
      const int nu = (int)std::min<int64_t>(slice, nq - u0);
      const long long e0 = ent_off[u0], e1 = ent_off[u0 + nu];
      if (e1 == e0 && T.rel[0].nnz == 0) continue;   // (no list items and no dependencies: no rule can hold)
      HIP_CHECK(hipMemsetAsync(planes, 0, (size_t)nu * RR_PLANES * W * 4, st));
      if (e1 > e0) {
        relation_scatter_kernel<<<(unsigned)((e1 - e0 + RR_THREADS - 1) / RR_THREADS), RR_THREADS, 0, st>>>(
            d_eq, d_eid, d_ef, e0, e1, u0, T.rel[0], T.rel[1], T.rel[2], planes, W);
        RR_LAUNCH_CHECK();
      }
      relation_mask_kernel<<<dim3(nbv, nu), RR_THREADS, 0, st>>>(sc, Vm, d_qg, u0, planes, W, T.dep_rows);
      RR_LAUNCH_CHECK();
    }
    toc(m);
    return RSYS_OK;
  };
  return model_retrieve_run(m, medium, rq.queries, nq, group, ng, init, k, ids_out, scores_out, counts_out, dev, win, qw.user);
}

// rsys_op_query_weights, the selected-sum section: one launch of selected_sum_w_kernel over device arrays
int op_selected_sum_weighted(int32_t ng, const int64_t* sel_off, const int32_t* sel_med, const int32_t* sel_ids, int32_t medium,
                             const float* emb_m, const float* X, int32_t dim, const float* sel_w, float* S) {
  ARG_CHECK(sel_off && sel_med && sel_ids && emb_m && X && sel_w && S, "rsys_op_query_weights: null buffer (selected sum)");
  ARG_CHECK(ng >= 1 && ng <= 65535 && dim >= 1 && (medium == 0 || medium == 1), "rsys_op_query_weights: 1 <= n_groups <= 65535, dim >= 1, medium 0 or 1");
  selected_sum_w_kernel<<<dim3((unsigned)((dim + RR_THREADS - 1) / RR_THREADS), (unsigned)ng), RR_THREADS>>>(sel_off, sel_med, sel_ids, medium,
                                                                                                            emb_m, X, dim, sel_w, S);
  RR_LAUNCH_CHECK();
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

}  // namespace rsys
