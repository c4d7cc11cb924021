// Shared by the translation units of the training step (model.hip: set-up, orchestration, inference; model_batch.hip; model_forward.hip;
// model_backward.hip; model_optim.hip -- one file until round 5) and of the request paths behind them: the timing brackets, the GEMM
// builders and the wrapper that picks split counts, a layer's AttnParams, the fp8 product table, the tile owners of packed rows, and
// the declarations of what one unit calls in another (the step's passes; the score buffers, group plans and list checks of the
// requests).  What is defined here is `static` or inline: each unit gets its own copy, none of it owns state.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>

#include "model.hpp"

namespace rsys {

#define RC(expr)                  \
  do {                            \
    int _rc = (expr);             \
    if (_rc != RSYS_OK) return _rc; \
  } while (0)

static inline int64_t pad8(int64_t n) { return (n + 7) / 8 * 8; }

static int dalloc(Model* m, void** p, size_t bytes) {
  bytes = (bytes + 255) / 256 * 256;
  HIP_CHECK(hipMalloc(p, bytes));
  m->allocs.push_back(*p);
  HIP_CHECK(hipMemset(*p, 0, bytes));
  return RSYS_OK;
}
#define DALLOC(ptr, bytes) RC(dalloc(m, (void**)&(ptr), (size_t)(bytes)))

// ------------------------------------------------------------------ timing
static void tic(Model* m, const char* name, double flops = 0.0) {
  PhaseTimer& t = m->timer;
  if (!t.enabled) return;
  if (!t.filter.empty() && strstr(name, t.filter.c_str()) == nullptr) { t.open.push_back(0); return; }
  t.open.push_back(1);
  if (t.used + 2 > t.pool.size()) {
    if (t.pool.size() >= 8192) { t.enabled = false; return; }   // (a report is taken every few steps; past this the caller forgot to collect)
    for (int i = 0; i < 64; ++i) {
      hipEvent_t e;
      if (hipEventCreate(&e) != hipSuccess) {   // (the runtime hands out a bounded number of timing events: ~10 K; stop measuring, keep running)
        (void)hipGetLastError();
        t.enabled = false;
        return;
      }
      t.pool.push_back(e);
    }
  }
  hipEvent_t e = t.pool[t.used++];
  if (hipEventRecord(e, m->stream) != hipSuccess) {             // (seen at the production shape with every step instrumented: the record fails once
    (void)hipGetLastError();                                    //  thousands of events are pending; an unchecked failure surfaced at the next launch check)
    t.enabled = false;
    return;
  }
  t.marks.push_back({std::string(name), e});
  t.acc_ms[std::string("#flops:") + name] += flops;
}
static void toc(Model* m) {
  PhaseTimer& t = m->timer;
  if (!t.enabled) return;
  if (!t.open.empty()) { const char rec = t.open.back(); t.open.pop_back(); if (!rec) return; }
  hipEvent_t e = t.pool[t.used++];
  if (hipEventRecord(e, m->stream) != hipSuccess) {   // (the span that was open stays unpaired and is dropped by rsys_timing_get)
    (void)hipGetLastError();
    t.enabled = false;
    return;
  }
  t.marks.push_back({std::string(""), e});
}

// ------------------------------------------------------------------ GEMM helper
// K splits of a weight-gradient GEMM on the 128x128 kernel: the smallest multiple of 8 (one split never straddles XCDs)
// that gives every CU two workgroups.  Measured on the trunk's shapes (tools/scan_splitk.py, K = 65536): two co-resident
// workgroups per CU hide each other's latencies, and beyond that every further split only adds its fixed cost (first
// tiles from HBM + 64 KB of atomics) -- dW13 (88 tiles) 8 splits 690 TFLOP/s vs 632 at 32, dW2 (44) 16: 620 vs 569 at 32,
// dWqkv (32) 16: 627 vs 561 at 32, dWo (16) 32: 464.
static int pick_splitk(int M, int N, int K, int bk) {
  const long long tiles = (long long)((M + 127) / 128) * ((N + 127) / 128);
  const int kt = (K + bk - 1) / bk;
  if (kt < 16) return 1;
  long long s = (512 + tiles - 1) / tiles;
  s = (s + 7) / 8 * 8;
  if (s > 128) s = 128;
  while (s > 8 && s * 4 > kt) s -= 8;   // keep at least 4 K tiles per split
  return (int)s;
}

// deterministic mode: the reduction kernels launched inside the scope write partial sums to the model's scratch (kernels.hpp)
struct DetScope {
  DetScratch saved;
  explicit DetScope(Model* m) : saved(g_det) { if (m->deterministic) { g_det.part = m->det_part; g_det.cap = m->det_part_floats; g_det.tmp = m->det_tmp; g_det.tmp_cap = m->det_tmp_floats; } else g_det = DetScratch(); }
  ~DetScope() { g_det = saved; }
};
static int det_slab_for(Model* m, long long need, GemmParams& p) {
  if (need <= 0) return RSYS_OK;
  if (need > m->det_slab_floats) {
    ++m->host_stream_syncs;
    HIP_CHECK(hipStreamSynchronize(m->stream));
    if (m->det_slab) HIP_CHECK(hipFree(m->det_slab));
    m->det_slab = nullptr; m->det_slab_floats = 0;
    HIP_CHECK(hipMalloc((void**)&m->det_slab, (size_t)need * 4));
    m->det_slab_floats = need;
  }
  p.slab = m->det_slab; p.slab_floats = m->det_slab_floats;
  return RSYS_OK;
}

// The three operand forms of the step's products, C [M][N] = sum_k A(m, k) B(n, k): the builder's name says how A and B lie in memory,
// the caller sets the epilogue's own fields on the value it gets back.
struct StepGemm : GemmParams { bool a_km = false, b_km = false; };   // (K-major: the reduction index is the slow one)
static inline StepGemm gemm_operands(const void* A, long long lda, const void* B, long long ldb, void* C, long long ldc, int M, int N, int K) {
  StepGemm p{};
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
  return p;
}
// y = x . W^T: x [M][K] and W [N][K], both row-major
static inline StepGemm gemm_xwt(const void* A, long long lda, const void* B, long long ldb, void* C, long long ldc, int M, int N, int K) {
  return gemm_operands(A, lda, B, ldb, C, ldc, M, N, K);
}
// dx = dy . W: dy [M][K] row-major, W [K][N] as it is stored (read K-major)
static inline StepGemm gemm_dyw(const void* A, long long lda, const void* B, long long ldb, void* C, long long ldc, int M, int N, int K) {
  StepGemm p = gemm_operands(A, lda, B, ldb, C, ldc, M, N, K);
  p.b_km = true;
  return p;
}
// dW += dY^T . X: dY [K][M] and X [K][N], both K-major; fp32 C, the K splits add with float atomics
static inline StepGemm gemm_dytx(const void* A, long long lda, const void* B, long long ldb, float* C, long long ldc, int M, int N, int K) {
  StepGemm p = gemm_operands(A, lda, B, ldb, C, ldc, M, N, K);
  p.a_km = p.b_km = true; p.c_f32 = 1; p.epi = EPI_ATOMIC;
  return p;
}
// the q | k | v projection's epilogue: q and k columns rotated at the rows' positions (pos == nullptr: row % T)
static inline void gemm_qkv_rope(GemmParams& p, const Model* m, const int* pos) {
  p.epi = EPI_QKV_ROPE;
  p.rope_cos = m->rope_cos; p.rope_sin = m->rope_sin; p.rope_cs = m->rope_cs; p.rope_pos = pos; p.T = m->T; p.hd = m->hd;
  p.n_q = m->H * m->hd; p.n_k = m->KV * m->hd;
}

template <typename T>
static int gemm(Model* m, const char* tag, StepGemm p) {
  if (p.alpha == 0.f) p.alpha = 1.f;
  if (p.epi == EPI_ATOMIC && p.splitk == 0)
    p.splitk = pick_splitk(p.M, p.N, (p.k_dev != nullptr && p.k_expect > 0) ? std::min(p.K, p.k_expect) : p.K, is_bf16<T>::value ? 64 : 32);
  if (p.splitk == 0) p.splitk = 1;
  p.flags |= m->gemm_flags;
  if (m->deterministic && p.epi == EPI_ATOMIC) RC(det_slab_for(m, gemm_slab_need<T>(p, false, false, p.a_km, p.b_km), p));
  if (m->timer.enabled) tic(m, (std::string(tag) + "@" + gemm_kernel_name(p, is_bf16<T>::value, false, false, p.a_km, p.b_km)).c_str(), 2.0 * p.M * p.N * (double)p.K);
  int rc = launch_gemm<T>(p, false, false, p.a_km, p.b_km, m->stream);
  toc(m);
  return rc;
}

template <typename T> static inline T* W(Model* m, int64_t off) { return (T*)m->Sh + off; }
template <typename T> static inline T* AT(void* p) { return (T*)p; }
template <typename T> static inline T* WT(Model* m, int64_t off) { return (T*)m->ShT + off; }

// AttnParams of layer l over the resident batch: shape, ids and tile maps of the token order -- the batch's own, or the selected-first
// order of the last layer under the compact top --, and the layer's q | k | v, O and log-sum-exp.  Callers add what is theirs alone:
// q_active, the fp8 amax slot, the backward's gradient and RoPE fields.
enum TokenOrder { TOKENS_BATCH, TOKENS_SELECTED_FIRST };
template <typename T>
static AttnParams layer_attn(Model* m, int l, TokenOrder order) {
  const Model::LayerAct& a = m->la[l];
  const bool sel = order == TOKENS_SELECTED_FIRST;
  AttnParams ap{};
  ap.B = m->cur_rows; ap.T = m->T; ap.H = m->H; ap.KV = m->KV; ap.hd = m->hd; ap.is_bf16 = is_bf16<T>::value ? 1 : 0;
  ap.uid = sel ? m->uid_p : m->uid_t; ap.tm = sel ? m->tm_p : m->tm_t;
  (sel ? m->maps_p : m->maps).apply(ap);
  ap.q = a.qkv; ap.k = AT<T>(a.qkv) + m->H * m->hd; ap.v = AT<T>(a.qkv) + (m->H + m->KV) * m->hd; ap.ld = m->Nqkv;
  ap.o = a.O; ap.ldo = m->D; ap.lse = a.lse;
  return ap;
}

// the eight fp8 products of a layer: amax slot(s) of the A operand (Model::f8_aamax), its column layout and format, the weight
// scale slot(s) (Model::f8_wamax: q k v o w1 w3 w2) and how the descales combine
enum { F8P_QKV = 0, F8P_O = 1, F8P_W13 = 2, F8P_W2 = 3, F8P_W2_DX = 4, F8P_W13_DX = 5, F8P_O_DX = 6, F8P_QKV_DX = 7 };
struct F8Op { int a_slot, layout, fmt, w_slot, n_w, desc_mode; };
static const F8Op kF8Ops[8] = {
  {0, F8_LAYOUT_PLAIN, F8_E4M3, 0, 3, 1},    // xn  . [Wq; Wk; Wv]^T
  {1, F8_LAYOUT_PLAIN, F8_E4M3, 3, 1, 1},    // O   . Wo^T
  {2, F8_LAYOUT_PLAIN, F8_E4M3, 4, 2, 1},    // hn  . [W1; W3]^T
  {3, F8_LAYOUT_PLAIN, F8_E4M3, 6, 1, 1},    // g   . W2^T
  {4, F8_LAYOUT_PLAIN, F8_E5M2, 6, 1, 2},    // dy  . W2
  {5, F8_LAYOUT_SWIGLU, F8_E5M2, 4, 2, 2},   // [da | db] . [W1; W3]   (two gradients, two weights: K segments)
  {7, F8_LAYOUT_PLAIN, F8_E5M2, 3, 1, 2},    // dh  . Wo
  {8, F8_LAYOUT_SEGS, F8_E5M2, 0, 3, 2},     // [dq | dk | dv] . [Wq; Wk; Wv]
};

// sharded amax slot `slot` of layer l (common.hpp f8_amax_note): producers add to it, the cast reads it
static inline float* f8_slot(Model* m, int l, int slot) { return m->f8_aamax + (int64_t)l * F8_AMAX_SHARDS * F8_AMAX_SHARD + slot; }
enum { F8S_XN = 0, F8S_O = 1, F8S_HN = 2, F8S_G = 3, F8S_DY2 = 4, F8S_DAB = 5, F8S_DH = 7, F8S_DQKV = 8 };

// One linear of the fp8 trunk.  `p` is the bf16 call (A = the bf16 operand [M][K], epilogue, outputs); the A operand is quantised
// (its amax first unless the producer already left it in the slot), the product runs on the fp8 pipeline with weight copy `w8`.
static int gemm_f8(Model* m, int l, int which, const char* tag, GemmParams p, const unsigned char* w8, long long ldw, bool amax_done = false) {
  const F8Op& o = kF8Ops[which];
  hipStream_t s = m->stream;
  F8Cast c{};
  c.src = p.A; c.ld_src = p.lda; c.rows = p.M; c.cols = p.K; c.rows_dev = p.m_dev; c.fmt = o.fmt; c.layout = o.layout;
  c.seg_cols = o.layout == F8_LAYOUT_SEGS ? m->KV * m->hd : 0; c.seg_rep = m->H / m->KV;   // (dq | dk | dv: units of one kv group)
  c.amax = f8_slot(m, l, o.a_slot); c.dst = m->a8; c.ld_dst = p.K;
  c.desc = m->f8_desc + (l * 8 + which) * 32; c.wamax = m->f8_wamax + l * 8 + o.w_slot; c.n_w = o.n_w; c.desc_mode = o.desc_mode;
  c.w_rep = which == F8P_QKV ? m->H / m->KV : 1;
  const bool tcopy = m->f8_dw && m->f8_tcopies && p.m_dev == nullptr && p.M % 128 == 0;
  if (tcopy) {   // K-contiguous copy for the weight gradient; the gradient operand's cast also writes that product's descales
    Model::F8T& t = m->f8t[l];
    unsigned char* const dst_t[8] = {t.xn, t.O, t.hn, t.g, t.gxt, t.dab, t.dht, t.dqkv};
    c.dst_t = dst_t[which]; c.ld_dst_t = m->f8_ldt;
    if (which >= F8P_W2_DX) {
      static const int x_slot[4] = {F8S_G, F8S_HN, F8S_O, F8S_XN};   // forward operand of w2, w13, o, qkv
      c.desc_dw = m->f8_desc_dw + (l * 4 + (which - F8P_W2_DX)) * 32;
      c.xamax = f8_slot(m, l, x_slot[which - F8P_W2_DX]);
      c.dw_units = which == F8P_W13_DX ? 2 : (which == F8P_QKV_DX ? m->H / m->KV + 2 : 1);
    }
  }
  tic(m, "hbm_f8_cast", ((amax_done ? 3.0 : 5.0) + (tcopy ? 1.0 : 0.0)) * p.M * (double)p.K);
  if (!amax_done) RC(launch_f8_amax(c, s));
  RC(launch_f8_cast(c, s));
  toc(m);
  p.A = m->a8; p.lda = p.K; p.B = w8; p.ldb = ldw;
  p.f8 = o.fmt == F8_E5M2 ? 2 : 1; p.f8_desc = c.desc;
  if (which == F8P_QKV) p.f8_seg_cols = m->KV * m->hd;
  if (which == F8P_W13) p.f8_alt = 1;
  if (which == F8P_W13_DX) p.f8_kb[0] = m->Ip / 128;
  if (which == F8P_QKV_DX) { p.f8_kb[0] = m->H * m->hd / 128; p.f8_kb[1] = (m->H + m->KV) * m->hd / 128; }
  if (p.alpha == 0.f) p.alpha = 1.f;
  p.splitk = 1;
  p.flags |= m->gemm_flags;
  if (m->timer.enabled) tic(m, (std::string(tag) + "@8f").c_str(), 2.0 * p.M * p.N * (double)p.K);
  const int rc = launch_gemm8p_f8(p, s);
  toc(m);
  return rc;
}
// weight gradient of linear `k` (0 w2, 1 w13, 2 o, 3 qkv) of layer l from the transposed fp8 copies: dW += q(dY)^T . q(X), K = tokens
static GemmParams f8_dw_params(Model* m, int l, int k, int NT) {
  const Model::F8T& t = m->f8t[l];
  const int D = m->D, Ip = m->Ip;
  GemmParams p{};
  p.lda = p.ldb = m->f8_ldt; p.K = NT; p.c_f32 = 1; p.epi = EPI_ATOMIC; p.alpha = 1.f; p.f8 = 2;
  p.f8_desc = m->f8_desc_dw + (l * 4 + k) * 32;
  float* G = m->f8_dw_stage ? m->f8_dw_stage - m->f8_dw_stage_base : m->G;   // (staged: f8_dw_round_accum moves it to the gradient)
  switch (k) {
    case 0: p.A = t.gxt; p.B = t.g; p.C = G + m->lo[l].w2; p.ldc = Ip; p.M = D; p.N = Ip; break;
    case 1: p.A = t.dab; p.B = t.hn; p.C = G + m->lo[l].w13; p.ldc = D; p.M = 2 * Ip; p.N = D; p.f8_rseg = Ip; p.f8_rowmode = 1; break;
    case 2: p.A = t.dht; p.B = t.O; p.C = G + m->lo[l].wo; p.ldc = D; p.M = D; p.N = D; break;
    default: p.A = t.dqkv; p.B = t.xn; p.C = G + m->lo[l].wqkv; p.ldc = D; p.M = m->Nqkv; p.N = D; p.f8_rseg = m->KV * m->hd; break;
  }
  return p;
}
// RSYS_F8_DW_ROUND_BF16: gradient[lo, hi) += bf16(staged product sums), stage back to zero (layers l_lo .. l_hi: their four weight
// tensors are contiguous, layers ascending)
static int f8_dw_round_accum(Model* m, int l_lo, int l_hi) {
  if (!m->f8_dw_stage) return RSYS_OK;
  const int64_t lo = m->lo[l_lo].wqkv, hi = m->lo[l_hi].w2 + pad8((int64_t)m->D * m->Ip);
  return launch_round_bf16_accum(m->f8_dw_stage + (lo - m->f8_dw_stage_base), m->G + lo, hi - lo, m->stream);
}
static inline bool use_f8_dw(const Model* m) { return m->f8_dw && !m->deterministic && m->cur_rows * 2 * m->S % 128 == 0; }
// one product at a time (layers whose products are large enough alone: the production shape)
static int f8_dw_launch(Model* m, int l, int k, const char* tag, int NT) {
  GemmParams p = f8_dw_params(m, l, k, NT);
  if (m->timer.enabled) tic(m, (std::string(tag) + "@8fs").c_str(), 2.0 * p.M * p.N * (double)p.K);
  const int rc = launch_gemm8p_f8_splitk(p, m->stream);
  toc(m);
  return rc;
}
static inline const unsigned char* W8(Model* m, int64_t off) { return m->W8 + (off - m->w8_base); }
static inline const unsigned char* W8T(Model* m, int64_t off) { return m->W8T + (off - m->w8_base); }

static SmallParams small_params(Model* m) {
  SmallParams sp;
  sp.per_cos = m->P + m->o_pcos; sp.per_sin = m->P + m->o_psin;
  sp.status_emb = m->P + m->o_status; sp.gender_emb = m->P + m->o_gender; sp.source_emb = m->P + m->o_source;
  sp.n_status = m->cfg.vocab_status; sp.n_gender = m->cfg.vocab_gender; sp.n_source = m->cfg.vocab_source;
  sp.min_ts = m->cfg.min_ts; sp.max_ts = m->cfg.max_ts;
  sp.rating_mean = m->cfg.rating_mean; sp.rating_std = m->cfg.rating_std;
  return sp;
}

// how many selected tokens to expect (K splits of the compact weight gradients only; the device-side count decides what is computed.
// The same hint for the row-limited GEMMs' kernel choice -- 128 x 128 tiles for ~3 K rows instead of 12 row tiles of 256 -- was
// measured and is not used: w2_dx 37 -> 72 us, w13_dx 57 -> 62 us): pretraining masks 2 * mask_rate of the interactions and a part of them carries a target; finetuning has one target per row
static int expected_selected(const Model* m) {
  const long long N = (long long)m->cur_rows * m->S;
  const long long e = m->cfg.finetune ? 2LL * m->cur_rows : (long long)(2.0 * m->cfg.mask_rate * (double)N * 0.6);
  return (int)std::max<long long>(256, std::min<long long>(m->ctop_cap, e));
}

// rows of medium `med` (global ids [0, V0) / [V0, V)) that this rank holds: `len` rows, the first one is id `col0` inside the
// medium and local table row `row` (replicated table: the whole medium)
static void shard_medium_range(const Model* m, int med, int* len, int* col0, int* row) {
  const int s = med == 0 ? 0 : m->V0, e = med == 0 ? m->V0 : m->V;
  const int a = std::max(s, m->row_lo), b = std::min(e, m->row_lo + m->TR);
  *len = std::max(0, b - a); *col0 = a - s; *row = a - m->row_lo;
  if (*len == 0) { *col0 = 0; *row = 0; }
}

// Packed rows: a segment owns whole 64-token tiles -- 32 interaction columns each -- of one row of S columns.
// owner [rows][nt] names the segment of every tile, -1 while it is free.  place() gives the tiles of columns [c0, c0 + n) of `row` to
// segment `id` and refuses a row outside the batch, a c0 that is negative or off a tile boundary, an end past the row and a tile that is
// taken; n == 0 places nothing.  `who` starts the refusal's text.  Host only: callers check every segment before their first launch.
struct TileOwners {
  int rows, S, nt;
  std::vector<int> owner;
  TileOwners(int rows_, int S_) : rows(rows_), S(S_), nt((S_ + 31) / 32), owner((size_t)rows_ * ((S_ + 31) / 32), -1) {}
  int place(const char* who, int row, int c0, int n, int id) {
    const std::string w = std::string(who) + ": ";
    ARG_CHECK(row >= 0 && row < rows, w + "a segment's row is outside the resident batch");
    ARG_CHECK(c0 >= 0 && c0 % 32 == 0, w + "a segment starts at an interaction column that is a multiple of 32");
    ARG_CHECK(n >= 0 && (long long)c0 + n <= S, w + "a segment lies inside its row");
    for (int t = c0 / 32; t < (c0 + n + 31) / 32; ++t) {
      ARG_CHECK(owner[(size_t)row * nt + t] < 0, w + "two segments share a 64-token tile");
      owner[(size_t)row * nt + t] = id;
    }
    return RSYS_OK;
  }
};

// ---- defined in model_forward.hip
template <typename T> int table_forward(Model* m);
template <typename T> int forward_trunk(Model* m);
template <typename T> int heads(Model* m, int evaluate, const float tw[4]);
template <typename T> int sharded_counts_early(Model* m, bool train, const float tw[4]);
int select_positions_all(Model* m);
// ---- defined in model_backward.hip
template <typename T> int backward_trunk(Model* m);

// ---- defined in retrieve.hip: what the request paths share (rsys_retrieve_topk / _request, rsys_rank_request, rsys_retrieve_target_rank,
// rsys_render_request)
// The device arrays of query scoring: the queries in fp32 and in the compute type (the same array in fp32 mode), one log-sum-exp per query,
// the partials and the score slab z [rows][ldz] of one chunk of RETRIEVE_CHUNK queries.
static inline long long score_ldz(const Model* m) { return pad8(std::max(m->V0, m->V1)); }   // row stride of the score slab, either medium
template <typename T> struct ScoreBufs {
  float* qf = nullptr; T* qt = nullptr; float* lse = nullptr; float2* part = nullptr; float* z = nullptr;
  long long ldz; int D;
  explicit ScoreBufs(const Model* m) : ldz(score_ldz(m)), D(m->D) {}
  // nq == 0: nothing is scored (an empty piece each); z_bytes == 0: the rows of one chunk
  void take(Carve& c, int64_t nq, size_t z_bytes = 0) {
    qf = c.take<float>((size_t)nq * D);
    qt = is_bf16<T>::value ? c.take<T>((size_t)nq * D) : (T*)qf;
    lse = c.take<float>(nq);
    part = c.take<float2>(nq ? (size_t)RETRIEVE_CHUNK * RETRIEVE_LSE_SPLIT : 0);
    z = (float*)c.take<char>(z_bytes ? z_bytes : (size_t)std::min<int64_t>(nq, RETRIEVE_CHUNK) * ldz * 4);
  }
};
// The prologue of the chunk loop around retrieve_chunk_scores, in two calls because its callers enqueue them in different orders:
// the queries [nq][D] fp32 into b.qf (and cast into b.qt in bf16 mode), and the fused item table brought up to date, *Fm = the medium's rows.
template <typename T> int score_upload_queries(const ScoreBufs<T>& b, const float* queries, int64_t nq, hipMemcpyKind kind, hipStream_t s);
template <typename T> int score_table_ready(Model* m, int medium, const T** Fm);
// The queries of each group in query order (members[goff[g] .. goff[g + 1])) and, per chunk c of `chunk` queries, the part of them it
// holds (ranges[c * ng + g]); group == nullptr: query q is group q.  Fails on a group id outside [0, ng) and, unless allow_empty, on an
// empty group.
struct GroupPlan { std::vector<int> goff, members; std::vector<int2> ranges; int nchunks = 0; };
int group_plan(const char* who, const int32_t* group, int64_t nq, int ng, int chunk, GroupPlan& gp, bool allow_empty = false);
// Ragged lists of a request (offsets [n + 1] and parallel arrays): the words their error texts are built from
struct ListKind { const char *given, *offsets, *media, *ids; };
constexpr ListKind LIST_HISTORY{"the history arrays are all given or all NULL", "hist_offsets", "list items' media must be 0 or 1",
                                "list ids must be in [0, V) of their medium"};
constexpr ListKind LIST_SELECTED{"the selected-item arrays are all given or all NULL", "sel_offsets", "selected items' media must be 0 or 1",
                                 "selected ids must be in [0, V) of their medium"};
// (exclusion lists carry no media: check_list_items takes them with medium == nullptr and V = {V_m, unused})
constexpr ListKind LIST_EXCLUDED{"excl_offsets and excl_ids are both given or both NULL", "excl_offsets", "",
                                 "exclusion ids must be medium-local, in [0, V_m)"};
// off and `arrays` all given or all NULL; if given, off[0] == 0 and off non-decreasing over n rows
int check_ragged(const char* who, const ListKind& what, const int64_t* off, int64_t n, std::initializer_list<const void*> arrays);
// every item's medium in {0, 1} and id in [0, V[medium]); medium == nullptr: ids in [0, V[0]).  off == nullptr: nothing to check
int check_list_items(const char* who, const ListKind& what, const int64_t* off, int64_t n, const int32_t* medium, const int32_t* ids,
                     const int V[2]);
// the two checks on a request's list value over n rows (users / groups), in the words of its kind
inline int check_ragged(const char* who, const HistoryList& l, int64_t n) {
  return check_ragged(who, LIST_HISTORY, l.off, n, {l.medium, l.ids, l.status});
}
inline int check_ragged(const char* who, const SelectedList& l, int64_t n) { return check_ragged(who, LIST_SELECTED, l.off, n, {l.medium, l.ids}); }
inline int check_list_items(const char* who, const HistoryList& l, int64_t n, const int V[2]) {
  return check_list_items(who, LIST_HISTORY, l.off, n, l.medium, l.ids, V);
}
inline int check_list_items(const char* who, const SelectedList& l, int64_t n, const int V[2]) {
  return check_list_items(who, LIST_SELECTED, l.off, n, l.medium, l.ids, V);
}
// A host CSC matrix checked (colptr, row indices in [0, n_rows) -- `rows` is that range in the caller's words --, values finite and >= 0)
// and reduced to the pattern of its non-zero entries: cp [n_cols + 1], rv
int csc_nonzero_pattern(const char* who, const char* rows, int64_t n_rows, int64_t n_cols, const int64_t* colptr, const int32_t* rowval,
                        const float* nzval, std::vector<int64_t>& cp, std::vector<int32_t>& rv);

}  // namespace rsys
