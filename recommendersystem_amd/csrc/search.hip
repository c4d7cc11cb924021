// Search model on the device (Training/search/train.py:76-130: `SearchModel.forward`, the AdamW step of `train_epoch` and
// `generate_embeddings`), one handle per medium (rsys_search_*), independent of rsys_model, on the core of encoder_handle.hpp (parameters,
// AdamW, the feature table, the ordered split-K product).  The reference forms W = E Wenc^T [V][Q] every
// step and soft-maxes x W^T over both media; every label of a batch lies in the handle's medium, so the other medium's columns carry
// neither loss nor gradient, and x W^T = (x Wenc) E_m^T.  The pipeline:
//   project    P = x Wenc [B][D] through launch_gemm (bf16 mode: bf16 operands, fp32 accumulation, bf16 output)
//   scores     z = P E_m^T [B][V_m] through launch_gemm into an fp32 slab (never rounded); the logits are z exp(logit_scale)
//   stats      per (row, column split) the online (max, sum exp, sum exp * logit); merged per row in split order
//   finish     lse, the row's loss w (lse - logit[y]) and d logit_scale share w (sum p logit - logit[y]); the batch sums in a fixed order
//   grad       G = w (softmax - onehot) in the operand dtype, zero in the padding
//   dP         = exp(logit_scale) G E_m through launch_gemm (K = V_m: split-K partial tiles to a slab, summed in split order)
//   dWenc     += x^T dP through launch_gemm (K-major operands)
//   export     E_m Wenc^T in fp32, chunks of rows, one wait at the end
//   topk       log_softmax of the factored scores of query rows, then the selection of retrieve.hip (topk_rows)
//   texts      the logits and lse of the 1-64 text queries of a request (rsys_query_texts_set): the projection above, then
//              one streaming pass over E_m per tile of up to 8 texts (text_scores_kernel) instead of the 256-row GEMM and its slab
// Every reduction runs in a fixed order: a call is bitwise reproducible.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "encoder_handle.hpp"

namespace rsys {

namespace {

constexpr int SEARCH_MAXB = 4096;
constexpr int SEARCH_MAXSPLIT = 64;        // column splits of a row in the statistics kernel
constexpr int SEARCH_GRAD_COLS = 4096;     // columns per workgroup of the gradient kernel
constexpr int SEARCH_EXPORT_ROWS = 8192;   // ids per GEMM of the export
constexpr int SEARCH_TOPK_MAXK = 8192;     // topk_rows' limit

struct RowStat { float m, s, t; };   // running maximum, sum exp(v - m), sum exp(v - m) v

// The logit of a raw score: one rounded product, the same value in every kernel.  Written as z * sc the compiler contracts it into the
// subtraction that follows (fma(z, sc, -lse)), which keeps the product's unrounded bits there but not in the maximum lse is built from:
// lse - logit[y] is then the product's rounding error instead of 0 where one item holds all the mass, and the loss can be negative.
// (HIP's __fmul_rn is a plain product, so the pragma.)
__device__ __forceinline__ float search_logit(float z, float sc) {
#pragma clang fp contract(off)
  return z * sc;
}

__device__ __forceinline__ RowStat stat_merge(RowStat a, RowStat b) {
  RowStat r;
  r.m = fmaxf(a.m, b.m);
  const float fa = a.m == -INFINITY ? 0.f : expf(a.m - r.m), fb = b.m == -INFINITY ? 0.f : expf(b.m - r.m);
  r.s = a.s * fa + b.s * fb;
  r.t = a.t * fa + b.t * fb;
  return r;
}

// part[row][split] = the statistics of the logits z[row][c] * exp(*ls) over the split's columns [split * cps, min(V, (split + 1) * cps));
// cps % 4 == 0 and ldz % 4 == 0 (float4 loads).  One workgroup per (split, row); the lanes' values are merged by a butterfly, the
// waves' in wave order.
__global__ void __launch_bounds__(256) search_stats_kernel(const float* __restrict__ z, long long ldz, int V, int cps,
                                                           const float* __restrict__ ls, float4* __restrict__ part) {
  const int row = blockIdx.y, split = blockIdx.x;
  const int c0 = split * cps, c1 = min(V, c0 + cps);
  const float sc = expf(*ls);
  const float* zr = z + (long long)row * ldz;
  RowStat a{-INFINITY, 0.f, 0.f};
  for (int c = c0 + 4 * (int)threadIdx.x; c < c1; c += 1024) {
    float v[4];
    if (c + 3 < c1) {
      const float4 q = *(const float4*)(zr + c);
      v[0] = search_logit(q.x, sc); v[1] = search_logit(q.y, sc); v[2] = search_logit(q.z, sc); v[3] = search_logit(q.w, sc);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = c + k < c1 ? search_logit(zr[c + k], sc) : -INFINITY;
    }
    const float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (mx > a.m) {
      const float r = expf(a.m - mx);   // (exp(-inf) = 0 on the first visit)
      a.s *= r; a.t *= r; a.m = mx;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (v[k] != -INFINITY) {
        const float e = expf(v[k] - a.m);
        a.s += e; a.t += e * v[k];
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RowStat b;
    b.m = __shfl_xor(a.m, o, 64); b.s = __shfl_xor(a.s, o, 64); b.t = __shfl_xor(a.t, o, 64);
    a = stat_merge(a, b);
  }
  __shared__ RowStat ws[4];
  if (lane_id() == 0) ws[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    RowStat r = ws[0];
    for (int w = 1; w < 4; ++w) r = stat_merge(r, ws[w]);
    part[(long long)row * gridDim.x + split] = make_float4(r.m, r.s, r.t, 0.f);
  }
}

// per row: the splits merged in split order -> lse[row]; with labels: the row's loss wn (lse - logit[y]) and its d logit_scale share
// wn (sum_j p_j logit_j - logit[y]); out[0] = the batch loss, and with grads *dls += the batch share, both summed per thread over the
// rows r, r + 1024, ... in fp64 and then over the threads in thread order.  One workgroup.
__global__ void __launch_bounds__(1024) search_finish_kernel(const float4* __restrict__ part, int nsplit, int B, const float* __restrict__ z,
                                                             long long ldz, const int* __restrict__ labels, const float* __restrict__ wn,
                                                             const float* __restrict__ ls, float* __restrict__ lse, float* out, float* dls,
                                                             int grads) {
  __shared__ double sl[1024], sd[1024];
  const float sc = expf(*ls);
  double al = 0.0, ad = 0.0;
  for (int row = threadIdx.x; row < B; row += 1024) {
    const float4 p0 = part[(long long)row * nsplit];
    RowStat r{p0.x, p0.y, p0.z};
    for (int k = 1; k < nsplit; ++k) {
      const float4 pk = part[(long long)row * nsplit + k];
      r = stat_merge(r, RowStat{pk.x, pk.y, pk.z});
    }
    const float l = r.m + logf(r.s);
    lse[row] = l;
    if (labels) {
      const float zy = search_logit(z[(long long)row * ldz + labels[row]], sc), w = wn[row];
      al += (double)(w * (l - zy));
      ad += (double)(w * (r.t / r.s - zy));
    }
  }
  sl[threadIdx.x] = al; sd[threadIdx.x] = ad;
  __syncthreads();
  if (threadIdx.x == 0 && labels) {
    double tl = 0.0, td = 0.0;
    for (int i = 0; i < 1024; ++i) { tl += sl[i]; td += sd[i]; }
    out[0] = (float)tl;
    if (grads) *dls += (float)td;
  }
}

__device__ __forceinline__ void search_store4(float* p, const float v[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void search_store4(bf16* p, const float v[4]) {
  bf16x4 t; t[0] = (bf16)v[0]; t[1] = (bf16)v[1]; t[2] = (bf16)v[2]; t[3] = (bf16)v[3];
  *(bf16x4*)p = t;
}

// G[row][c] = T(wn[row] (exp(z[row][c] exp(*ls) - lse[row]) - [c == labels[row]])) for row < B = gridDim.y and c < V; zero for the
// padding columns [V, Vpad).  Vpad % 4 == 0, ldz == ldg == Vpad.
template <typename T>
__global__ void __launch_bounds__(256) search_grad_kernel(const float* __restrict__ z, int Vpad, int V, int B, const int* __restrict__ labels,
                                                          const float* __restrict__ wn, const float* __restrict__ lse,
                                                          const float* __restrict__ ls, T* __restrict__ G) {
  const int row = blockIdx.y;
  const int c0 = blockIdx.x * SEARCH_GRAD_COLS, c1 = min(Vpad, c0 + SEARCH_GRAD_COLS);
  const bool live = row < B;
  const float sc = expf(*ls), l = live ? lse[row] : 0.f, w = live ? wn[row] : 0.f;
  const int y = live ? labels[row] : -1;
  const float* zr = z + (long long)row * Vpad;
  T* gr = G + (long long)row * Vpad;
  for (int c = c0 + 4 * (int)threadIdx.x; c < c1; c += 1024) {
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (live && c < V) {
      const float4 q = *(const float4*)(zr + c);
      const float zz[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c + k < V) v[k] = w * (expf(search_logit(zz[k], sc) - l) - (c + k == y ? 1.f : 0.f));
    }
    search_store4(gr + c, v);
  }
}

// dP[i] *= exp(*ls) (the fp32 gradient the debug hook returns), dPt[i] = T(dP[i]) when dPt is given
template <typename T>
__global__ void __launch_bounds__(256) search_scale_kernel(float* __restrict__ dP, T* __restrict__ dPt, long long n4, const float* __restrict__ ls) {
  const float sc = expf(*ls);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const float4 q = *(const float4*)(dP + 4 * i);
    const float v[4] = {q.x * sc, q.y * sc, q.z * sc, q.w * sc};
    search_store4(dP + 4 * i, v);
    if (dPt) search_store4(dPt + 4 * i, v);
  }
}

// z[row][c] = z[row][c] exp(*ls) - lse[row] for c < V: the log-probabilities the selection ranks
__global__ void __launch_bounds__(256) search_logp_kernel(float* __restrict__ z, long long ldz, int V, const float* __restrict__ lse,
                                                          const float* __restrict__ ls) {
  const int row = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= V) return;
  float* p = z + (long long)row * ldz + c;
  *p = search_logit(*p, expf(*ls)) - lse[row];
}

// ---- the rows of a request's text queries (rsys_query_texts_set): one to a few dozen queries, a decode shape
constexpr int TX_THREADS = 256;
constexpr int TX_ROWS = 4;            // items a wave scores at once (reuses each LDS read of a text four times)
constexpr int TX_MAXTQ = 8;           // texts per workgroup (largest tile)
constexpr int TX_LDS = 65536;         // the tile's P rows in fp32: 8 rows at D <= 2048, 4 up to 4096, 2 up to 8192 (powers of two only)
constexpr int TX_MAXN = 64;           // texts per call

// one 16-byte load of a table row as fp32 values: 4 floats, or 8 bf16 (a bf16 is the upper half of its float)
template <typename T> struct TextVec;
template <> struct TextVec<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void load(const float* p, float (&e)[4]) {
    const float4 q = *(const float4*)p;
    e[0] = q.x; e[1] = q.y; e[2] = q.z; e[3] = q.w;
  }
};
template <> struct TextVec<bf16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void load(const bf16* p, float (&e)[8]) {
    const uint4 q = *(const uint4*)p;
    const unsigned u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { e[2 * k] = __uint_as_float(u[k] << 16); e[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u); }
  }
};

// z[t][i] = search_logit(P_t . E[i], exp(*ls)) for the TQ texts t0 + [0, TQ) of this workgroup's tile and TX_ROWS items per wave step,
// i < V only (the padding rows of the table are never stored).  blockIdx.x = text tile, blockIdx.y = item block: the tiles of one item
// block run side by side and read its rows of E from HBM once.  The tile's rows of P are staged in LDS as fp32; lane l sums the 16-byte
// vectors l + 64 j (j ascending) of each product in column order, then a butterfly over the 64 lanes adds the partials: a fixed order,
// no atomics, the same bits whatever TQ.  D % 64 == 0.
template <typename T, int TQ>
__global__ void __launch_bounds__(TX_THREADS) text_scores_kernel(const T* __restrict__ P, int n, const T* __restrict__ E, int V, int D,
                                                                 int rows_per_block, const float* __restrict__ ls, float* __restrict__ z,
                                                                 long long ldz) {
  extern __shared__ float4 p4[];   // [TQ][D / 4]
  constexpr int N = TextVec<T>::N, H = N / 4;
  const int t0 = blockIdx.x * TQ, d4 = D >> 2, nv = D / N;
  for (int t = threadIdx.x; t < TQ * nv; t += TX_THREADS) {
    const int gg = t / nv, c = t - gg * nv;
    float e[N];
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = 0.f;
    if (t0 + gg < n) TextVec<T>::load(P + (long long)(t0 + gg) * D + (long long)c * N, e);
#pragma unroll
    for (int h = 0; h < H; ++h) p4[gg * d4 + c * H + h] = make_float4(e[4 * h], e[4 * h + 1], e[4 * h + 2], e[4 * h + 3]);
  }
  __syncthreads();
  const float sc = expf(*ls);
  const int w = threadIdx.x >> 6, lane = lane_id();
  const long long rb = (long long)blockIdx.y * rows_per_block;
  const long long rend = rb + rows_per_block < V ? rb + rows_per_block : V;
  for (long long r0 = rb + w * TX_ROWS; r0 < rend; r0 += (TX_THREADS / 64) * TX_ROWS) {
    float acc[TX_ROWS][TQ];
#pragma unroll
    for (int r = 0; r < TX_ROWS; ++r)
#pragma unroll
      for (int gg = 0; gg < TQ; ++gg) acc[r][gg] = 0.f;
    const T* er[TX_ROWS];
#pragma unroll
    for (int r = 0; r < TX_ROWS; ++r) er[r] = E + (r0 + r < V ? r0 + r : V - 1) * D;
    for (int c = lane; c < nv; c += 64) {
      float e[TX_ROWS][N];
#pragma unroll
      for (int r = 0; r < TX_ROWS; ++r) TextVec<T>::load(er[r] + (long long)c * N, e[r]);
#pragma unroll
      for (int gg = 0; gg < TQ; ++gg)
#pragma unroll
        for (int h = 0; h < H; ++h) {
          const float4 s = p4[gg * d4 + c * H + h];
#pragma unroll
          for (int r = 0; r < TX_ROWS; ++r) {
            float a = acc[r][gg];
            a = fmaf(e[r][4 * h], s.x, a); a = fmaf(e[r][4 * h + 1], s.y, a); a = fmaf(e[r][4 * h + 2], s.z, a); a = fmaf(e[r][4 * h + 3], s.w, a);
            acc[r][gg] = a;
          }
        }
    }
    float out = 0.f;
#pragma unroll
    for (int r = 0; r < TX_ROWS; ++r)
#pragma unroll
      for (int gg = 0; gg < TQ; ++gg) {
        float v = acc[r][gg];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == r * TQ + gg) out = v;
      }
    const int r = lane / TQ, gg = lane - r * TQ;
    if (r < TX_ROWS && r0 + r < rend && t0 + gg < n) z[(long long)(t0 + gg) * ldz + r0 + r] = search_logit(out, sc);
  }
}

}  // namespace

// ------------------------------------------------------------------ the handle
struct SearchModel : EncoderCore {
  int V = 0, Vpad = 0, D = 0, Q = 0, maxb = 0, bcap = 0;   // E_m [Vpad][D] (rows >= V zero), Wenc [Q][D]
  bf16* feat16 = nullptr;                           // bf16 copy of E_m (bf16 mode)
  float* X32 = nullptr; void* Xt = nullptr;         // queries [bcap][Q]: the fp32 upload and the operand (the same buffer in fp32 mode)
  void* Pt = nullptr;                               // x Wenc [bcap][D] in the operand dtype
  float* z = nullptr;                               // scores [bcap][Vpad] fp32
  void* Gs = nullptr;                               // w (softmax - onehot) [bcap][Vpad] in the operand dtype
  float* dP = nullptr; void* dPt = nullptr;         // [bcap][D]: fp32 sum, operand copy (bf16 mode)
  float4* part = nullptr;
  int* labels = nullptr; float *wn = nullptr, *lse = nullptr, *loss = nullptr;
  float* exp32 = nullptr;                           // export [V][Q], allocated by the first export
  DevScratch tws;                                   // top-k workspace
  int last_B = 0; bool last_grads = false;
  int last_nsplit = 0, last_ksplits = 0;            // of the last call: statistics splits; K splits of dP as routed, 0 without a backward
  int g_rows = 0;                                   // rows of Gs an earlier call wrote (the rest is zero)
  std::vector<float> h_wn;                          // host source of a call's upload, alive until its closing wait
  void free_own() override {
    tws.release();
    if (exp32) hipFree(exp32);
  }
  int features_ready() override {                   // the bf16 operand copy of the table
    if (bf16_mode()) ENC_RC(launch_cast<bf16>(feat, feat16, (long long)Vpad * D, stream));
    return EncoderCore::features_ready();
  }
};

static int search_create(int64_t V, int32_t D, int32_t Q, int32_t dtype, int32_t maxb, int32_t device, void** out) {
  ARG_CHECK(out, "rsys_search_create: null output");
  ARG_CHECK(V >= 1 && V <= (1 << 24), "rsys_search_create: 1 <= V_m <= 2^24");
  ARG_CHECK(D >= 64 && D % 64 == 0 && D <= 8192, "rsys_search_create: D must be a multiple of 64 in [64, 8192] (2048: the transformer's embed_dim)");
  ARG_CHECK(Q >= 64 && Q % 64 == 0 && Q <= 16384, "rsys_search_create: Q must be a multiple of 64 in [64, 16384] (3072: the query embeddings)");
  ARG_CHECK(maxb >= 1 && maxb <= SEARCH_MAXB, "rsys_search_create: 1 <= max_batch <= 4096");
  ENC_RC(enc_check_device("rsys_search", dtype, device));
  SearchModel* h = new SearchModel();
  h->V = (int)V; h->Vpad = (int)((V + 255) / 256 * 256); h->D = D; h->Q = Q; h->maxb = maxb;
  h->bcap = (maxb + 255) / 256 * 256;
  h->api = "rsys_search"; h->wname = "encoder.weight"; h->device = device; h->dtype = dtype;
  h->frows = V; h->fpad = h->Vpad; h->fcols = h->wcols = D; h->wrows = Q;
  const size_t tsz = h->bf16_mode() ? 2 : 4;
  const int rc = [&]() -> int {
    ENC_RC(enc_init(h, 1.f));   // logit_scale = 1.0 (train.py:85)
    if (h->bf16_mode()) ENC_ALLOC(h->feat16, (size_t)h->Vpad * D * 2);
    ENC_ALLOC(h->X32, (size_t)h->bcap * Q * 4);
    if (h->bf16_mode()) ENC_ALLOC(h->Xt, (size_t)h->bcap * Q * 2); else h->Xt = h->X32;
    ENC_ALLOC(h->Pt, (size_t)h->bcap * D * tsz);
    ENC_ALLOC(h->z, (size_t)h->bcap * h->Vpad * 4);
    ENC_ALLOC(h->Gs, (size_t)h->bcap * h->Vpad * tsz);
    ENC_ALLOC(h->dP, (size_t)h->bcap * D * 4);
    if (h->bf16_mode()) ENC_ALLOC(h->dPt, (size_t)h->bcap * D * 2); else h->dPt = h->dP;
    ENC_ALLOC(h->part, (size_t)h->bcap * SEARCH_MAXSPLIT * sizeof(float4));
    ENC_ALLOC(h->labels, h->bcap * 4); ENC_ALLOC(h->wn, h->bcap * 4); ENC_ALLOC(h->lse, h->bcap * 4); ENC_ALLOC(h->loss, 16);
    return RSYS_OK;
  }();
  if (rc != RSYS_OK) { enc_free(h); return rc; }
  *out = (EncoderCore*)h;
  return RSYS_OK;
}

// rows [0, B) of x uploaded, the operand copy made, rows [B, Bpad) of the operand zero
template <typename T>
static int search_upload_x(SearchModel* h, const float* x, int B, int Bpad) {
  hipStream_t s = h->stream;
  const long long n = (long long)B * h->Q;
  HIP_CHECK(hipMemcpyAsync(h->X32, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
  if (h->bf16_mode()) ENC_RC(launch_cast<bf16>(h->X32, (bf16*)h->Xt, n, s));
  if (Bpad > B) HIP_CHECK(hipMemsetAsync((T*)h->Xt + n, 0, (size_t)(Bpad - B) * h->Q * sizeof(T), s));
  return RSYS_OK;
}

// P = x Wenc over Bpad rows, in the operand dtype
template <typename T>
static int search_project(SearchModel* h, int Bpad) {
  const bool bf = h->bf16_mode();
  GemmParams p{};   // P[m][n] = sum_k x[m][k] Wenc[k][n]: Wenc is the K-major operand
  p.A = h->Xt; p.lda = h->Q;
  p.B = bf ? (const void*)h->Wsh : (const void*)h->P; p.ldb = h->D;
  p.C = h->Pt; p.ldc = h->D; p.c_f32 = bf ? 0 : 1;
  p.M = Bpad; p.N = h->D; p.K = h->Q; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
  return launch_gemm<T>(p, false, false, false, true, h->stream);
}

// P = x Wenc and z = P E_m^T over Bpad rows, then the row statistics and lse of rows [0, B); with labels also the loss
template <typename T>
static int search_scores(SearchModel* h, int B, int Bpad, bool with_loss, bool grads, int* nsplit_out) {
  hipStream_t s = h->stream;
  const bool bf = h->bf16_mode();
  ENC_RC(search_project<T>(h, Bpad));
  {
    GemmParams p{};   // z[m][n] = sum_k P[m][k] E[n][k]
    p.A = h->Pt; p.lda = h->D;
    p.B = bf ? (const void*)h->feat16 : (const void*)h->feat; p.ldb = h->D;
    p.C = h->z; p.ldc = h->Vpad; p.c_f32 = 1;
    p.M = Bpad; p.N = h->Vpad; p.K = h->D; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
    ENC_RC(launch_gemm<T>(p, false, false, false, false, s));
  }
  // enough workgroups to fill the chip at small B, at least 1024 columns each
  int nsplit = std::max(1, std::min(SEARCH_MAXSPLIT, std::min((2048 + B - 1) / B, h->V / 1024)));
  const int cps = ((h->V + nsplit - 1) / nsplit + 3) / 4 * 4;
  nsplit = (h->V + cps - 1) / cps;
  search_stats_kernel<<<dim3(nsplit, B), 256, 0, s>>>(h->z, h->Vpad, h->V, cps, h->ls(), h->part);
  HIP_CHECK(hipGetLastError());
  search_finish_kernel<<<1, 1024, 0, s>>>(h->part, nsplit, B, h->z, h->Vpad, with_loss ? h->labels : nullptr, h->wn, h->ls(), h->lse, h->loss,
                                          h->G + h->nw(), grads ? 1 : 0);
  HIP_CHECK(hipGetLastError());
  h->last_nsplit = nsplit; h->last_ksplits = 0;
  if (nsplit_out) *nsplit_out = nsplit;
  return RSYS_OK;
}

template <typename T>
static int search_backward(SearchModel* h, int B, int Bpad) {
  hipStream_t s = h->stream;
  const bool bf = h->bf16_mode();
  // rows [B, Bpad) of G must be zero for the two products below: they are (hipMemset at creation) unless an earlier call wrote them
  if (h->g_rows > B) HIP_CHECK(hipMemsetAsync((T*)h->Gs + (long long)B * h->Vpad, 0, (size_t)(h->g_rows - B) * h->Vpad * sizeof(T), s));
  h->g_rows = B;
  search_grad_kernel<T><<<dim3((h->Vpad + SEARCH_GRAD_COLS - 1) / SEARCH_GRAD_COLS, B), 256, 0, s>>>(h->z, h->Vpad, h->V, B, h->labels, h->wn,
                                                                                                     h->lse, h->ls(), (T*)h->Gs);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemsetAsync(h->dP, 0, (size_t)Bpad * h->D * 4, s));
  {
    GemmParams p{};   // dP[m][n] = sum_k G[m][k] E[k][n]: E is the K-major operand, K = Vpad; ordered split-K through the slab
    p.A = h->Gs; p.lda = h->Vpad;
    p.B = bf ? (const void*)h->feat16 : (const void*)h->feat; p.ldb = h->D;
    p.C = h->dP; p.ldc = h->D; p.c_f32 = 1;
    p.M = Bpad; p.N = h->D; p.K = h->Vpad; p.epi = EPI_ATOMIC; p.alpha = 1.f;
    // K splits of at least 2048 items each until the chip has ~2048 workgroups of 128 x 128 outputs; whole XCDs (multiples of 8)
    const long long tiles = (long long)((Bpad + 127) / 128) * ((h->D + 127) / 128);
    const long long sk = std::min<long long>(64, std::min<long long>(h->Vpad / 2048, std::max<long long>(1, 2048 / tiles)));
    p.splitk = sk >= 8 ? (int)(sk / 8 * 8) : 1;
    ENC_RC(enc_ordered_gemm<T>(h, p, false, true, &h->last_ksplits));
  }
  search_scale_kernel<T><<<grid_for((long long)Bpad * h->D / 4), 256, 0, s>>>(h->dP, bf ? (T*)h->dPt : (T*)nullptr, (long long)Bpad * h->D / 4,
                                                                                h->ls());
  HIP_CHECK(hipGetLastError());
  {
    GemmParams p{};   // G[Wenc][m][n] += sum_k x[k][m] dP[k][n]: both operands K-major
    p.A = h->Xt; p.lda = h->Q;
    p.B = h->dPt; p.ldb = h->D;
    p.C = h->G; p.ldc = h->D; p.c_f32 = 1;
    p.M = h->Q; p.N = h->D; p.K = Bpad; p.epi = EPI_ATOMIC; p.alpha = 1.f; p.splitk = 1;
    ENC_RC(enc_ordered_gemm<T>(h, p, true, true));
  }
  return RSYS_OK;
}

static int search_forward_backward(SearchModel* h, const float* x, const int32_t* labels, const float* w, int B, int evaluate, float* loss_out,
                                   float* wsum_out) {
  ARG_CHECK(h->has_features, "rsys_search_forward_backward: features are not set (rsys_search_features_set)");
  ARG_CHECK(x && labels && w, "rsys_search_forward_backward: null buffer");
  ARG_CHECK(B >= 1 && B <= h->maxb, "rsys_search_forward_backward: 1 <= B <= max_batch");
  double W = 0.0;
  for (int i = 0; i < B; ++i) {
    ARG_CHECK(labels[i] >= 0 && labels[i] < h->V, "rsys_search_forward_backward: labels must be medium-local ids in [0, V_m)");
    ARG_CHECK(std::isfinite(w[i]) && w[i] >= 0.f, "rsys_search_forward_backward: weights must be finite and >= 0");
    W += w[i];
  }
  ARG_CHECK(W > 0.0, "rsys_search_forward_backward: the weights must not sum to 0");
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int Bpad = (B + 255) / 256 * 256;
  const bool grads = evaluate == 0;
  h->h_wn.resize(B);
  for (int i = 0; i < B; ++i) h->h_wn[i] = (float)((double)w[i] / W);
  HIP_CHECK(hipMemcpyAsync(h->labels, labels, (size_t)B * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(h->wn, h->h_wn.data(), (size_t)B * 4, hipMemcpyHostToDevice, s));
  if (h->bf16_mode()) {
    ENC_RC(search_upload_x<bf16>(h, x, B, Bpad));
    ENC_RC(search_scores<bf16>(h, B, Bpad, true, grads, nullptr));
    if (grads) ENC_RC(search_backward<bf16>(h, B, Bpad));
  } else {
    ENC_RC(search_upload_x<float>(h, x, B, Bpad));
    ENC_RC(search_scores<float>(h, B, Bpad, true, grads, nullptr));
    if (grads) ENC_RC(search_backward<float>(h, B, Bpad));
  }
  float l = 0.f;
  HIP_CHECK(hipMemcpyAsync(&l, h->loss, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  h->last_B = B; h->last_grads = grads;
  if (loss_out) *loss_out = l;
  if (wsum_out) *wsum_out = (float)W;
  return RSYS_OK;
}

static int search_export(SearchModel* h, float* out) {
  ARG_CHECK(h->has_features, "rsys_search_export: features are not set (rsys_search_features_set)");
  ARG_CHECK(out, "rsys_search_export: null output");
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (!h->exp32) HIP_CHECK(hipMalloc((void**)&h->exp32, (size_t)h->V * h->Q * 4));
  for (long long r0 = 0; r0 < h->V; r0 += SEARCH_EXPORT_ROWS) {
    const int rows = (int)std::min<long long>(SEARCH_EXPORT_ROWS, h->V - r0);
    GemmParams p{};   // out[m][n] = sum_k E[m][k] Wenc[n][k], fp32 in both modes
    p.A = h->feat + r0 * h->D; p.lda = h->D; p.B = h->P; p.ldb = h->D; p.C = h->exp32 + r0 * h->Q; p.ldc = h->Q; p.c_f32 = 1;
    p.M = rows; p.N = h->Q; p.K = h->D; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
    ENC_RC(launch_gemm<float>(p, false, false, false, false, s));
  }
  HIP_CHECK(hipMemcpyAsync(out, h->exp32, (size_t)h->V * h->Q * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

static int search_topk(SearchModel* h, const float* x, int nq, int k, int32_t* ids_out, float* logp_out) {
  ARG_CHECK(h->has_features, "rsys_search_topk: features are not set (rsys_search_features_set)");
  ARG_CHECK(x && ids_out && logp_out, "rsys_search_topk: null buffer");
  ARG_CHECK(nq >= 1 && nq <= h->maxb, "rsys_search_topk: 1 <= n_queries <= max_batch");
  ARG_CHECK(k >= 1 && k <= std::min(h->V, SEARCH_TOPK_MAXK), "rsys_search_topk: 1 <= k <= min(V_m, 8192)");
  for (long long i = 0; i < (long long)nq * h->Q; ++i) ARG_CHECK(std::isfinite(x[i]), "rsys_search_topk: the query embeddings must be finite");
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int Bpad = (nq + 255) / 256 * 256;
  void* ws; int *ids, *cnt; float* vals;
  ENC_RC(carve_into(h->tws, s, [&](Carve& c) {
    ws = c.take<char>(topk_rows_ws_bytes(nq, h->V, k));
    ids = c.take<int>((size_t)nq * k);
    vals = c.take<float>((size_t)nq * k);
    cnt = c.take<int>(nq);
  }));
  if (h->bf16_mode()) {
    ENC_RC(search_upload_x<bf16>(h, x, nq, Bpad));
    ENC_RC(search_scores<bf16>(h, nq, Bpad, false, false, nullptr));
  } else {
    ENC_RC(search_upload_x<float>(h, x, nq, Bpad));
    ENC_RC(search_scores<float>(h, nq, Bpad, false, false, nullptr));
  }
  search_logp_kernel<<<dim3((h->V + 255) / 256, nq), 256, 0, s>>>(h->z, h->Vpad, h->V, h->lse, h->ls());
  HIP_CHECK(hipGetLastError());
  ENC_RC(topk_rows(h->z, h->Vpad, nq, h->V, k, ws, ids, vals, cnt, s));
  HIP_CHECK(hipMemcpyAsync(ids_out, ids, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(logp_out, vals, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  h->last_B = nq; h->last_grads = false;
  return RSYS_OK;
}

// ---- text queries of a request
template <typename T, int TQ>
static int launch_text_tile(SearchModel* h, int n, const T* E, float* z) {
  int rpb = 64;   // items per workgroup; more only where the grid's y range needs it
  while (((long long)h->V + rpb - 1) / rpb > 65535) rpb *= 2;
  const dim3 grid((unsigned)((n + TQ - 1) / TQ), (unsigned)((h->V + rpb - 1) / rpb));
  text_scores_kernel<T, TQ><<<grid, TX_THREADS, (size_t)TQ * h->D * 4, h->stream>>>((const T*)h->Pt, n, E, h->V, h->D, rpb, h->ls(), z, h->V);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

// z [n][V_m] (logits, fp32) and lse [n] of n texts x [n][Q] (host) into device memory, on the handle's stream, no wait: the upload and
// the projection of rsys_search_topk, text_scores_kernel in tiles of TQ texts, the log-sum-exp launches of rsys_op_lse (part: n *
// RETRIEVE_LSE_SPLIT float2).  The caller has checked x and 1 <= n <= min(64, max_batch).
template <typename T>
static int search_text_rows_t(SearchModel* h, const float* x, int n, float* z, float2* part, float* lse) {
  const int Bpad = (n + 255) / 256 * 256;
  h->last_B = 0;   // (the handle's query and projection buffers are rewritten: rsys_search_debug_get has no forward to report)
  ENC_RC(search_upload_x<T>(h, x, n, Bpad));
  ENC_RC(search_project<T>(h, Bpad));
  const T* E = h->bf16_mode() ? (const T*)h->feat16 : (const T*)h->feat;
  // the largest power of two of texts that the call can use and whose fp32 rows fit the LDS tile (D <= 8192: at least two); the same
  // bits at every tile size
  const int fit = std::min({TX_MAXTQ, TX_LDS / (h->D * 4), n});
  int tq = 1;
  while (tq * 2 <= fit) tq *= 2;
  if (tq == 1) ENC_RC((launch_text_tile<T, 1>(h, n, E, z)));
  else if (tq == 2) ENC_RC((launch_text_tile<T, 2>(h, n, E, z)));
  else if (tq == 4) ENC_RC((launch_text_tile<T, 4>(h, n, E, z)));
  else ENC_RC((launch_text_tile<T, TX_MAXTQ>(h, n, E, z)));
  return lse_rows(z, h->V, n, h->V, part, lse, h->stream);
}

static int search_text_check(SearchModel* h, const char* who, const float* x, int64_t n) {
  const std::string w = std::string(who) + ": ";
  ARG_CHECK(h->has_features, w + "the search handle's features are not set (rsys_search_features_set)");
  ARG_CHECK(x != nullptr, w + "null embeddings");
  ARG_CHECK(n >= 1 && n <= std::min(TX_MAXN, h->maxb), w + "1 <= n_texts <= min(64, the handle's max_batch)");
  for (long long i = 0; i < (long long)n * h->Q; ++i) ARG_CHECK(std::isfinite(x[i]), w + "the text embeddings must be finite");
  return RSYS_OK;
}

static int search_text_rows(SearchModel* h, const float* x, int n, float* z, float2* part, float* lse) {
  return h->bf16_mode() ? search_text_rows_t<bf16>(h, x, n, z, part, lse) : search_text_rows_t<float>(h, x, n, z, part, lse);
}

// rsys_op_text_rows: the rows alone, to the host
static int op_text_rows(SearchModel* h, const float* x, int n, float* z_out, float* lse_out) {
  ARG_CHECK(z_out && lse_out, "rsys_op_text_rows: null output");
  ENC_RC(search_text_check(h, "rsys_op_text_rows", x, n));
  HIP_CHECK(hipSetDevice(h->device));
  DevScratch ws;
  float *z, *lse; float2* part;
  int rc = carve_into(ws, h->stream, [&](Carve& c) {
    z = c.take<float>((size_t)n * h->V);
    lse = c.take<float>(n);
    part = c.take<float2>((size_t)n * RETRIEVE_LSE_SPLIT);
  });
  if (rc == RSYS_OK) rc = search_text_rows(h, x, n, z, part, lse);
  if (rc == RSYS_OK && hipMemcpyAsync(z_out, z, (size_t)n * h->V * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = RSYS_ERR_HIP;
  if (rc == RSYS_OK && hipMemcpyAsync(lse_out, lse, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream) != hipSuccess) rc = RSYS_ERR_HIP;
  const hipError_t e = hipStreamSynchronize(h->stream);
  ws.release();
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("rsys_op_text_rows: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  return rc;
}

// rsys_query_texts_set: the rows of n texts into the model's buffer of `medium`, held with their groups and weights until the next
// request entry point takes them (capi.hip: PendingQueries).  A refused call holds nothing for the medium.
int model_query_texts_set(Model* m, void* search, int medium, const float* x, int64_t n, const int32_t* group, const float* w) {
  ARG_CHECK(medium == 0 || medium == 1, "query_texts_set: medium must be 0 or 1");
  TextSet& ts = m->qtexts[medium];
  ts.n = 0; ts.group.clear();
  if (n == 0) return RSYS_OK;
  SearchModel* h = static_cast<SearchModel*>((EncoderCore*)search);
  ARG_CHECK(h != nullptr, "query_texts_set: null search handle");
  ARG_CHECK(h->device == m->device, "query_texts_set: the search handle is on another device than the model");
  ARG_CHECK(h->V == (medium == 0 ? m->V0 : m->V1), "query_texts_set: the search handle's V_m is not the model's for this medium");
  ENC_RC(search_text_check(h, "query_texts_set", x, n));
  ARG_CHECK(group != nullptr, "query_texts_set: null groups");
  std::vector<float> wv((size_t)n, 1.f);
  if (w)
    for (int64_t i = 0; i < n; ++i) {
      ARG_CHECK(std::isfinite(w[i]), "query_texts_set: weights must be finite");
      wv[i] = w[i];
    }
  HIP_CHECK(hipSetDevice(m->device));
  float2* part;
  ENC_RC(carve_into(ts.buf, m->stream, [&](Carve& c) {
    ts.z = c.take<float>((size_t)n * h->V);
    ts.lse = c.take<float>(n);
    ts.d_w = c.take<float>(n);
    part = c.take<float2>((size_t)n * RETRIEVE_LSE_SPLIT);
  }));
  int rc = search_text_rows(h, x, (int)n, ts.z, part, ts.lse);
  if (rc == RSYS_OK && hipMemcpyAsync(ts.d_w, wv.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
    set_error("query_texts_set: the copy of the weights failed"); rc = RSYS_ERR_HIP;
  }
  const hipError_t e = hipStreamSynchronize(h->stream);   // the one wait: the model's stream reads the rows from here on
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("query_texts_set: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  if (rc != RSYS_OK) return rc;
  ts.n = (int)n; ts.ldz = h->V; ts.group.assign(group, group + n);
  return RSYS_OK;
}

static int search_debug_get(SearchModel* h, const char* name, float* out, int64_t n) {
  ARG_CHECK(name && out, "rsys_search_debug_get: null argument");
  ARG_CHECK(h->last_B > 0, "rsys_search_debug_get: no forward yet");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  if (strcmp(name, "lse") == 0) {
    ARG_CHECK(n == h->last_B, "rsys_search_debug_get: lse takes B floats of the last call");
    HIP_CHECK(hipMemcpy(out, h->lse, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RSYS_OK;
  }
  if (strcmp(name, "splits") == 0) {
    ARG_CHECK(n == 2, "rsys_search_debug_get: splits takes 2 floats");
    out[0] = (float)h->last_nsplit; out[1] = (float)h->last_ksplits;
    return RSYS_OK;
  }
  if (strcmp(name, "dP") == 0) {
    ARG_CHECK(h->last_grads, "rsys_search_debug_get: the last call ran no backward");
    ARG_CHECK(n == (long long)h->last_B * h->D, "rsys_search_debug_get: dP takes B * D floats of the last call");
    HIP_CHECK(hipMemcpy(out, h->dP, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RSYS_OK;
  }
  set_error(std::string("rsys_search_debug_get: unknown name '") + name + "' (lse, dP, splits)");
  return RSYS_ERR_ARG;
}

}  // namespace rsys

using namespace rsys;

extern "C" {

int32_t rsys_search_create(int64_t V, int32_t D, int32_t Q, int32_t dtype, int32_t max_batch, int32_t device, void** out) {
  return search_create(V, D, Q, dtype, max_batch, device, out);
}
int32_t rsys_search_destroy(void* hv) { enc_free((EncoderCore*)hv); return RSYS_OK; }
int32_t rsys_search_param_get(void* hv, const char* name, float* out, int64_t n) {
  ENC_HANDLE(SearchModel, hv); ARG_CHECK(out, "rsys_search_param_get: null output"); return enc_param_io(h, name, out, nullptr, n, 0);
}
int32_t rsys_search_param_set(void* hv, const char* name, const float* in, int64_t n) {
  ENC_HANDLE(SearchModel, hv); ARG_CHECK(in, "rsys_search_param_set: null input"); return enc_param_io(h, name, nullptr, in, n, 0);
}
int32_t rsys_search_grad_get(void* hv, const char* name, float* out, int64_t n) {
  ENC_HANDLE(SearchModel, hv); ARG_CHECK(out, "rsys_search_grad_get: null output"); return enc_param_io(h, name, out, nullptr, n, 1);
}
int32_t rsys_search_zero_grad(void* hv) { ENC_HANDLE(SearchModel, hv); return enc_zero_grad(h); }
int32_t rsys_search_features_set(void* hv, const float* features, int64_t V, int64_t D) {
  ENC_HANDLE(SearchModel, hv);
  return enc_features_set(h, features, V, D);
}
int32_t rsys_search_forward_backward(void* hv, const float* x, const int32_t* labels, const float* weights, int32_t B, int32_t evaluate,
                                     float* loss_out, float* weight_sum_out) {
  ENC_HANDLE(SearchModel, hv);
  return search_forward_backward(h, x, labels, weights, B, evaluate, loss_out, weight_sum_out);
}
int32_t rsys_search_adamw_create(void* hv, float beta1, float beta2, float eps, float weight_decay) {
  ENC_HANDLE(SearchModel, hv);
  ARG_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "rsys_search_adamw_create: betas must be in [0, 1)");
  ARG_CHECK(eps > 0.f && weight_decay >= 0.f, "rsys_search_adamw_create: eps > 0 and weight_decay >= 0");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  HIP_CHECK(hipMemset(h->M1, 0, (size_t)h->nflat * 4));
  HIP_CHECK(hipMemset(h->M2, 0, (size_t)h->nflat * 4));
  h->b1 = beta1; h->b2 = beta2; h->eps = eps; h->wd = weight_decay; h->adam_step = 0; h->has_adam = true;
  return RSYS_OK;
}
int32_t rsys_search_adamw_step(void* hv, float lr, float clip, float* norm_out, int32_t* skipped_out) {
  ENC_HANDLE(SearchModel, hv);
  return enc_adamw_step(h, lr, clip, norm_out, skipped_out);
}
int32_t rsys_search_adamw_state_get(void* hv, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step) {
  ENC_HANDLE(SearchModel, hv);
  ENC_RC(enc_adamw_state_io(h, name, exp_avg, exp_avg_sq, nullptr, nullptr, n));
  if (step) *step = h->adam_step;
  return RSYS_OK;
}
int32_t rsys_search_adamw_state_set(void* hv, const char* name, const float* exp_avg, const float* exp_avg_sq, int64_t n, int32_t step) {
  ENC_HANDLE(SearchModel, hv);
  ARG_CHECK(exp_avg && exp_avg_sq, "rsys_search_adamw_state_set: null input");
  ARG_CHECK(step >= 0, "rsys_search_adamw_state_set: step >= 0");
  ENC_RC(enc_adamw_state_io(h, name, nullptr, nullptr, exp_avg, exp_avg_sq, n));
  h->adam_step = step;
  return RSYS_OK;
}
int32_t rsys_search_export(void* hv, float* out) { ENC_HANDLE(SearchModel, hv); return search_export(h, out); }
int32_t rsys_search_topk(void* hv, const float* x, int32_t n_queries, int32_t k, int32_t* ids_out, float* logp_out) {
  ENC_HANDLE(SearchModel, hv);
  return search_topk(h, x, n_queries, k, ids_out, logp_out);
}
int32_t rsys_op_text_rows(void* hv, const float* x, int32_t n, float* z_out, float* lse_out) {
  ENC_HANDLE(SearchModel, hv);
  return op_text_rows(h, x, n, z_out, lse_out);
}
int32_t rsys_search_debug_get(void* hv, const char* name, float* out, int64_t n) { ENC_HANDLE(SearchModel, hv); return search_debug_get(h, name, out, n); }

}  // extern "C"
