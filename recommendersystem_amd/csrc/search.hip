// Search model on the device (Training/search/train.py:76-130: `SearchModel.forward`, the AdamW step of `train_epoch` and
// `generate_embeddings`), one handle per medium (rsys_search_*), independent of rsys_model.  The reference forms W = E Wenc^T [V][Q] every
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
// Every reduction runs in a fixed order: a call is bitwise reproducible.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "model.hpp"

namespace rsys {

namespace {

#define SEARCH_RC(expr) do { int _rc = (expr); if (_rc != RSYS_OK) return _rc; } while (0)

constexpr int SEARCH_MAXB = 4096;
constexpr int SEARCH_MAXSPLIT = 64;        // column splits of a row in the statistics kernel
constexpr int SEARCH_GRAD_COLS = 4096;     // columns per workgroup of the gradient kernel
constexpr int SEARCH_EXPORT_ROWS = 8192;   // ids per GEMM of the export
constexpr int SEARCH_TOPK_MAXK = 8192;     // topk_rows' limit

struct RowStat { float m, s, t; };   // running maximum, sum exp(v - m), sum exp(v - m) v

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
      v[0] = q.x * sc; v[1] = q.y * sc; v[2] = q.z * sc; v[3] = q.w * sc;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = c + k < c1 ? zr[c + k] * sc : -INFINITY;
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
      const float zy = z[(long long)row * ldz + labels[row]] * sc, w = wn[row];
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
        if (c + k < V) v[k] = w * (expf(zz[k] * sc - l) - (c + k == y ? 1.f : 0.f));
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
  *p = *p * expf(*ls) - lse[row];
}

inline unsigned search_grid(long long work, int per_block = 256, long long cap = 8192) {
  return (unsigned)std::max<long long>(1, std::min<long long>((work + per_block - 1) / per_block, cap));
}

}  // namespace

// ------------------------------------------------------------------ the handle
struct SearchModel {
  int device = 0, V = 0, Vpad = 0, D = 0, Q = 0, dtype = 0, maxb = 0, bcap = 0;
  hipStream_t stream = nullptr;
  long long nflat = 0;                              // [Wenc (Q x D) | logit_scale | 3 pad]
  float *feat = nullptr;                            // E_m [Vpad][D] fp32, rows >= V zero
  bf16* feat16 = nullptr;                           // bf16 copy (bf16 mode)
  float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr;
  bf16* Wsh = nullptr;                              // bf16 copy of Wenc (bf16 mode)
  bool has_features = false, has_adam = false;
  float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f, wd = 0.1f;
  int adam_step = 0;
  float *sumsq = nullptr, *sq_part = nullptr;
  float* X32 = nullptr; void* Xt = nullptr;         // queries [bcap][Q]: the fp32 upload and the operand (the same buffer in fp32 mode)
  void* Pt = nullptr;                               // x Wenc [bcap][D] in the operand dtype
  float* z = nullptr;                               // scores [bcap][Vpad] fp32
  void* Gs = nullptr;                               // w (softmax - onehot) [bcap][Vpad] in the operand dtype
  float* dP = nullptr; void* dPt = nullptr;         // [bcap][D]: fp32 sum, operand copy (bf16 mode)
  float4* part = nullptr;
  int* labels = nullptr; float *wn = nullptr, *lse = nullptr, *loss = nullptr;
  float* slab = nullptr; long long slab_floats = 0;
  float* exp32 = nullptr;                           // export [V][Q], allocated by the first export
  void* tws = nullptr; size_t tws_bytes = 0;        // top-k workspace, grown on demand
  int last_B = 0; bool last_grads = false;
  int g_rows = 0;                                   // rows of Gs an earlier call wrote (the rest is zero)
  std::vector<float> h_wn;                          // host source of a call's upload, alive until its closing wait
  std::vector<void*> allocs;
  bool bf16_mode() const { return dtype == RSYS_DTYPE_BF16; }
  float* ls() const { return P + (long long)Q * D; }
};

static int search_alloc(SearchModel* h, void** p, size_t bytes) {
  bytes = std::max<size_t>(256, (bytes + 255) / 256 * 256);
  HIP_CHECK(hipMalloc(p, bytes));
  HIP_CHECK(hipMemset(*p, 0, bytes));
  h->allocs.push_back(*p);
  return RSYS_OK;
}
#define SEARCH_ALLOC(ptr, bytes) SEARCH_RC(search_alloc(h, (void**)&(ptr), (size_t)(bytes)))

static void search_free(SearchModel* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (void* p : h->allocs) hipFree(p);
  if (h->slab) hipFree(h->slab);
  if (h->exp32) hipFree(h->exp32);
  if (h->tws) hipFree(h->tws);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

static int search_create(int64_t V, int32_t D, int32_t Q, int32_t dtype, int32_t maxb, int32_t device, SearchModel** out) {
  ARG_CHECK(out, "rsys_search_create: null output");
  ARG_CHECK(V >= 1 && V <= (1 << 24), "rsys_search_create: 1 <= V_m <= 2^24");
  ARG_CHECK(D >= 64 && D % 64 == 0 && D <= 8192, "rsys_search_create: D must be a multiple of 64 in [64, 8192] (2048: the transformer's embed_dim)");
  ARG_CHECK(Q >= 64 && Q % 64 == 0 && Q <= 16384, "rsys_search_create: Q must be a multiple of 64 in [64, 16384] (3072: the query embeddings)");
  ARG_CHECK(dtype == RSYS_DTYPE_FP32 || dtype == RSYS_DTYPE_BF16, "rsys_search_create: dtype must be RSYS_DTYPE_FP32 or RSYS_DTYPE_BF16");
  ARG_CHECK(maxb >= 1 && maxb <= SEARCH_MAXB, "rsys_search_create: 1 <= max_batch <= 4096");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("rsys_search_create: no HIP device visible"); return RSYS_ERR_HIP; }
  ARG_CHECK(device >= 0 && device < ndev, "rsys_search_create: device index out of range");
  HIP_CHECK(hipSetDevice(device));
  SearchModel* h = new SearchModel();
  h->device = device; h->V = (int)V; h->Vpad = (int)((V + 255) / 256 * 256); h->D = D; h->Q = Q; h->dtype = dtype; h->maxb = maxb;
  h->bcap = (maxb + 255) / 256 * 256;
  h->nflat = (long long)Q * D + 4;
  const size_t tsz = h->bf16_mode() ? 2 : 4;
  const int rc = [&]() -> int {
    HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    SEARCH_ALLOC(h->feat, (size_t)h->Vpad * D * 4);
    if (h->bf16_mode()) SEARCH_ALLOC(h->feat16, (size_t)h->Vpad * D * 2);
    SEARCH_ALLOC(h->P, h->nflat * 4); SEARCH_ALLOC(h->G, h->nflat * 4); SEARCH_ALLOC(h->M1, h->nflat * 4); SEARCH_ALLOC(h->M2, h->nflat * 4);
    if (h->bf16_mode()) SEARCH_ALLOC(h->Wsh, h->nflat * 2);
    SEARCH_ALLOC(h->sumsq, 16); SEARCH_ALLOC(h->sq_part, (size_t)sumsq_parts() * 4);
    SEARCH_ALLOC(h->X32, (size_t)h->bcap * Q * 4);
    if (h->bf16_mode()) SEARCH_ALLOC(h->Xt, (size_t)h->bcap * Q * 2); else h->Xt = h->X32;
    SEARCH_ALLOC(h->Pt, (size_t)h->bcap * D * tsz);
    SEARCH_ALLOC(h->z, (size_t)h->bcap * h->Vpad * 4);
    SEARCH_ALLOC(h->Gs, (size_t)h->bcap * h->Vpad * tsz);
    SEARCH_ALLOC(h->dP, (size_t)h->bcap * D * 4);
    if (h->bf16_mode()) SEARCH_ALLOC(h->dPt, (size_t)h->bcap * D * 2); else h->dPt = h->dP;
    SEARCH_ALLOC(h->part, (size_t)h->bcap * SEARCH_MAXSPLIT * sizeof(float4));
    SEARCH_ALLOC(h->labels, h->bcap * 4); SEARCH_ALLOC(h->wn, h->bcap * 4); SEARCH_ALLOC(h->lse, h->bcap * 4); SEARCH_ALLOC(h->loss, 16);
    const float ls = 1.f;   // logit_scale = 1.0 (train.py:85); Wenc stays zero until set
    HIP_CHECK(hipMemcpy(h->ls(), &ls, 4, hipMemcpyHostToDevice));
    return RSYS_OK;
  }();
  if (rc != RSYS_OK) { search_free(h); return rc; }
  *out = h;
  return RSYS_OK;
}

// the bf16 operand copy of the feature table after feat changed; the stream is idle on return
static int search_features_ready(SearchModel* h) {
  if (h->bf16_mode()) SEARCH_RC(launch_cast<bf16>(h->feat, h->feat16, (long long)h->Vpad * h->D, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  h->has_features = true;
  return RSYS_OK;
}

static int search_slab(SearchModel* h, long long need) {
  if (need <= h->slab_floats) return RSYS_OK;
  HIP_CHECK(hipStreamSynchronize(h->stream));
  if (h->slab) HIP_CHECK(hipFree(h->slab));
  h->slab = nullptr; h->slab_floats = 0;
  HIP_CHECK(hipMalloc((void**)&h->slab, (size_t)need * 4));
  h->slab_floats = need;
  return RSYS_OK;
}

// A product whose sum must have a fixed order (EPI_ATOMIC into fp32 C): with a slab in its parameters launch_gemm stays off the
// split-K forms that add partial tiles with float atomics (gemm8p's mixed-layout form, gemm4k), and every K split stores its partial
// tile into the slab, summed in split order afterwards.  The slab is grown to what the routed kernel needs.
template <typename T>
static int search_ordered_gemm(SearchModel* h, GemmParams p, bool a_km, bool b_km) {
  SEARCH_RC(search_slab(h, 256));
  p.slab = h->slab; p.slab_floats = h->slab_floats;
  SEARCH_RC(search_slab(h, std::max<long long>(256, gemm_slab_need<T>(p, false, false, a_km, b_km))));
  p.slab = h->slab; p.slab_floats = h->slab_floats;
  return launch_gemm<T>(p, false, false, a_km, b_km, h->stream);
}

// rows [0, B) of x uploaded, the operand copy made, rows [B, Bpad) of the operand zero
template <typename T>
static int search_upload_x(SearchModel* h, const float* x, int B, int Bpad) {
  hipStream_t s = h->stream;
  const long long n = (long long)B * h->Q;
  HIP_CHECK(hipMemcpyAsync(h->X32, x, (size_t)n * 4, hipMemcpyHostToDevice, s));
  if (h->bf16_mode()) SEARCH_RC(launch_cast<bf16>(h->X32, (bf16*)h->Xt, n, s));
  if (Bpad > B) HIP_CHECK(hipMemsetAsync((T*)h->Xt + n, 0, (size_t)(Bpad - B) * h->Q * sizeof(T), s));
  return RSYS_OK;
}

// P = x Wenc and z = P E_m^T over Bpad rows, then the row statistics and lse of rows [0, B); with labels also the loss
template <typename T>
static int search_scores(SearchModel* h, int B, int Bpad, bool with_loss, bool grads, int* nsplit_out) {
  hipStream_t s = h->stream;
  const bool bf = h->bf16_mode();
  {
    GemmParams p{};   // P[m][n] = sum_k x[m][k] Wenc[k][n]: Wenc is the K-major operand
    p.A = h->Xt; p.lda = h->Q;
    p.B = bf ? (const void*)h->Wsh : (const void*)h->P; p.ldb = h->D;
    p.C = h->Pt; p.ldc = h->D; p.c_f32 = bf ? 0 : 1;
    p.M = Bpad; p.N = h->D; p.K = h->Q; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
    SEARCH_RC(launch_gemm<T>(p, false, false, false, true, s));
  }
  {
    GemmParams p{};   // z[m][n] = sum_k P[m][k] E[n][k]
    p.A = h->Pt; p.lda = h->D;
    p.B = bf ? (const void*)h->feat16 : (const void*)h->feat; p.ldb = h->D;
    p.C = h->z; p.ldc = h->Vpad; p.c_f32 = 1;
    p.M = Bpad; p.N = h->Vpad; p.K = h->D; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
    SEARCH_RC(launch_gemm<T>(p, false, false, false, false, s));
  }
  // enough workgroups to fill the chip at small B, at least 1024 columns each
  int nsplit = std::max(1, std::min(SEARCH_MAXSPLIT, std::min((2048 + B - 1) / B, h->V / 1024)));
  const int cps = ((h->V + nsplit - 1) / nsplit + 3) / 4 * 4;
  nsplit = (h->V + cps - 1) / cps;
  search_stats_kernel<<<dim3(nsplit, B), 256, 0, s>>>(h->z, h->Vpad, h->V, cps, h->ls(), h->part);
  HIP_CHECK(hipGetLastError());
  search_finish_kernel<<<1, 1024, 0, s>>>(h->part, nsplit, B, h->z, h->Vpad, with_loss ? h->labels : nullptr, h->wn, h->ls(), h->lse, h->loss,
                                          h->G + (long long)h->Q * h->D, grads ? 1 : 0);
  HIP_CHECK(hipGetLastError());
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
    SEARCH_RC(search_ordered_gemm<T>(h, p, false, true));
  }
  search_scale_kernel<T><<<search_grid((long long)Bpad * h->D / 4), 256, 0, s>>>(h->dP, bf ? (T*)h->dPt : (T*)nullptr, (long long)Bpad * h->D / 4,
                                                                                h->ls());
  HIP_CHECK(hipGetLastError());
  {
    GemmParams p{};   // G[Wenc][m][n] += sum_k x[k][m] dP[k][n]: both operands K-major
    p.A = h->Xt; p.lda = h->Q;
    p.B = h->dPt; p.ldb = h->D;
    p.C = h->G; p.ldc = h->D; p.c_f32 = 1;
    p.M = h->Q; p.N = h->D; p.K = Bpad; p.epi = EPI_ATOMIC; p.alpha = 1.f; p.splitk = 1;
    SEARCH_RC(search_ordered_gemm<T>(h, p, true, true));
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
    SEARCH_RC(search_upload_x<bf16>(h, x, B, Bpad));
    SEARCH_RC(search_scores<bf16>(h, B, Bpad, true, grads, nullptr));
    if (grads) SEARCH_RC(search_backward<bf16>(h, B, Bpad));
  } else {
    SEARCH_RC(search_upload_x<float>(h, x, B, Bpad));
    SEARCH_RC(search_scores<float>(h, B, Bpad, true, grads, nullptr));
    if (grads) SEARCH_RC(search_backward<float>(h, B, Bpad));
  }
  float l = 0.f;
  HIP_CHECK(hipMemcpyAsync(&l, h->loss, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  h->last_B = B; h->last_grads = grads;
  if (loss_out) *loss_out = l;
  if (wsum_out) *wsum_out = (float)W;
  return RSYS_OK;
}

// name -> (offset, size) in the flat buffers
static int search_tensor(SearchModel* h, const char* name, long long* off, long long* size) {
  ARG_CHECK(name, "rsys_search: null name");
  if (strcmp(name, "encoder.weight") == 0) { *off = 0; *size = (long long)h->Q * h->D; return RSYS_OK; }
  if (strcmp(name, "logit_scale") == 0) { *off = (long long)h->Q * h->D; *size = 1; return RSYS_OK; }
  set_error(std::string("rsys_search: unknown parameter '") + name + "' (trainable: encoder.weight, logit_scale; the frozen table goes "
            "through rsys_search_features_set)");
  return RSYS_ERR_ARG;
}

static int search_param_io(SearchModel* h, const char* name, float* out, const float* in, int64_t n, int grad) {
  long long off, size;
  SEARCH_RC(search_tensor(h, name, &off, &size));
  ARG_CHECK(n == size, "rsys_search: element count does not match the parameter's");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  float* base = grad ? h->G : h->P;
  if (out) HIP_CHECK(hipMemcpy(out, base + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (in) {
    HIP_CHECK(hipMemcpy(base + off, in, (size_t)n * 4, hipMemcpyHostToDevice));
    if (h->bf16_mode()) SEARCH_RC(launch_cast<bf16>(h->P, h->Wsh, (long long)h->Q * h->D, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  return RSYS_OK;
}

static int search_adamw_step(SearchModel* h, float lr, float clip, float* norm_out, int32_t* skipped_out) {
  if (!h->has_adam) { set_error("rsys_search_adamw_step: no optimizer (rsys_search_adamw_create)"); return RSYS_ERR_STATE; }
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  SEARCH_RC(launch_sumsq(h->G, h->nflat, h->sumsq, h->sq_part, s, true));
  float ss = 0.f;
  HIP_CHECK(hipMemcpyAsync(&ss, h->sumsq, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  const float norm = sqrtf(ss);
  const bool skip = !std::isfinite(norm);
  if (norm_out) *norm_out = norm;
  if (skipped_out) *skipped_out = skip ? 1 : 0;
  if (skip) {   // GradScaler: no update and no step count; the gradient is cleared as the next zero_grad would
    HIP_CHECK(hipMemsetAsync(h->G, 0, (size_t)h->nflat * 4, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return RSYS_OK;
  }
  ++h->adam_step;
  const long long nd = (long long)h->Q * h->D;
  if (h->bf16_mode())
    SEARCH_RC(launch_adamw<bf16>(h->P, h->G, h->M1, h->M2, h->Wsh, nd, h->nflat, lr, h->b1, h->b2, h->eps, h->wd, h->adam_step, h->sumsq, 1.f,
                                 clip, 1, s));
  else
    SEARCH_RC(launch_adamw<float>(h->P, h->G, h->M1, h->M2, (float*)nullptr, nd, h->nflat, lr, h->b1, h->b2, h->eps, h->wd, h->adam_step,
                                  h->sumsq, 1.f, clip, 1, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

static int search_adamw_state_io(SearchModel* h, const char* name, float* m_out, float* v_out, const float* m_in, const float* v_in, int64_t n) {
  if (!h->has_adam) { set_error("rsys_search_adamw_state: no optimizer (rsys_search_adamw_create)"); return RSYS_ERR_STATE; }
  long long off, size;
  SEARCH_RC(search_tensor(h, name, &off, &size));
  ARG_CHECK(n == size, "rsys_search_adamw_state: element count does not match the parameter's");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  if (m_out) HIP_CHECK(hipMemcpy(m_out, h->M1 + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (v_out) HIP_CHECK(hipMemcpy(v_out, h->M2 + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (m_in) HIP_CHECK(hipMemcpy(h->M1 + off, m_in, (size_t)n * 4, hipMemcpyHostToDevice));
  if (v_in) HIP_CHECK(hipMemcpy(h->M2 + off, v_in, (size_t)n * 4, hipMemcpyHostToDevice));
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
    SEARCH_RC(launch_gemm<float>(p, false, false, false, false, s));
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
  auto align = [](size_t b) { return (b + 255) / 256 * 256; };
  const size_t ws_b = align(topk_rows_ws_bytes(nq, h->V, k)), ids_b = align((size_t)nq * k * 4), vals_b = ids_b, cnt_b = align((size_t)nq * 4);
  const size_t need = ws_b + ids_b + vals_b + cnt_b;
  if (h->tws_bytes < need) {
    HIP_CHECK(hipStreamSynchronize(s));
    if (h->tws) HIP_CHECK(hipFree(h->tws));
    h->tws = nullptr; h->tws_bytes = 0;
    HIP_CHECK(hipMalloc(&h->tws, need));
    h->tws_bytes = need;
  }
  char* base = (char*)h->tws;
  int* ids = (int*)(base + ws_b); float* vals = (float*)(base + ws_b + ids_b); int* cnt = (int*)(base + ws_b + ids_b + vals_b);
  if (h->bf16_mode()) {
    SEARCH_RC(search_upload_x<bf16>(h, x, nq, Bpad));
    SEARCH_RC(search_scores<bf16>(h, nq, Bpad, false, false, nullptr));
  } else {
    SEARCH_RC(search_upload_x<float>(h, x, nq, Bpad));
    SEARCH_RC(search_scores<float>(h, nq, Bpad, false, false, nullptr));
  }
  search_logp_kernel<<<dim3((h->V + 255) / 256, nq), 256, 0, s>>>(h->z, h->Vpad, h->V, h->lse, h->ls());
  HIP_CHECK(hipGetLastError());
  SEARCH_RC(topk_rows(h->z, h->Vpad, nq, h->V, k, base, ids, vals, cnt, s));
  HIP_CHECK(hipMemcpyAsync(ids_out, ids, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(logp_out, vals, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  h->last_B = nq; h->last_grads = false;
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
  if (strcmp(name, "dP") == 0) {
    ARG_CHECK(h->last_grads, "rsys_search_debug_get: the last call ran no backward");
    ARG_CHECK(n == (long long)h->last_B * h->D, "rsys_search_debug_get: dP takes B * D floats of the last call");
    HIP_CHECK(hipMemcpy(out, h->dP, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RSYS_OK;
  }
  set_error(std::string("rsys_search_debug_get: unknown name '") + name + "' (lse, dP)");
  return RSYS_ERR_ARG;
}

int search_features_from_device(void* hv, const float* rows, int64_t V, int64_t D, int device) {
  ARG_CHECK(hv, "null handle");
  SearchModel* h = (SearchModel*)hv;
  ARG_CHECK(V == h->V, "rsys_search_features_from_model: the medium's item count must be the handle's V_m");
  ARG_CHECK(D == h->D, "rsys_search_features_from_model: the model's embed_dim must be the handle's D");
  ARG_CHECK(device == h->device, "rsys_search_features_from_model: the model and the handle must be on one device");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  HIP_CHECK(hipMemcpyAsync(h->feat, rows, (size_t)V * D * 4, hipMemcpyDeviceToDevice, h->stream));
  return search_features_ready(h);
}

}  // namespace rsys

using namespace rsys;

#define SEARCH_HANDLE(hv)                                                       \
  SearchModel* h = (SearchModel*)(hv);                                          \
  do {                                                                          \
    if (h == nullptr) { set_error("null handle"); return RSYS_ERR_ARG; }        \
  } while (0)

extern "C" {

int32_t rsys_search_create(int64_t V, int32_t D, int32_t Q, int32_t dtype, int32_t max_batch, int32_t device, void** out) {
  return search_create(V, D, Q, dtype, max_batch, device, (SearchModel**)out);
}
int32_t rsys_search_destroy(void* hv) { search_free((SearchModel*)hv); return RSYS_OK; }
int32_t rsys_search_param_get(void* hv, const char* name, float* out, int64_t n) {
  SEARCH_HANDLE(hv); ARG_CHECK(out, "rsys_search_param_get: null output"); return search_param_io(h, name, out, nullptr, n, 0);
}
int32_t rsys_search_param_set(void* hv, const char* name, const float* in, int64_t n) {
  SEARCH_HANDLE(hv); ARG_CHECK(in, "rsys_search_param_set: null input"); return search_param_io(h, name, nullptr, in, n, 0);
}
int32_t rsys_search_grad_get(void* hv, const char* name, float* out, int64_t n) {
  SEARCH_HANDLE(hv); ARG_CHECK(out, "rsys_search_grad_get: null output"); return search_param_io(h, name, out, nullptr, n, 1);
}
int32_t rsys_search_zero_grad(void* hv) {
  SEARCH_HANDLE(hv);
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipMemsetAsync(h->G, 0, (size_t)h->nflat * 4, h->stream));
  return RSYS_OK;
}
int32_t rsys_search_features_set(void* hv, const float* features, int64_t V, int64_t D) {
  SEARCH_HANDLE(hv);
  ARG_CHECK(features, "rsys_search_features_set: null table");
  ARG_CHECK(V == h->V, "rsys_search_features_set: V must be the handle's V_m");
  ARG_CHECK(D == h->D, "rsys_search_features_set: D must be the handle's D");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  HIP_CHECK(hipMemcpy(h->feat, features, (size_t)V * D * 4, hipMemcpyHostToDevice));
  return search_features_ready(h);
}
int32_t rsys_search_forward_backward(void* hv, const float* x, const int32_t* labels, const float* weights, int32_t B, int32_t evaluate,
                                     float* loss_out, float* weight_sum_out) {
  SEARCH_HANDLE(hv);
  return search_forward_backward(h, x, labels, weights, B, evaluate, loss_out, weight_sum_out);
}
int32_t rsys_search_adamw_create(void* hv, float beta1, float beta2, float eps, float weight_decay) {
  SEARCH_HANDLE(hv);
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
  SEARCH_HANDLE(hv);
  return search_adamw_step(h, lr, clip, norm_out, skipped_out);
}
int32_t rsys_search_adamw_state_get(void* hv, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step) {
  SEARCH_HANDLE(hv);
  SEARCH_RC(search_adamw_state_io(h, name, exp_avg, exp_avg_sq, nullptr, nullptr, n));
  if (step) *step = h->adam_step;
  return RSYS_OK;
}
int32_t rsys_search_adamw_state_set(void* hv, const char* name, const float* exp_avg, const float* exp_avg_sq, int64_t n, int32_t step) {
  SEARCH_HANDLE(hv);
  ARG_CHECK(exp_avg && exp_avg_sq, "rsys_search_adamw_state_set: null input");
  ARG_CHECK(step >= 0, "rsys_search_adamw_state_set: step >= 0");
  SEARCH_RC(search_adamw_state_io(h, name, nullptr, nullptr, exp_avg, exp_avg_sq, n));
  h->adam_step = step;
  return RSYS_OK;
}
int32_t rsys_search_export(void* hv, float* out) { SEARCH_HANDLE(hv); return search_export(h, out); }
int32_t rsys_search_topk(void* hv, const float* x, int32_t n_queries, int32_t k, int32_t* ids_out, float* logp_out) {
  SEARCH_HANDLE(hv);
  return search_topk(h, x, n_queries, k, ids_out, logp_out);
}
int32_t rsys_search_debug_get(void* hv, const char* name, float* out, int64_t n) { SEARCH_HANDLE(hv); return search_debug_get(h, name, out, n); }

}  // extern "C"
