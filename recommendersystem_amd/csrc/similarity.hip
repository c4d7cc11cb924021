// Item-similarity LambdaRank model on the device (Training/item_similarity/pairwise_ltr.py with --features transformer / content:
// `LTRModel.embed`, `process_batch`, `lambdarank_loss`, `ndcg`, the AdamW step of `train_epoch`, `generate_embeddings` and the scoring
// and selection of `load_hard_negatives`).  A handle of its own (rsys_sim_*), independent of rsys_model, on the core of encoder_handle.hpp
// (parameters, AdamW, the feature table, the ordered split-K product).  The pipeline:
//   gather     X[r] = T(dropout(f[id_r])): in training one row per (query, slot) for the source copy and one for the target, every row
//              with its own mask (launch_dropout's counter RNG keyed on (seed, step, row, column)); in evaluation one row per source
//   encoder    Y = X W^T through launch_gemm (gemm_route picks the kernel); bf16 mode: bf16 operands, fp32 accumulation, bf16 output
//   pair       x = <normalize(Y_src), normalize(Y_tgt)> * exp(logit_scale) in fp32, one wave per pair
//   rank       per list one workgroup: bitonic sort of (score key, slot) in LDS -> 1-based ranks, ties by slot
//   lambda     per list a workgroup per 256 slots: every slot sums its own side of all of its pairs (no atomics), loss partials per block
//   backward   dY of both rows of a pair (one wave), dW += dY^T X (K-major split-K summed in split order), d logit_scale = sum dL/dx * x
//              in one workgroup
//   export     the encoder in fp32 over every id, normalised; held on the device (fp32 + bf16 copy) for the hard negatives
//   negatives  bf16 scores of the sources against the export (output rounded to bf16), split / self / positive masks, the top-k
//              selection of retrieve.hip, the stable -inf fill
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

constexpr int SIM_MAXN = 2048;            // slots per list: the rank sort holds 2048 (key, slot) pairs in LDS
constexpr int SIM_MAXQ = 4096;
constexpr int SIM_PAIR_WAVES = 4;         // pairs per workgroup of the pair kernels (one wave each)
constexpr int SIM_LT = 256;               // slots per workgroup of the pair-loss kernel
constexpr int SIM_EXPORT_ROWS = 2048;     // ids per chunk of the export
constexpr int SIM_HN_CHUNK = 256;         // sources per hard-negative score GEMM
constexpr unsigned SIM_EXPORT_STREAM = 0xffffffffu;   // RNG stream of the train-mode export's dropout

__device__ __forceinline__ void store4(float* p, const float v[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store4(bf16* p, const float v[4]) {
  bf16x4 t; t[0] = (bf16)v[0]; t[1] = (bf16)v[1]; t[2] = (bf16)v[2]; t[3] = (bf16)v[3];
  *(bf16x4*)p = t;
}

// X[r][c] = T(f[rowid[r]][c] * keep / (1 - p)) for r < R, zero for R <= r < Rpad.  keep = u01 >= p from Philox(seed) at counter
// ((r0 + r) * F + c) / 4 and `stream`: launch_dropout's mask of the gathered matrix whose first row is row r0.  drop = 0: no mask.
// rowid == nullptr: row r is id r0 + r (the export).
template <typename T>
__global__ void __launch_bounds__(256) sim_gather_kernel(const float* __restrict__ f, int F, const int* __restrict__ rowid, long long R,
                                                         long long Rpad, long long r0, float p, unsigned long long seed, unsigned stream,
                                                         int drop, T* __restrict__ X) {
  const long long n4 = Rpad * F / 4;
  const Philox ph(seed);
  const float keep = 1.f / (1.f - p);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long e = 4 * i, r = e / F;
    const int c = (int)(e - r * F);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < R) {
      const long long id = rowid ? (long long)rowid[r] : r0 + r;
      const float4 s = *(const float4*)(f + id * F + c);
      v[0] = s.x; v[1] = s.y; v[2] = s.z; v[3] = s.w;
      if (drop) {
        uint32_t rr[4];
        ph.gen((unsigned long long)((r0 * F + e) >> 2), stream, rr);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = u01(rr[k]) >= p ? v[k] * keep : 0.f;
      }
    }
    store4(X + e, v);
  }
}

// keep mask of sim_gather_kernel for rows [0, R) with r0 = 0 (test hook): out[r][c] = 1 if kept
__global__ void sim_mask_kernel(int F, long long R, float p, unsigned long long seed, unsigned stream, unsigned char* out) {
  const long long n4 = R * F / 4;
  const Philox ph(seed);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    uint32_t rr[4];
    ph.gen((unsigned long long)i, stream, rr);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[4 * i + k] = u01(rr[k]) >= p ? 1 : 0;
  }
}

// rows of a bf16 table by id: out[r] = tab[ids[r]] (E % 8 == 0)
__global__ void sim_rows_kernel(const bf16* __restrict__ tab, int E, const int* __restrict__ ids, int rows, bf16* __restrict__ out) {
  const long long n8 = (long long)rows * E / 8;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    const long long e = 8 * i, r = e / E;
    const int c = (int)(e - r * E);
    *(bf16x8*)(out + e) = *(const bf16x8*)(tab + (long long)ids[r] * E + c);
  }
}

// rows of the source copy and of the target of pair (q, j): training has one source row per pair, evaluation one per query
__device__ __forceinline__ void pair_rows(long long pair, int nq, int n, int train, long long& rs, long long& rt) {
  rs = train ? pair : pair / n;
  rt = (train ? (long long)nq * n : nq) + pair;
}

// x[pair] = <u / max(|u|, 1e-12), v / max(|v|, 1e-12)> * exp(logit_scale), fp32; one wave per pair
template <typename T>
__global__ void __launch_bounds__(64 * SIM_PAIR_WAVES) sim_pair_fwd_kernel(const T* __restrict__ Y, int E, int nq, int n, int train,
                                                                          const float* __restrict__ ls, float* __restrict__ x) {
  const long long pair = (long long)blockIdx.x * SIM_PAIR_WAVES + (threadIdx.x >> 6);
  if (pair >= (long long)nq * n) return;
  long long rs, rt;
  pair_rows(pair, nq, n, train, rs, rt);
  const T* u = Y + rs * E;
  const T* v = Y + rt * E;
  float uu = 0.f, vv = 0.f, uv = 0.f;
  for (int c = lane_id(); c < E; c += 64) {
    const float a = to_f32(u[c]), b = to_f32(v[c]);
    uu += a * a; vv += b * b; uv += a * b;
  }
  uu = wave_sum(uu); vv = wave_sum(vv); uv = wave_sum(uv);
  const float nu = fmaxf(sqrtf(uu), 1e-12f), nv = fmaxf(sqrtf(vv), 1e-12f);
  if (lane_id() == 0) x[pair] = uv / (nu * nv) * expf(*ls);
}

// backward of sim_pair_fwd_kernel (training rows) for g = dL/dx: dY rows of both members (T), gx[pair] = g * x (d logit_scale share)
template <typename T>
__global__ void __launch_bounds__(64 * SIM_PAIR_WAVES) sim_pair_bwd_kernel(const T* __restrict__ Y, int E, int nq, int n,
                                                                          const float* __restrict__ ls, const float* __restrict__ dldx,
                                                                          const float* __restrict__ x, T* __restrict__ dY,
                                                                          float* __restrict__ gx) {
  const long long pair = (long long)blockIdx.x * SIM_PAIR_WAVES + (threadIdx.x >> 6);
  if (pair >= (long long)nq * n) return;
  long long rs, rt;
  pair_rows(pair, nq, n, 1, rs, rt);
  const T* u = Y + rs * E;
  const T* v = Y + rt * E;
  float uu = 0.f, vv = 0.f, uv = 0.f;
  for (int c = lane_id(); c < E; c += 64) {
    const float a = to_f32(u[c]), b = to_f32(v[c]);
    uu += a * a; vv += b * b; uv += a * b;
  }
  uu = wave_sum(uu); vv = wave_sum(vv); uv = wave_sum(uv);
  const float su = sqrtf(uu), sv = sqrtf(vv), nu = fmaxf(su, 1e-12f), nv = fmaxf(sv, 1e-12f);
  const float g = dldx[pair], gd = g * expf(*ls), dot = uv / (nu * nv);
  // a = u / nu, b = v / nv, d dot = b . da + a . db; through the normalisation du = (da - a <a, da>) / nu while |u| > 1e-12, and
  // da / 1e-12 where the clamp holds (the denominator is then a constant)
  const bool cu = su > 1e-12f, cv = sv > 1e-12f;
  T* du = dY + rs * E;
  T* dv = dY + rt * E;
  for (int c = lane_id(); c < E; c += 64) {
    const float a = to_f32(u[c]) / nu, b = to_f32(v[c]) / nv;
    du[c] = from_f32<T>(cu ? gd * (b - a * dot) / nu : gd * b / 1e-12f);
    dv[c] = from_f32<T>(cv ? gd * (a - b * dot) / nv : gd * a / 1e-12f);
  }
  if (lane_id() == 0) gx[pair] = g * x[pair];
}

// per list q: order[q][j] = 1-based position of slot j in descending value order, ties by ascending slot (-0.0 == +0.0; -inf and NaN
// last); perm[q][r] = the slot at position r + 1
__global__ void __launch_bounds__(1024) sim_rank_kernel(const float* __restrict__ val, int n, int* __restrict__ order, int* __restrict__ perm) {
  const int q = blockIdx.x;
  __shared__ unsigned long long s[SIM_MAXN];
  int N2 = 1;
  while (N2 < n) N2 <<= 1;
  const float* vq = val + (long long)q * n;
  for (int i = threadIdx.x; i < N2; i += 1024)
    s[i] = i < n ? (((unsigned long long)score_key(vq[i]) << 32) | (unsigned long long)(0xffffffffu - (unsigned)i)) : 0ull;
  __syncthreads();
  for (int size = 2; size <= N2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < N2 / 2; i += 1024) {
        const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = s[lo], b = s[hi];
        if ((a < b) == desc) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
  for (int r = threadIdx.x; r < n; r += 1024) {
    const int slot = (int)(0xffffffffu - (unsigned)s[r]);
    perm[(long long)q * n + r] = slot;
    order[(long long)q * n + slot] = r + 1;
  }
}

__device__ __forceinline__ float softplus_neg(float d) { return fmaxf(-d, 0.f) + log1pf(expf(-fabsf(d))); }   // -logsigmoid(d)
__device__ __forceinline__ float sigmoid_neg(float d) { return 1.f / (1.f + expf(d)); }                      // sigmoid(-d)

// LambdaRank of list q (pairwise_ltr.py:183-190): slot i of this workgroup sums over every j its own side of the pair:
//   y_i > y_j: loss += c softplus(-(x_i - x_j)), g -= c sigmoid(-(x_i - x_j));   y_j > y_i: g += c sigmoid(-(x_j - x_i))
// with c = |(D_i - D_j)(y_i - y_j)|, D = 1 / log2(1 + order).  dldx = g * wscale[q]; lpart[q][block] = the block's loss (unweighted).
__global__ void __launch_bounds__(SIM_LT) sim_lambda_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                            const int* __restrict__ order, int n, const float* __restrict__ wscale,
                                                            float* __restrict__ dldx, float* __restrict__ lpart) {
  const int q = blockIdx.y, i = blockIdx.x * SIM_LT + threadIdx.x;
  __shared__ float xs[SIM_MAXN], ys[SIM_MAXN], ds[SIM_MAXN];
  __shared__ float red[16];
  const long long b = (long long)q * n;
  for (int j = threadIdx.x; j < n; j += SIM_LT) {
    xs[j] = x[b + j];
    ys[j] = y[b + j];
    ds[j] = 1.f / log2f((float)(1 + order[b + j]));
  }
  __syncthreads();
  float loss = 0.f, g = 0.f;
  if (i < n) {
    const float xi = xs[i], yi = ys[i], di = ds[i];
    for (int j = 0; j < n; ++j) {
      const float yj = ys[j];
      if (yi > yj) {
        const float c = fabsf((di - ds[j]) * (yi - yj)), d = xi - xs[j];
        loss += c * softplus_neg(d);
        g -= c * sigmoid_neg(d);
      } else if (yj > yi) {
        const float c = fabsf((ds[j] - di) * (yj - yi)), d = xs[j] - xi;
        g += c * sigmoid_neg(d);
      }
    }
    dldx[b + i] = g * wscale[q];
  }
  loss = block_sum(loss, red);
  if (threadIdx.x == 0) lpart[(long long)q * gridDim.x + blockIdx.x] = loss;
}

// loss = sum_q w_q L_q / sum_q w_q: L_q = its block partials in block order, the queries in order, an fp64 accumulator
__global__ void sim_loss_kernel(const float* __restrict__ lpart, int nb, int nq, const float* __restrict__ w, double invW, float* loss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double acc = 0.0;
  for (int q = 0; q < nq; ++q) {
    float lq = 0.f;
    for (int b = 0; b < nb; ++b) lq += lpart[(long long)q * nb + b];
    acc += (double)w[q] * (double)lq;
  }
  *loss = (float)(acc * invW);
}

// *dst += sum of v[0, n): one workgroup, strided per thread, then the block's fixed tree
__global__ void __launch_bounds__(1024) sim_sum_kernel(const float* __restrict__ v, long long n, float* dst) {
  __shared__ float red[16];
  float acc = 0.f;
  for (long long i = threadIdx.x; i < n; i += 1024) acc += v[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) *dst += acc;
}

// out[q] = DCG / IDCG of list q (pairwise_ltr.py:192-208): gains y in the order of perm_x, ideal gains in the order of perm_y,
// discounts log2(r + 2)
__global__ void __launch_bounds__(256) sim_ndcg_kernel(const float* __restrict__ y, const int* __restrict__ perm_x,
                                                       const int* __restrict__ perm_y, int n, float* __restrict__ out) {
  const int q = blockIdx.x;
  __shared__ float red[16];
  const long long b = (long long)q * n;
  float dcg = 0.f, idcg = 0.f;
  for (int r = threadIdx.x; r < n; r += 256) {
    const float disc = log2f((float)r + 2.f);
    dcg += y[b + perm_x[b + r]] / disc;
    idcg += y[b + perm_y[b + r]] / disc;
  }
  dcg = block_sum(dcg, red);
  idcg = block_sum(idcg, red);
  if (threadIdx.x == 0) out[q] = dcg / idcg;
}

// out[r] = Y[r] / max(|Y[r]|, 1e-12) (F.normalize), one wave per row
__global__ void __launch_bounds__(256) sim_normalize_kernel(const float* __restrict__ Y, int E, long long rows, float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* y = Y + r * E;
  float ss = 0.f;
  for (int c = lane_id(); c < E; c += 64) ss += y[c] * y[c];
  const float nrm = fmaxf(sqrtf(wave_sum(ss)), 1e-12f);
  for (int c = lane_id(); c < E; c += 64) out[r * E + c] = y[c] / nrm;
}

// hard-negative scores of chunk row r, stored reversed: sc[r][V - 1 - i] = bf16(z[r][i]), or -inf for i == src[r] and the split's
// mask (training: testmask bit set; test: bit clear).  The selection breaks ties by ascending column, so on the reversed row the
// LARGER id wins a tie, as in np.argsort(w, kind="stable")[-n:].
__global__ void __launch_bounds__(256) sim_hn_mask_kernel(const float* __restrict__ z, long long ldz, int V, const int* __restrict__ src,
                                                          const unsigned* __restrict__ tmask, long long tmw, int split, float* __restrict__ sc) {
  const int r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  const int s = src[r];
  const unsigned bit = (tmask[(long long)s * tmw + (i >> 5)] >> (i & 31)) & 1u;
  const bool masked = i == s || (split == 0 ? bit != 0u : bit == 0u);
  sc[(long long)r * V + (V - 1 - i)] = masked ? -INFINITY : bf16_rounded(z[(long long)r * ldz + i]);
}

__global__ void sim_hn_pos_kernel(const long long* __restrict__ pos, long long n, float* sc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) sc[pos[i]] = -INFINITY;
}

// output row r: the c = counts[r] selected ids at the end in ascending (score, id) order, and before them the n - c largest
// inadmissible ids in ascending order (found by walking the reversed row from its start, i.e. from the largest id down)
__global__ void __launch_bounds__(256) sim_hn_finish_kernel(const float* __restrict__ sc, int V, const int* __restrict__ ids,
                                                            const int* __restrict__ counts, int n, int* __restrict__ out) {
  const int r = blockIdx.x, c = counts[r];
  const int* ir = ids + (long long)r * n;
  int* o = out + (long long)r * n;
  const float* sr = sc + (long long)r * V;
  for (int t = threadIdx.x; t < c; t += 256) o[n - c + t] = V - 1 - ir[c - 1 - t];
  const int need = n - c;
  __shared__ int wc[4];
  const int w = threadIdx.x >> 6, lane = lane_id();
  const unsigned long long lt = (1ull << lane) - 1ull;
  int base = 0;
  for (int j0 = 0; j0 < V && base < need; j0 += 256) {
    const int j = j0 + threadIdx.x;
    const bool masked = j < V && !(sr[j] > -INFINITY);
    const unsigned long long bl = __ballot(masked);
    if (lane == 0) wc[w] = __popcll(bl);
    __syncthreads();
    int off = base, tot = 0;
    for (int v = 0; v < 4; ++v) {
      if (v < w) off += wc[v];
      tot += wc[v];
    }
    if (masked) {
      const int f = off + __popcll(bl & lt);
      if (f < need) o[need - 1 - f] = V - 1 - j;
    }
    base += tot;
    __syncthreads();
  }
}

}  // namespace

// ------------------------------------------------------------------ the handle
struct SimModel : EncoderCore {
  int V = 0, F = 0, E = 0, maxq = 0, nmax = 0;      // features [V][F], W [E][F]
  float p = 0.f;
  long long rcap = 0;                               // rows of the per-call operands
  void *X = nullptr, *Y = nullptr, *dY = nullptr;
  int* rowid = nullptr;
  float *x = nullptr, *rel = nullptr, *dldx = nullptr, *gx = nullptr, *w = nullptr, *wscale = nullptr, *lpart = nullptr, *loss = nullptr;
  float* qout = nullptr;
  int *order = nullptr, *perm = nullptr, *order_y = nullptr, *perm_y = nullptr;
  float *Xe = nullptr, *Ye = nullptr;               // export chunk
  float* exp32 = nullptr; bf16* exp16 = nullptr; bool has_export = false;
  unsigned* tmask = nullptr; long long tmw = 0;
  DevScratch hws;                                   // hard-negative workspace
  DevScratch pws;                                   // catalogue-rank workspace (similarity_metrics.hip)
  int last_nq = 0, last_n = 0, last_drop = 0; long long last_rows = 0;
  uint64_t last_seed = 0, last_step = 0;
  int last_ksplits = 0;                             // K splits of the last call's dW product as routed, 0: it ran none
  std::vector<int> h_rowid; std::vector<float> h_wscale;   // host sources of a call's uploads, alive until its closing wait
  void free_own() override {
    hws.release(); pws.release();
    if (exp32) hipFree(exp32);
    if (exp16) hipFree(exp16);
    if (tmask) hipFree(tmask);
  }
};

static int sim_create(int64_t V, int32_t F, int32_t E, int32_t dtype, int32_t maxq, int32_t nmax, float dropout, int32_t device, void** out) {
  ARG_CHECK(out, "rsys_sim_create: null output");
  ARG_CHECK(V >= 1 && V <= (1 << 30), "rsys_sim_create: 1 <= V <= 2^30");
  ARG_CHECK(F >= 64 && F % 64 == 0 && F <= 16384, "rsys_sim_create: F must be a multiple of 64 in [64, 16384] (2048: transformer, 5120: content)");
  ARG_CHECK(E >= 64 && E % 64 == 0 && E <= 8192, "rsys_sim_create: E must be a multiple of 64 in [64, 8192]");
  ARG_CHECK(maxq >= 1 && maxq <= SIM_MAXQ, "rsys_sim_create: 1 <= max_queries <= 4096");
  ARG_CHECK(nmax >= 1 && nmax <= SIM_MAXN, "rsys_sim_create: 1 <= items_per_query <= 2048");
  ARG_CHECK(dropout >= 0.f && dropout < 1.f, "rsys_sim_create: 0 <= dropout < 1");
  ENC_RC(enc_check_device("rsys_sim", dtype, device));
  SimModel* h = new SimModel();
  h->api = "rsys_sim"; h->wname = "encoder.1.weight"; h->device = device; h->dtype = dtype;
  h->frows = h->fpad = V; h->fcols = h->wcols = F; h->wrows = E;   // (the table is not padded)
  h->has_adam = true;   // the optimizer exists from creation: AdamW(betas 0.9 / 0.999, eps 1e-8, weight decay 0.1), the core's defaults
  h->V = (int)V; h->F = F; h->E = E; h->maxq = maxq; h->nmax = nmax; h->p = dropout;
  const size_t tsz = h->bf16_mode() ? 2 : 4;
  h->rcap = ((2LL * maxq * nmax) + 255) / 256 * 256;
  const long long pairs = (long long)maxq * nmax;
  const int rc = [&]() -> int {
    ENC_RC(enc_init(h, logf(1.f / 0.07f)));   // logit_scale = log(1 / 0.07) (pairwise_ltr.py:134)
    ENC_ALLOC(h->X, (size_t)h->rcap * F * tsz); ENC_ALLOC(h->Y, (size_t)h->rcap * E * tsz); ENC_ALLOC(h->dY, (size_t)h->rcap * E * tsz);
    ENC_ALLOC(h->rowid, h->rcap * 4);
    ENC_ALLOC(h->x, pairs * 4); ENC_ALLOC(h->rel, pairs * 4); ENC_ALLOC(h->dldx, pairs * 4); ENC_ALLOC(h->gx, pairs * 4);
    ENC_ALLOC(h->w, maxq * 4); ENC_ALLOC(h->wscale, maxq * 4); ENC_ALLOC(h->qout, maxq * 4);
    ENC_ALLOC(h->lpart, (size_t)maxq * ((SIM_MAXN + SIM_LT - 1) / SIM_LT) * 4); ENC_ALLOC(h->loss, 16);
    ENC_ALLOC(h->order, pairs * 4); ENC_ALLOC(h->perm, pairs * 4); ENC_ALLOC(h->order_y, pairs * 4); ENC_ALLOC(h->perm_y, pairs * 4);
    ENC_ALLOC(h->Xe, (size_t)SIM_EXPORT_ROWS * F * 4); ENC_ALLOC(h->Ye, (size_t)SIM_EXPORT_ROWS * E * 4);
    return RSYS_OK;
  }();
  if (rc != RSYS_OK) { enc_free(h); return rc; }
  *out = (EncoderCore*)h;
  return RSYS_OK;
}

// the encoder on rows [0, Rpad) of X: Y = X W^T (bf16 mode: the bf16 W copy, bf16 output)
template <typename T>
static int sim_encode(SimModel* h, long long Rpad) {
  GemmParams p{};
  p.A = h->X; p.lda = h->F;
  p.B = h->bf16_mode() ? (const void*)h->Wsh : (const void*)h->P; p.ldb = h->F;
  p.C = h->Y; p.ldc = h->E; p.c_f32 = h->bf16_mode() ? 0 : 1;
  p.M = (int)Rpad; p.N = h->E; p.K = h->F; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
  return launch_gemm<T>(p, false, false, false, false, h->stream);
}

// G[W] += dY^T X over K = Rpad rows: K-major operands, the split-K partial tiles summed in split order
template <typename T>
static int sim_weight_grad(SimModel* h, long long Rpad) {
  GemmParams p{};
  p.A = h->dY; p.lda = h->E;
  p.B = h->X; p.ldb = h->F;
  p.C = h->G; p.ldc = h->F; p.c_f32 = 1;
  p.M = h->E; p.N = h->F; p.K = (int)Rpad; p.epi = EPI_ATOMIC; p.alpha = 1.f;
  p.splitk = (int)std::max<long long>(1, std::min<long long>(64, Rpad / 4096));
  return enc_ordered_gemm<T>(h, p, true, true, &h->last_ksplits);
}

static int sim_check_lists(SimModel* h, int nq, int n, const int32_t* src, const int32_t* tgt, const float* rel, const float* w) {
  ARG_CHECK(h->has_features, "rsys_sim: features are not set (rsys_sim_features_set)");
  ARG_CHECK(src && tgt && rel && w, "rsys_sim: null buffer");
  ARG_CHECK(nq >= 1 && nq <= h->maxq, "rsys_sim: 1 <= n_q <= max_queries");
  ARG_CHECK(n >= 1 && n <= h->nmax, "rsys_sim: 1 <= n <= items_per_query");
  double W = 0.0;
  for (int q = 0; q < nq; ++q) {
    ARG_CHECK(src[q] >= 0 && src[q] < h->V, "rsys_sim: source ids must be in [0, V)");
    ARG_CHECK(std::isfinite(w[q]) && w[q] >= 0.f, "rsys_sim: weights must be finite and >= 0");
    W += w[q];
  }
  ARG_CHECK(W > 0.0, "rsys_sim: the weights must not sum to 0");
  for (long long i = 0; i < (long long)nq * n; ++i) {
    ARG_CHECK(tgt[i] >= 0 && tgt[i] < h->V, "rsys_sim: target ids must be in [0, V)");
    ARG_CHECK(std::isfinite(rel[i]), "rsys_sim: relevances must be finite");
  }
  return RSYS_OK;
}

// scores x of a batch (training: every slot its own source row and dropout mask; else one source row per query, no dropout) and
// ranks; with_loss: the LambdaRank loss and dL/dx; grads: the backward into G.  The caller waits on the stream before returning.
template <typename T>
static int sim_run(SimModel* h, int nq, int n, const int32_t* src, const int32_t* tgt, const float* rel, const float* w, bool train,
                   uint64_t seed, uint64_t step, bool with_loss, bool grads) {
  hipStream_t s = h->stream;
  const long long P2 = (long long)nq * n;
  const long long R = train ? 2 * P2 : nq + P2, Rpad = (R + 255) / 256 * 256;
  std::vector<int>& rowid = h->h_rowid;
  rowid.resize(R);
  for (int q = 0; q < nq; ++q) {
    if (!train) rowid[q] = src[q];
    for (int j = 0; j < n; ++j) {
      const long long pr = (long long)q * n + j;
      if (train) rowid[pr] = src[q];
      rowid[(train ? P2 : nq) + pr] = tgt[pr];
    }
  }
  double W = 0.0;
  for (int q = 0; q < nq; ++q) W += w[q];
  std::vector<float>& wscale = h->h_wscale;
  wscale.resize(nq);
  for (int q = 0; q < nq; ++q) wscale[q] = (float)((double)w[q] / W);
  HIP_CHECK(hipMemcpyAsync(h->rowid, rowid.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(h->rel, rel, (size_t)P2 * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(h->w, w, (size_t)nq * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(h->wscale, wscale.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
  const int drop = train && h->p > 0.f ? 1 : 0;
  sim_gather_kernel<T><<<grid_for(Rpad * h->F / 4), 256, 0, s>>>(h->feat, h->F, h->rowid, R, Rpad, 0, h->p, seed, (unsigned)step, drop,
                                                                  (T*)h->X);
  HIP_CHECK(hipGetLastError());
  ENC_RC(sim_encode<T>(h, Rpad));
  const float* ls = h->ls();
  const unsigned pgrid = (unsigned)((P2 + SIM_PAIR_WAVES - 1) / SIM_PAIR_WAVES);
  sim_pair_fwd_kernel<T><<<pgrid, 64 * SIM_PAIR_WAVES, 0, s>>>((const T*)h->Y, h->E, nq, n, train ? 1 : 0, ls, h->x);
  HIP_CHECK(hipGetLastError());
  sim_rank_kernel<<<nq, 1024, 0, s>>>(h->x, n, h->order, h->perm);
  HIP_CHECK(hipGetLastError());
  h->last_nq = nq; h->last_n = n; h->last_drop = drop; h->last_rows = R;
  h->last_seed = seed; h->last_step = step; h->last_ksplits = 0;
  if (!with_loss) return RSYS_OK;
  const int nb = (n + SIM_LT - 1) / SIM_LT;
  sim_lambda_kernel<<<dim3(nb, nq), SIM_LT, 0, s>>>(h->x, h->rel, h->order, n, h->wscale, h->dldx, h->lpart);
  HIP_CHECK(hipGetLastError());
  sim_loss_kernel<<<1, 64, 0, s>>>(h->lpart, nb, nq, h->w, 1.0 / W, h->loss);
  HIP_CHECK(hipGetLastError());
  if (grads) {
    T* dY = (T*)h->dY;
    if (Rpad > R) HIP_CHECK(hipMemsetAsync(dY + R * h->E, 0, (size_t)(Rpad - R) * h->E * sizeof(T), s));
    sim_pair_bwd_kernel<T><<<pgrid, 64 * SIM_PAIR_WAVES, 0, s>>>((const T*)h->Y, h->E, nq, n, ls, h->dldx, h->x, dY, h->gx);
    HIP_CHECK(hipGetLastError());
    ENC_RC(sim_weight_grad<T>(h, Rpad));
    sim_sum_kernel<<<1, 1024, 0, s>>>(h->gx, P2, h->G + h->nw());
    HIP_CHECK(hipGetLastError());
  }
  return RSYS_OK;
}

static int sim_forward_backward(SimModel* h, int nq, int n, const int32_t* src, const int32_t* tgt, const float* rel, const float* w,
                                int evaluate, uint64_t seed, uint64_t step, float* loss_out) {
  ENC_RC(sim_check_lists(h, nq, n, src, tgt, rel, w));
  HIP_CHECK(hipSetDevice(h->device));
  const bool train = evaluate == 0;
  ENC_RC(h->bf16_mode() ? sim_run<bf16>(h, nq, n, src, tgt, rel, w, train, seed, step, true, train)
                        : sim_run<float>(h, nq, n, src, tgt, rel, w, train, seed, step, true, train));
  float l = 0.f;
  HIP_CHECK(hipMemcpyAsync(&l, h->loss, 4, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  if (loss_out) *loss_out = l;
  return RSYS_OK;
}

static int sim_ndcg(SimModel* h, int nq, int n, const int32_t* src, const int32_t* tgt, const float* rel, const float* w, double* out) {
  ARG_CHECK(out, "rsys_sim_ndcg: null output");
  ENC_RC(sim_check_lists(h, nq, n, src, tgt, rel, w));
  HIP_CHECK(hipSetDevice(h->device));
  ENC_RC(h->bf16_mode() ? sim_run<bf16>(h, nq, n, src, tgt, rel, w, false, 0, 0, false, false)
                        : sim_run<float>(h, nq, n, src, tgt, rel, w, false, 0, 0, false, false));
  hipStream_t s = h->stream;
  sim_rank_kernel<<<nq, 1024, 0, s>>>(h->rel, n, h->order_y, h->perm_y);
  HIP_CHECK(hipGetLastError());
  sim_ndcg_kernel<<<nq, 256, 0, s>>>(h->rel, h->perm, h->perm_y, n, h->qout);
  HIP_CHECK(hipGetLastError());
  std::vector<float> nd(nq);
  HIP_CHECK(hipMemcpyAsync(nd.data(), h->qout, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  double a = 0.0, b = 0.0;
  for (int q = 0; q < nq; ++q) { a += (double)w[q] * (double)nd[q]; b += (double)w[q]; }
  out[0] = a; out[1] = b;
  return RSYS_OK;
}

static int sim_export_alloc(SimModel* h) {
  if (h->exp32) return RSYS_OK;
  HIP_CHECK(hipMalloc((void**)&h->exp32, (size_t)h->V * h->E * 4));
  HIP_CHECK(hipMalloc((void**)&h->exp16, (size_t)h->V * h->E * 2));
  return RSYS_OK;
}

static int sim_embed_all(SimModel* h, int train_mode, uint64_t seed, float* out) {
  ARG_CHECK(h->has_features, "rsys_sim_embed_all: features are not set (rsys_sim_features_set)");
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  ENC_RC(sim_export_alloc(h));
  const int drop = train_mode && h->p > 0.f ? 1 : 0;
  for (long long r0 = 0; r0 < h->V; r0 += SIM_EXPORT_ROWS) {
    const int rows = (int)std::min<long long>(SIM_EXPORT_ROWS, h->V - r0);
    sim_gather_kernel<float><<<grid_for((long long)rows * h->F / 4), 256, 0, s>>>(h->feat, h->F, nullptr, rows, rows, r0, h->p, seed,
                                                                                   SIM_EXPORT_STREAM, drop, h->Xe);
    HIP_CHECK(hipGetLastError());
    GemmParams p{};
    p.A = h->Xe; p.lda = h->F; p.B = h->P; p.ldb = h->F; p.C = h->Ye; p.ldc = h->E; p.c_f32 = 1;
    p.M = rows; p.N = h->E; p.K = h->F; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
    ENC_RC(launch_gemm<float>(p, false, false, false, false, s));
    sim_normalize_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, s>>>(h->Ye, h->E, rows, h->exp32 + r0 * h->E);
    HIP_CHECK(hipGetLastError());
  }
  ENC_RC(launch_cast<bf16>(h->exp32, h->exp16, (long long)h->V * h->E, s));
  h->has_export = true;
  if (out) HIP_CHECK(hipMemcpyAsync(out, h->exp32, (size_t)h->V * h->E * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

static int sim_export_set(SimModel* h, const float* emb) {
  ARG_CHECK(emb, "rsys_sim_export_set: null table");
  HIP_CHECK(hipSetDevice(h->device));
  ENC_RC(sim_export_alloc(h));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  HIP_CHECK(hipMemcpy(h->exp32, emb, (size_t)h->V * h->E * 4, hipMemcpyHostToDevice));
  ENC_RC(launch_cast<bf16>(h->exp32, h->exp16, (long long)h->V * h->E, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  h->has_export = true;
  return RSYS_OK;
}

static int sim_testmask_set(SimModel* h, const int32_t* bits) {
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  h->tmw = (h->V + 31) / 32;
  if (!bits) {
    if (h->tmask) HIP_CHECK(hipFree(h->tmask));
    h->tmask = nullptr;
    return RSYS_OK;
  }
  if (!h->tmask) HIP_CHECK(hipMalloc((void**)&h->tmask, (size_t)h->V * h->tmw * 4));
  HIP_CHECK(hipMemcpy(h->tmask, bits, (size_t)h->V * h->tmw * 4, hipMemcpyHostToDevice));
  return RSYS_OK;
}

static int sim_hard_negatives(SimModel* h, int split, int n_src, const int32_t* sources, const int64_t* pos_off, const int32_t* pos_ids,
                              int n, int32_t* ids_out) {
  ARG_CHECK(split == 0 || split == 1, "rsys_sim_hard_negatives: split must be 0 (training) or 1 (test)");
  ARG_CHECK(h->tmask, "rsys_sim_hard_negatives: no testmask (rsys_sim_testmask_set)");
  ARG_CHECK(h->has_export, "rsys_sim_hard_negatives: no export (rsys_sim_embed_all or rsys_sim_export_set)");
  ARG_CHECK(sources && ids_out, "rsys_sim_hard_negatives: null buffer");
  ARG_CHECK(n_src >= 1, "rsys_sim_hard_negatives: n_src >= 1");
  ARG_CHECK(n >= 1 && n <= h->nmax && n <= h->V, "rsys_sim_hard_negatives: 1 <= n <= min(items_per_query, V)");
  ARG_CHECK((pos_off == nullptr) == (pos_ids == nullptr), "rsys_sim_hard_negatives: pos_offsets and pos_ids are both given or both NULL");
  for (int i = 0; i < n_src; ++i) ARG_CHECK(sources[i] >= 0 && sources[i] < h->V, "rsys_sim_hard_negatives: source ids must be in [0, V)");
  if (pos_off) {
    ARG_CHECK(pos_off[0] == 0, "rsys_sim_hard_negatives: pos_offsets[0] must be 0");
    for (int i = 0; i < n_src; ++i) {
      ARG_CHECK(pos_off[i + 1] >= pos_off[i], "rsys_sim_hard_negatives: pos_offsets must be non-decreasing");
      for (int64_t j = pos_off[i]; j < pos_off[i + 1]; ++j)
        ARG_CHECK(pos_ids[j] >= 0 && pos_ids[j] < h->V, "rsys_sim_hard_negatives: positive ids must be in [0, V)");
    }
  }
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const int V = h->V, E = h->E, C = std::min(n_src, SIM_HN_CHUNK);
  const long long ldz = (V + 7) / 8 * 8;
  long long max_pos = 0;
  if (pos_off)
    for (int c0 = 0; c0 < n_src; c0 += SIM_HN_CHUNK)
      max_pos = std::max<long long>(max_pos, pos_off[std::min(n_src, c0 + SIM_HN_CHUNK)] - pos_off[c0]);
  bf16* A; float *z, *sc, *tvals; void* tws; int *tids, *cnt, *out, *dsrc; long long* dpos;
  ENC_RC(carve_into(h->hws, s, [&](Carve& c) {
    A = c.take<bf16>((size_t)C * E);
    z = c.take<float>((size_t)C * ldz);
    sc = c.take<float>((size_t)C * V);
    tws = c.take<char>(topk_rows_ws_bytes(C, V, n));
    tids = c.take<int>((size_t)C * n);
    tvals = c.take<float>((size_t)C * n);
    cnt = c.take<int>(C);
    out = c.take<int>((size_t)C * n);
    dsrc = c.take<int>(C);
    dpos = c.take<long long>(max_pos);
  }));
  std::vector<long long> hpos;
  for (int c0 = 0; c0 < n_src; c0 += SIM_HN_CHUNK) {
    const int nc = std::min(SIM_HN_CHUNK, n_src - c0);
    HIP_CHECK(hipMemcpyAsync(dsrc, sources + c0, (size_t)nc * 4, hipMemcpyHostToDevice, s));
    sim_rows_kernel<<<grid_for((long long)nc * E / 8), 256, 0, s>>>(h->exp16, E, dsrc, nc, A);
    HIP_CHECK(hipGetLastError());
    GemmParams p{};
    p.A = A; p.lda = E; p.B = h->exp16; p.ldb = E; p.C = z; p.ldc = ldz; p.c_f32 = 1;
    p.M = nc; p.N = V; p.K = E; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
    ENC_RC(launch_gemm<bf16>(p, false, false, false, false, s));
    sim_hn_mask_kernel<<<dim3((V + 255) / 256, nc), 256, 0, s>>>(z, ldz, V, dsrc, h->tmask, h->tmw, split, sc);
    HIP_CHECK(hipGetLastError());
    hpos.clear();
    if (pos_off)
      for (int r = 0; r < nc; ++r)
        for (int64_t j = pos_off[c0 + r]; j < pos_off[c0 + r + 1]; ++j) hpos.push_back((long long)r * V + (V - 1 - pos_ids[j]));
    if (!hpos.empty()) {
      HIP_CHECK(hipMemcpyAsync(dpos, hpos.data(), hpos.size() * 8, hipMemcpyHostToDevice, s));
      sim_hn_pos_kernel<<<grid_for((long long)hpos.size(), 256, 1LL << 30), 256, 0, s>>>(dpos, (long long)hpos.size(), sc);
      HIP_CHECK(hipGetLastError());
    }
    ENC_RC(topk_rows(sc, V, nc, V, n, tws, tids, tvals, cnt, s));
    sim_hn_finish_kernel<<<nc, 256, 0, s>>>(sc, V, tids, cnt, n, out);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(ids_out + (long long)c0 * n, out, (size_t)nc * n * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));   // (hpos and the source slice are refilled for the next chunk)
  }
  return RSYS_OK;
}

// the ranks / masked score rows of similarity_metrics.hip over the held export and test mask; no model state changes
static int sim_pair_ranks(SimModel* h, int32_t n_src, const int32_t* sources, const int64_t* off, const int32_t* tids, int32_t* ranks_out) {
  ARG_CHECK(h->tmask, "rsys_sim_pair_ranks: no testmask (rsys_sim_testmask_set)");
  ARG_CHECK(h->has_export, "rsys_sim_pair_ranks: no export (rsys_sim_embed_all or rsys_sim_export_set)");
  HIP_CHECK(hipSetDevice(h->device));
  return pair_ranks_run(h->exp32, h->V, h->E, h->tmask, h->tmw, n_src, sources, off, tids, ranks_out, &h->pws, h->stream);
}

static int sim_pair_scores(SimModel* h, int32_t n_src, const int32_t* sources, float* out) {
  ARG_CHECK(h->tmask, "rsys_sim_pair_scores: no testmask (rsys_sim_testmask_set)");
  ARG_CHECK(h->has_export, "rsys_sim_pair_scores: no export (rsys_sim_embed_all or rsys_sim_export_set)");
  HIP_CHECK(hipSetDevice(h->device));
  return pair_scores_run(h->exp32, h->V, h->E, h->tmask, h->tmw, n_src, sources, out, &h->pws, h->stream);
}

static int sim_debug_get(SimModel* h, const char* name, void* out, int64_t n) {
  ARG_CHECK(name && out, "rsys_sim_debug_get: null argument");
  ARG_CHECK(h->last_nq > 0, "rsys_sim_debug_get: no forward yet");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  const long long P2 = (long long)h->last_nq * h->last_n;
  if (strcmp(name, "splits") == 0) {
    ARG_CHECK(n == 1, "rsys_sim_debug_get: splits takes 1 int");
    *(int32_t*)out = h->last_ksplits;
    return RSYS_OK;
  }
  const bool ranks = strcmp(name, "ranks") == 0, scores = strcmp(name, "scores") == 0;
  if (ranks || scores || strcmp(name, "dldx") == 0) {
    ARG_CHECK(n == P2, "rsys_sim_debug_get: n must be n_q * n of the last call");
    const void* src = ranks ? (const void*)h->order : scores ? (const void*)h->x : (const void*)h->dldx;
    HIP_CHECK(hipMemcpy(out, src, (size_t)n * 4, hipMemcpyDeviceToHost));
    return RSYS_OK;
  }
  if (strcmp(name, "dropout_mask") == 0) {
    const long long cnt = h->last_rows * h->F;
    ARG_CHECK(n == cnt, "rsys_sim_debug_get: dropout_mask takes rows * F bytes of the last call");
    ARG_CHECK(cnt <= (1LL << 28), "rsys_sim_debug_get: dropout_mask is for small calls (<= 2^28 entries)");
    unsigned char* d = nullptr;
    HIP_CHECK(hipMalloc((void**)&d, (size_t)cnt));
    hipError_t e = hipSuccess;
    if (h->last_drop) {
      sim_mask_kernel<<<grid_for(cnt / 4), 256, 0, h->stream>>>(h->F, h->last_rows, h->p, h->last_seed, (unsigned)h->last_step, d);
      e = hipGetLastError();
    } else {
      e = hipMemsetAsync(d, 1, (size_t)cnt, h->stream);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, (size_t)cnt, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    hipFree(d);
    if (e != hipSuccess) { set_error(std::string("rsys_sim_debug_get: ") + hipGetErrorString(e)); return RSYS_ERR_HIP; }
    return RSYS_OK;
  }
  set_error(std::string("rsys_sim_debug_get: unknown name '") + name + "' (ranks, scores, dldx, dropout_mask, splits)");
  return RSYS_ERR_ARG;
}

}  // namespace rsys

using namespace rsys;

extern "C" {

int32_t rsys_sim_create(int64_t V, int32_t F, int32_t E, int32_t dtype, int32_t max_queries, int32_t items_per_query, float dropout,
                        int32_t device, void** out) {
  return sim_create(V, F, E, dtype, max_queries, items_per_query, dropout, device, out);
}
int32_t rsys_sim_destroy(void* hv) { enc_free((EncoderCore*)hv); return RSYS_OK; }
int32_t rsys_sim_param_get(void* hv, const char* name, float* out, int64_t n) {
  ENC_HANDLE(SimModel, hv); ARG_CHECK(out, "rsys_sim_param_get: null output"); return enc_param_io(h, name, out, nullptr, n, 0);
}
int32_t rsys_sim_param_set(void* hv, const char* name, const float* in, int64_t n) {
  ENC_HANDLE(SimModel, hv); ARG_CHECK(in, "rsys_sim_param_set: null input"); return enc_param_io(h, name, nullptr, in, n, 0);
}
int32_t rsys_sim_grad_get(void* hv, const char* name, float* out, int64_t n) {
  ENC_HANDLE(SimModel, hv); ARG_CHECK(out, "rsys_sim_grad_get: null output"); return enc_param_io(h, name, out, nullptr, n, 1);
}
int32_t rsys_sim_zero_grad(void* hv) { ENC_HANDLE(SimModel, hv); return enc_zero_grad(h); }
int32_t rsys_sim_features_set(void* hv, const float* features, int64_t V, int64_t F) { ENC_HANDLE(SimModel, hv); return enc_features_set(h, features, V, F); }
int32_t rsys_sim_forward_backward(void* hv, int32_t n_q, int32_t n, const int32_t* source, const int32_t* target, const float* relevance,
                                  const float* weight, int32_t evaluate, uint64_t seed, uint64_t step, float* loss_out) {
  ENC_HANDLE(SimModel, hv);
  return sim_forward_backward(h, n_q, n, source, target, relevance, weight, evaluate, seed, step, loss_out);
}
int32_t rsys_sim_ndcg(void* hv, int32_t n_q, int32_t n, const int32_t* source, const int32_t* target, const float* relevance,
                      const float* weight, double out[2]) {
  ENC_HANDLE(SimModel, hv);
  return sim_ndcg(h, n_q, n, source, target, relevance, weight, out);
}
int32_t rsys_sim_adamw_step(void* hv, float lr, float clip, float* norm_out, int32_t* skipped_out) {
  ENC_HANDLE(SimModel, hv);
  return enc_adamw_step(h, lr, clip, norm_out, skipped_out);
}
int32_t rsys_sim_adamw_state_get(void* hv, const char* name, float* exp_avg, float* exp_avg_sq, int64_t n, int32_t* step) {
  ENC_HANDLE(SimModel, hv);
  ENC_RC(enc_adamw_state_io(h, name, exp_avg, exp_avg_sq, nullptr, nullptr, n));
  if (step) *step = h->adam_step;
  return RSYS_OK;
}
int32_t rsys_sim_embed_all(void* hv, int32_t train_mode, uint64_t seed, float* out) { ENC_HANDLE(SimModel, hv); return sim_embed_all(h, train_mode, seed, out); }
int32_t rsys_sim_export_set(void* hv, const float* emb) { ENC_HANDLE(SimModel, hv); return sim_export_set(h, emb); }
int32_t rsys_sim_testmask_set(void* hv, const int32_t* bits) { ENC_HANDLE(SimModel, hv); return sim_testmask_set(h, bits); }
int32_t rsys_sim_hard_negatives(void* hv, int32_t split, int32_t n_src, const int32_t* sources, const int64_t* pos_offsets,
                                const int32_t* pos_ids, int32_t n, int32_t* ids_out) {
  ENC_HANDLE(SimModel, hv);
  return sim_hard_negatives(h, split, n_src, sources, pos_offsets, pos_ids, n, ids_out);
}
int32_t rsys_sim_pair_ranks(void* hv, int32_t n_src, const int32_t* sources, const int64_t* tgt_offsets, const int32_t* tgt_ids,
                            int32_t* ranks_out) {
  ENC_HANDLE(SimModel, hv);
  return sim_pair_ranks(h, n_src, sources, tgt_offsets, tgt_ids, ranks_out);
}
int32_t rsys_sim_pair_scores(void* hv, int32_t n_src, const int32_t* sources, float* out) { ENC_HANDLE(SimModel, hv); return sim_pair_scores(h, n_src, sources, out); }
int32_t rsys_sim_debug_get(void* hv, const char* name, void* out, int64_t n) { ENC_HANDLE(SimModel, hv); return sim_debug_get(h, name, out, n); }

}  // extern "C"
