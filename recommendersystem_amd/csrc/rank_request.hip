// Ranking and diversity reranking of retrieved candidates on the device (Inference/render.jl:335-435, `ranking(state, idxs)` and
// `reranking!(state, idxs, r, partialk)`): per group (one render request) the <= 1024 candidates of its page are scored by its users'
// summed log retrieval probability plus rating blend, then picked greedily under three decaying penalties.  Only ids (and optionally
// the score row) come back.  The kernels:
//   scores     retrieve.hip's gemm_retrieve and log-sum-exp over the whole item table of the medium per user (chunks of 256 users),
//              then one pass per group: score[i] = score[i] + (lp_u[i] + r_u[i]) over the group's users in user order
//   gram       G_g = E_c^T E_c over the candidates' rows of the item-similarity table, fp32: 64 x 64 output tiles, candidate rows
//              gathered through LDS, each element one fmaf chain in column order (no split-K, no atomics; G is exactly symmetric)
//   pairs      bit row j of group g: the candidates that are stored rows of column ids[j] of "{m}.related" (one thread per row, a
//              binary search of each stored row in the host-sorted candidate ids)
//   flags      related flags of the group: OR-scatter along the columns of its users' list items (medium m, status not 3 / 5)
//   loop       one workgroup of 1024 threads per group, one candidate per lane, the three penalties in registers; per round a
//              workgroup argmax on a 64-bit key, then one Gram row and one bit row
// Exact semantics (reference: Julia, fp32; every product and sum rounded on its own, no contraction):
//   lp_u = z - lse_u + log(coef), except -inf where coef * exp(z - lse_u) is 0 in fp32 (render.jl takes log.(p) of the probability)
//   r_u = c0 * rating_mean + c1 * r_masked (r_masked alone without rating coefficients)
//   per round score = ((r - mmr) - ss) - rel; argmax = Julia's findmax under isless (-inf < ... < -0.0 < +0.0 < ... < inf < NaN, the
//   first index wins); r[best] = -inf, and a position can be picked again once fewer finite scores than rounds remain
//   ss = ss * decay, + same_series where the candidate is a stored row of column ids[best]; rel = rel * decay, + flag * related if
//   flag[best]; mmr = max(mmr * decay, G[:, best] * mmr_penalty) with Julia's max (NaN propagates, max(-0.0, +0.0) = +0.0)
#include <algorithm>
#include <cmath>
#include <numeric>

#include "model_internal.hpp"

namespace rsys {

namespace {

constexpr int RK_MAXN = 1024;      // candidates per group: one lane each in the loop's workgroup
constexpr int RK_THREADS = 256;
constexpr int RK_TILE = 64;        // Gram output tile (4 x 4 elements per thread)
constexpr int RK_KT = 16;          // Gram columns per LDS stage
constexpr int RK_MAXQ = 4096;
constexpr int ST_DELETED = 3, ST_PLANNED = 5;   // render.jl:13-23

// one group on the device
struct RankGroup {
  long long c0;          // first candidate: candidate ids, scores, picks
  long long g0;          // first element of the n x n Gram matrix (row-major)
  long long b0;          // first word of the n bit rows of w = ceil(n / 32) words
  long long f0;          // first word of the w words of related flags
  int n, k;              // candidates, rounds = min(partialk, n)
  float decay, mmr, ss, rel;
};

struct RelCsc {
  int64_t* colptr = nullptr;   // [V_m + 1], device
  int32_t* rowval = nullptr;   // [nnz], device (explicit zeros dropped at load)
  int64_t n = 0, nnz = 0;
};

__device__ __forceinline__ bool bit(const unsigned* b, long long i) { return (b[i >> 5] >> (i & 31)) & 1u; }

// Julia's isless as an unsigned order: -inf < ... < -0.0 < +0.0 < ... < inf < every NaN (all NaNs equal)
__device__ __forceinline__ unsigned isless_key(float s) {
  if (s != s) return 0xffffffffu;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Julia's max(x, y) for Float32: NaN if either is NaN, +0.0 over -0.0
__device__ __forceinline__ float jl_max(float x, float y) {
  if (x != x || y != y) return __int_as_float(0x7fc00000);
  if (x == y) return signbit(x) ? y : x;
  return x > y ? x : y;
}

// position of `id` in the n sorted ids, or -1
__device__ __forceinline__ int find_sorted(const int32_t* sorted, int n, int id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sorted[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && sorted[lo] == id ? lo : -1;
}

// sc[c0 + i] = (first ? 0 : sc[c0 + i]) + sum over the group's users of this chunk (members[range.x .. range.y), ascending user index)
// of (lp_u[i] + r_u[i]), one rounding per operation.  W (rank_score_w_kernel; rsys_query_weights_set): the term is w[u] * (lp_u[i] +
// r_u[i]), product and sum rounded on their own, a user whose weight is +-0.0 skipped; W == false (rank_score_kernel) never reads `w`.
template <bool W>
__device__ __forceinline__ void rank_score_body(const RankGroup* grp, const int32_t* cand, const float* z, long long ldz, const float* lse,
                                                const int* members, const int2* ranges, int q0, const float* rm, const int64_t* rm_off,
                                                float coef, float logc, int have_rc, float c0m, float c1, int first, float* sc,
                                                const float* w) {
  const RankGroup gd = grp[blockIdx.y];
  const int i = blockIdx.x * RK_THREADS + threadIdx.x;
  if (i >= gd.n) return;
  const int2 r = ranges[blockIdx.y];
  const int id = cand[gd.c0 + i];
  float s = first ? 0.f : sc[gd.c0 + i];
  for (int t = r.x; t < r.y; ++t) {
    const int u = members[t];
    const float d = __fsub_rn(z[(long long)(u - q0) * ldz + id], lse[u]);
    const float p = __fmul_rn(coef, expf(d));
    const float lp = p == 0.f ? -INFINITY : __fadd_rn(d, logc);
    const float x = rm[rm_off[u] + i];
    const float ru = have_rc ? __fadd_rn(c0m, __fmul_rn(c1, x)) : x;
    if constexpr (W) s = weighted_add(s, w[u], __fadd_rn(lp, ru));
    else s = __fadd_rn(s, __fadd_rn(lp, ru));
  }
  sc[gd.c0 + i] = s;
}
__global__ void __launch_bounds__(RK_THREADS) rank_score_kernel(const RankGroup* grp, const int32_t* cand, const float* z, long long ldz,
                                                                const float* lse, const int* members, const int2* ranges, int q0,
                                                                const float* rm, const int64_t* rm_off, float coef, float logc,
                                                                int have_rc, float c0m, float c1, int first, float* sc) {
  rank_score_body<false>(grp, cand, z, ldz, lse, members, ranges, q0, rm, rm_off, coef, logc, have_rc, c0m, c1, first, sc, nullptr);
}
// the weighted form: w[u] per user, indexed as lse is
__global__ void __launch_bounds__(RK_THREADS) rank_score_w_kernel(const RankGroup* grp, const int32_t* cand, const float* z, long long ldz,
                                                                  const float* lse, const int* members, const int2* ranges, int q0,
                                                                  const float* rm, const int64_t* rm_off, float coef, float logc,
                                                                  int have_rc, float c0m, float c1, int first, const float* w, float* sc) {
  rank_score_body<true>(grp, cand, z, ldz, lse, members, ranges, q0, rm, rm_off, coef, logc, have_rc, c0m, c1, first, sc, w);
}

// the text queries of a request (rsys_query_texts_set), before the users' chunks: sc[c0 + i] = +0.0, then per text of the group in text
// order (members[range.x .. range.y): rows of z / lse / w) weighted_add(s, w_t, z_t[id] - lse_t).  No coefficient and no rating term
// apply to a text; a group without texts gets +0.0, which is what chunk 0 starts from with first = 1.
__global__ void __launch_bounds__(RK_THREADS) rank_text_kernel(const RankGroup* grp, const int32_t* cand, const float* z, long long ldz,
                                                               const float* lse, const int* members, const int2* ranges, const float* w,
                                                               float* sc) {
  const RankGroup gd = grp[blockIdx.y];
  const int i = blockIdx.x * RK_THREADS + threadIdx.x;
  if (i >= gd.n) return;
  const int2 r = ranges[blockIdx.y];
  const int id = cand[gd.c0 + i];
  float s = 0.f;
  for (int t = r.x; t < r.y; ++t) {
    const int q = members[t];
    s = weighted_add(s, w[q], __fsub_rn(z[(long long)q * ldz + id], lse[q]));
  }
  sc[gd.c0 + i] = s;
}

// G_g[i][j] = sum over columns c in ascending order of E[id_i][c] * E[id_j][c] (one fmaf chain) for the 64 x 64 tile (blockIdx.y,
// blockIdx.x) of group blockIdx.z.  Both operand tiles are gathered into LDS column-major; thread (ty, tx) owns rows 4 ty.., cols 4 tx..
__global__ void __launch_bounds__(RK_THREADS) gram_kernel(const RankGroup* grp, const int32_t* cand, const float* E, int dim, float* G) {
  const RankGroup gd = grp[blockIdx.z];
  const int n = gd.n, i0 = blockIdx.y * RK_TILE, j0 = blockIdx.x * RK_TILE;
  if (i0 >= n || j0 >= n) return;
  __shared__ __attribute__((aligned(16))) float As[RK_KT][RK_TILE];
  __shared__ __attribute__((aligned(16))) float Bs[RK_KT][RK_TILE];
  const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
  const int lr = t >> 2, lc = (t & 3) * 4;   // loader: tile row lr, columns lc .. lc + 3 of the stage
  const float* ea = i0 + lr < n ? E + (long long)cand[gd.c0 + i0 + lr] * dim : nullptr;
  const float* eb = j0 + lr < n ? E + (long long)cand[gd.c0 + j0 + lr] * dim : nullptr;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  for (int k0 = 0; k0 < dim; k0 += RK_KT) {
    const bool in = k0 + lc < dim;   // (dim is a multiple of 4: a float4 is wholly in or out)
    const float4 va = ea && in ? *(const float4*)(ea + k0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 vb = eb && in ? *(const float4*)(eb + k0 + lc) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    As[lc][lr] = va.x; As[lc + 1][lr] = va.y; As[lc + 2][lr] = va.z; As[lc + 3][lr] = va.w;
    Bs[lc][lr] = vb.x; Bs[lc + 1][lr] = vb.y; Bs[lc + 2][lr] = vb.z; Bs[lc + 3][lr] = vb.w;
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < RK_KT; ++kk) {
      const float4 a = *(const float4*)&As[kk][ty * 4];
      const float4 b = *(const float4*)&Bs[kk][tx * 4];
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = fmaf(av[p], bv[q], acc[p][q]);
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + ty * 4 + p;
    if (i >= n) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx * 4 + q;
      if (j < n) G[gd.g0 + (long long)i * n + j] = acc[p][q];
    }
  }
}

// bit row j of group blockIdx.y (words zeroed before): bit i set when candidate i is a stored row of column ids[j] of `related`.  Only
// this thread writes row j.
__global__ void __launch_bounds__(RK_THREADS) pair_rows_kernel(const RankGroup* grp, const int32_t* cand, const int32_t* sorted_ids,
                                                               const int32_t* sorted_pos, const int64_t* colptr, const int32_t* rowval,
                                                               unsigned* bits) {
  const RankGroup gd = grp[blockIdx.y];
  const int j = blockIdx.x * RK_THREADS + threadIdx.x;
  if (j >= gd.n) return;
  const int w = (gd.n + 31) >> 5, col = cand[gd.c0 + j];
  unsigned* row = bits + gd.b0 + (long long)j * w;
  for (int64_t e = colptr[col]; e < colptr[col + 1]; ++e) {
    const int p = find_sorted(sorted_ids + gd.c0, gd.n, rowval[e]);
    if (p >= 0) {
      const int i = sorted_pos[gd.c0 + p];
      row[i >> 5] |= 1u << (i & 31);
    }
  }
}

// related flags: for list entry e (group ent_g[e], item ent_id[e] of medium m, status not 3 / 5) every candidate of the group that is
// a stored row of the item's column (OR: independent of order and scheduling)
__global__ void __launch_bounds__(RK_THREADS) related_flags_kernel(const RankGroup* grp, const int32_t* ent_g, const int32_t* ent_id,
                                                                   long long nent, const int32_t* sorted_ids, const int32_t* sorted_pos,
                                                                   const int64_t* colptr, const int32_t* rowval, unsigned* flags) {
  const long long e = (long long)blockIdx.x * RK_THREADS + threadIdx.x;
  if (e >= nent) return;
  const RankGroup gd = grp[ent_g[e]];
  const int col = ent_id[e];
  for (int64_t x = colptr[col]; x < colptr[col + 1]; ++x) {
    const int p = find_sorted(sorted_ids + gd.c0, gd.n, rowval[x]);
    if (p >= 0) {
      const int i = sorted_pos[gd.c0 + p];
      atomicOr(&flags[gd.f0 + (i >> 5)], 1u << (i & 31));
    }
  }
}

// the greedy loop of render.jl:420-430 for group blockIdx.x: picks[c0 + round] = the position chosen in that round
__global__ void __launch_bounds__(RK_MAXN) rerank_kernel(const RankGroup* grp, const float* r_in, const float* G, const unsigned* bits,
                                                         const unsigned* flags, int* picks) {
  const RankGroup gd = grp[blockIdx.x];
  const int n = gd.n, i = threadIdx.x, w = (n + 31) >> 5;
  const bool act = i < n;
  const unsigned* fl = flags + gd.f0;
  float r = act ? r_in[gd.c0 + i] : 0.f, mmr = 0.f, ss = 0.f, rel = 0.f;
  const float flag = act && bit(fl, i) ? 1.f : 0.f;
  __shared__ unsigned long long red[2][RK_MAXN / 64];
  for (int round = 0; round < gd.k; ++round) {
    const float s = __fsub_rn(__fsub_rn(__fsub_rn(r, mmr), ss), rel);
    unsigned long long key = act ? ((unsigned long long)isless_key(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)i) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long x = __shfl_xor(key, o, 64);
      key = x > key ? x : key;
    }
    unsigned long long* rd = red[round & 1];   // (two buffers: one barrier per round)
    if (lane_id() == 0) rd[i >> 6] = key;
    __syncthreads();
    unsigned long long best = rd[0];
#pragma unroll
    for (int v = 1; v < RK_MAXN / 64; ++v) best = rd[v] > best ? rd[v] : best;
    const int b = (int)(0xffffffffu - (unsigned)best);
    if (i == 0) picks[gd.c0 + round] = b;
    if (act) {
      if (i == b) r = -INFINITY;
      ss = __fmul_rn(ss, gd.decay);
      if (bit(bits + gd.b0 + (long long)b * w, i)) ss = __fadd_rn(ss, gd.ss);
      rel = __fmul_rn(rel, gd.decay);
      if (bit(fl, b)) rel = __fadd_rn(rel, __fmul_rn(flag, gd.rel));
      mmr = jl_max(__fmul_rn(mmr, gd.decay), __fmul_rn(G[gd.g0 + (long long)b * n + i], gd.mmr));   // (G symmetric: row b = column b)
    }
  }
}

// sorted copy of group blockIdx.x's candidate ids with their positions (what make_groups sorts on the host when the ids are there): a
// bitonic sort of (id, position) keys in LDS, one candidate per lane; the ids of a group are distinct, so the order is total
__global__ void __launch_bounds__(RK_MAXN) sort_cand_kernel(const RankGroup* grp, const int32_t* cand, int32_t* sorted_ids, int32_t* sorted_pos) {
  const RankGroup gd = grp[blockIdx.x];
  const int n = gd.n, i = threadIdx.x;
  __shared__ unsigned long long key[RK_MAXN];
  key[i] = i < n ? ((unsigned long long)(unsigned)cand[gd.c0 + i] << 32) | (unsigned)i : ~0ull;
  __syncthreads();
  for (int size = 2; size <= RK_MAXN; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (i < RK_MAXN / 2) {
        const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const unsigned long long a = key[lo], b = key[hi];
        if ((a > b) == asc) { key[lo] = b; key[hi] = a; }
      }
      __syncthreads();
    }
  }
  if (i < n) {
    sorted_ids[gd.c0 + i] = (int32_t)(key[i] >> 32);
    sorted_pos[gd.c0 + i] = (int32_t)(key[i] & 0xffffffffu);
  }
}

// the page of group blockIdx.x: the ids picked in rounds [lo[g], hi[g]) to page[off[g] ..]
__global__ void __launch_bounds__(RK_THREADS) page_gather_kernel(const RankGroup* grp, const int32_t* cand, const int* picks, const int32_t* lo,
                                                                 const int32_t* hi, const int64_t* off, int32_t* page) {
  const int g = blockIdx.x;
  const RankGroup gd = grp[g];
  for (int t = lo[g] + threadIdx.x; t < hi[g]; t += RK_THREADS) page[off[g] + t - lo[g]] = cand[gd.c0 + picks[gd.c0 + t]];
}

#define RK_LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

// host side of a request's candidates: the groups' device descriptors and sorted copies of the ids
struct Groups {
  std::vector<RankGroup> g;
  std::vector<int32_t> sorted_ids, sorted_pos;
  long long N = 0, gram = 0, bits = 0, flags = 0;
};

// ids_on_device: the ids are a retrieval result in device memory (distinct and in range by construction); sort_cand_kernel sorts them there
int make_groups(const char* who, int ng, const int64_t* cand_off, const int32_t* cand_ids, const int32_t* partialk, const float* pen, int Vm,
                Groups& G, bool ids_on_device = false) {
  ARG_CHECK(cand_off && (cand_ids || ids_on_device), std::string(who) + ": candidate offsets and ids are required");
  ARG_CHECK(cand_off[0] == 0, std::string(who) + ": cand_offsets[0] must be 0");
  G.g.resize(ng);
  for (int j = 0; j < ng; ++j) {
    const int64_t n = cand_off[j + 1] - cand_off[j];
    ARG_CHECK(n >= 1 && n <= RK_MAXN, std::string(who) + ": every group needs 1 <= n <= 1024 candidates");
    RankGroup& d = G.g[j];
    d.c0 = cand_off[j]; d.n = (int)n;
    d.g0 = G.gram; d.b0 = G.bits; d.f0 = G.flags;
    const long long w = (n + 31) / 32;
    G.gram += n * n; G.bits += n * w; G.flags += w;
    if (partialk) {
      ARG_CHECK(partialk[j] >= 1, std::string(who) + ": partialk must be >= 1");
      d.k = (int)std::min<int64_t>(partialk[j], n);
    }
    if (pen) { d.decay = pen[4 * j]; d.mmr = pen[4 * j + 1]; d.ss = pen[4 * j + 2]; d.rel = pen[4 * j + 3]; }
  }
  G.N = cand_off[ng];
  if (ids_on_device) return RSYS_OK;
  G.sorted_ids.resize((size_t)G.N); G.sorted_pos.resize((size_t)G.N);
  std::vector<int32_t> idx;
  for (int j = 0; j < ng; ++j) {
    const RankGroup& d = G.g[j];
    idx.resize(d.n);
    std::iota(idx.begin(), idx.end(), 0);
    const int32_t* c = cand_ids + d.c0;
    for (int i = 0; i < d.n; ++i) ARG_CHECK(c[i] >= 0 && c[i] < Vm, std::string(who) + ": candidate ids must be in [0, V_m)");
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { return c[a] < c[b]; });
    for (int i = 0; i < d.n; ++i) {
      G.sorted_ids[d.c0 + i] = c[idx[i]];
      G.sorted_pos[d.c0 + i] = idx[i];
      ARG_CHECK(i == 0 || c[idx[i]] != c[idx[i - 1]], std::string(who) + ": a group's candidate ids must be distinct");
    }
  }
  return RSYS_OK;
}

}  // namespace

struct RankTables {
  RelCsc related[2];
  DevScratch ws;        // the request's device workspace
};

static RankTables* rank_tables(Model* m) {
  if (!m->rank) m->rank = new RankTables();
  return m->rank;
}

void rank_free(Model* m) {
  RankTables* R = m->rank;
  if (!R) return;
  for (RelCsc& c : R->related) { dfree(c.colptr); dfree(c.rowval); }
  R->ws.release();
  delete R;
  m->rank = nullptr;
}

int model_rank_related_set(Model* m, int medium, int64_t n, const int64_t* colptr, const int32_t* rowval, const float* nzval) {
  ARG_CHECK(medium == 0 || medium == 1, "rank_related_set: medium must be 0 or 1");
  const int64_t Vm = medium == 0 ? m->V0 : m->V1;
  std::vector<int64_t> cp;
  std::vector<int32_t> rv;
  if (colptr) {
    ARG_CHECK(rowval && nzval, "rank_related_set: rowval and nzval are required with colptr");
    ARG_CHECK(n == Vm, "rank_related_set: the matrix must be V_m x V_m");
    RC(csc_nonzero_pattern("rank_related_set", "[0, V_m)", n, n, colptr, rowval, nzval, cp, rv));
  }
  HIP_CHECK(hipSetDevice(m->device));
  HIP_CHECK(hipStreamSynchronize(m->stream));
  RelCsc& c = rank_tables(m)->related[medium];
  dfree(c.colptr); dfree(c.rowval);
  c.n = c.nnz = 0;
  if (!colptr) return RSYS_OK;
  RC(upload((void**)&c.colptr, cp.data(), cp.size() * 8));
  RC(upload((void**)&c.rowval, rv.data(), rv.size() * 4));
  c.n = n; c.nnz = (int64_t)rv.size();
  return RSYS_OK;
}

// the Gram matrices of the groups into G (device), on the model's stream
static int launch_gram(Model* m, const Groups& gs, const RankGroup* d_grp, const int32_t* d_cand, const float* E, int dim, float* G) {
  int nmax = 0;
  for (const RankGroup& d : gs.g) nmax = std::max(nmax, d.n);
  const unsigned t = (unsigned)((nmax + RK_TILE - 1) / RK_TILE);
  tic(m, "rank_gram");
  gram_kernel<<<dim3(t, t, (unsigned)gs.g.size()), RK_THREADS, 0, m->stream>>>(d_grp, d_cand, E, dim, G);
  RK_LAUNCH_CHECK();
  toc(m);
  return RSYS_OK;
}

// the host plan of a checked request, as rank_request_body hands it to rank_t: the groups, every user's group and first r_masked value,
// the distinct (group, id) list entries behind the related flags, the similarity table of the reranking
struct RankPlan {
  Groups gs;
  std::vector<int32_t> ugroup, ent_g, ent_id;
  std::vector<int64_t> rm_off;
  const float* E = nullptr; int dim = 0;
};

template <typename T>
static int rank_t(Model* m, int medium, const Request& rq, const RankCands& rc, const RankPlan& pl, int32_t* ids_out, float* r_out,
                  const RankDev* dev) {
  const int ng = rq.ng;
  const int64_t nu = rq.nq, n_rm = rc.n_rm;
  const Groups& gs = pl.gs;
  const std::vector<int32_t>& ent_g = pl.ent_g;
  const std::vector<int32_t>& ent_id = pl.ent_id;
  const QueryTexts& qt = rq.qt;
  const int32_t* cand_ids = rc.cand_ids;   // (the three inputs that a RankDev replaces, below)
  const float* queries = rq.queries;
  const float* r_masked = rc.r_masked;
  const int Vm = medium == 0 ? m->V0 : m->V1;
  hipStream_t s = m->stream;
  const bool score = rc.r_in == nullptr, rerank = ids_out != nullptr || dev != nullptr;
  const bool texts = score && qt.n > 0;   // (with rc.r_in the texts are consumed and not read)
  std::vector<int32_t> tmem, trng;
  if (texts) text_plan(qt, ng, tmem, trng);
  int64_t npage = 0;
  if (dev) for (int g = 0; g < ng; ++g) npage = std::max<int64_t>(npage, dev->page_off[g] + dev->page_hi[g] - dev->page_lo[g]);
  // users of each group in user order; per chunk of RETRIEVE_CHUNK users the range of them it holds.  Only scoring reads the plan;
  // rank_request_body has checked the group ids and that no group is empty, in its own words, so group_plan's two checks cannot fail here.
  GroupPlan gp;
  if (score) RC(group_plan("rank_request", pl.ugroup.data(), nu, ng, RETRIEVE_CHUNK, gp));
  const int nchunks = gp.nchunks;
  const int64_t nent = (int64_t)ent_g.size();
  ScoreBufs<T> b(m);
  float *d_rm, *sc, *G, *d_uw; int *d_members, *picks; int2* d_ranges; int64_t* d_rmoff; RankGroup* d_grp;
  int32_t *d_cand, *d_sid, *d_spos, *d_eg, *d_eid, *d_plo, *d_phi, *d_page, *d_tmem, *d_trng; int64_t* d_poff; unsigned *bits, *flags;
  RC(carve_into(rank_tables(m)->ws, s, [&](Carve& c) {
    b.take(c, score ? nu : 0);
    d_members = c.take<int>(nu);
    d_ranges = c.take<int2>((size_t)std::max(nchunks, 1) * ng);
    d_uw = c.take<float>(score && rq.qw.user ? nu : 0);
    d_tmem = c.take<int32_t>(tmem.size());
    d_trng = c.take<int32_t>(trng.size());
    d_rm = c.take<float>(score ? n_rm : 0);
    d_rmoff = c.take<int64_t>(nu);
    d_grp = c.take<RankGroup>(ng);
    d_cand = c.take<int32_t>(gs.N);
    d_sid = c.take<int32_t>(rerank ? gs.N : 0);
    d_spos = c.take<int32_t>(rerank ? gs.N : 0);
    sc = c.take<float>(gs.N);
    G = c.take<float>(rerank ? gs.gram : 0);
    bits = c.take<unsigned>(rerank ? gs.bits : 0);
    flags = c.take<unsigned>(rerank ? gs.flags : 0);
    d_eg = c.take<int32_t>(nent);
    d_eid = c.take<int32_t>(nent);
    picks = c.take<int>(rerank ? gs.N : 0);
    d_plo = c.take<int32_t>(dev ? ng : 0);
    d_phi = c.take<int32_t>(dev ? ng : 0);
    d_poff = c.take<int64_t>(dev ? ng : 0);
    d_page = c.take<int32_t>(npage);
  }));
  // (dev: candidates, queries and r_masked are device arrays; same kernels on the same values)
  const hipMemcpyKind in_kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (dev) { cand_ids = dev->d_cand; queries = dev->d_queries; r_masked = dev->d_rm; }

  tic(m, "rank_prep");
  HIP_CHECK(hipMemcpyAsync(d_grp, gs.g.data(), (size_t)ng * sizeof(RankGroup), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_cand, cand_ids, (size_t)gs.N * 4, in_kind, s));
  if (score) {
    RC(score_upload_queries(b, queries, nu, in_kind, s));
    HIP_CHECK(hipMemcpyAsync(d_members, gp.members.data(), gp.members.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_ranges, gp.ranges.data(), gp.ranges.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    if (rq.qw.user) HIP_CHECK(hipMemcpyAsync(d_uw, rq.qw.user, (size_t)nu * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_rm, r_masked, (size_t)n_rm * 4, in_kind, s));
    HIP_CHECK(hipMemcpyAsync(d_rmoff, pl.rm_off.data(), (size_t)nu * 8, hipMemcpyHostToDevice, s));
    if (texts) {
      HIP_CHECK(hipMemcpyAsync(d_tmem, tmem.data(), tmem.size() * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_trng, trng.data(), trng.size() * 4, hipMemcpyHostToDevice, s));
    }
  } else {
    HIP_CHECK(hipMemcpyAsync(sc, rc.r_in, (size_t)gs.N * 4, hipMemcpyHostToDevice, s));
  }
  if (rerank) {
    if (dev) {
      sort_cand_kernel<<<ng, RK_MAXN, 0, s>>>(d_grp, d_cand, d_sid, d_spos);
      RK_LAUNCH_CHECK();
      HIP_CHECK(hipMemcpyAsync(d_plo, dev->page_lo, (size_t)ng * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_phi, dev->page_hi, (size_t)ng * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_poff, dev->page_off, (size_t)ng * 8, hipMemcpyHostToDevice, s));
    } else {
      HIP_CHECK(hipMemcpyAsync(d_sid, gs.sorted_ids.data(), (size_t)gs.N * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_spos, gs.sorted_pos.data(), (size_t)gs.N * 4, hipMemcpyHostToDevice, s));
    }
    if (nent) {
      HIP_CHECK(hipMemcpyAsync(d_eg, ent_g.data(), (size_t)nent * 4, hipMemcpyHostToDevice, s));
      HIP_CHECK(hipMemcpyAsync(d_eid, ent_id.data(), (size_t)nent * 4, hipMemcpyHostToDevice, s));
    }
    HIP_CHECK(hipMemsetAsync(bits, 0, (size_t)gs.bits * 4, s));
    HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)gs.flags * 4, s));
    if (dev && dev->keep_picks) HIP_CHECK(hipMemsetAsync(picks, 0xff, (size_t)gs.N * 4, s));   // (test hook: the rounds not run read -1)
  }
  toc(m);
  if (score) {
    const T* Fm;
    RC(score_table_ready<T>(m, medium, &Fm));
    const float coef = rc.retrieval_coef ? *rc.retrieval_coef : 1.f;
    const float logc = logf(coef);
    const int have_rc = rc.rating_coefs != nullptr;
    const float c0m = have_rc ? rc.rating_coefs[0] * rc.rating_mean : 0.f, c1 = have_rc ? rc.rating_coefs[1] : 0.f;
    if (texts) {   // the users' first chunk then adds to the texts' sums
      tic(m, "rank_texts");
      rank_text_kernel<<<dim3(RK_MAXN / RK_THREADS, ng), RK_THREADS, 0, s>>>(d_grp, d_cand, qt.z, qt.ldz, qt.lse, d_tmem, (const int2*)d_trng,
                                                                            qt.d_w, sc);
      RK_LAUNCH_CHECK();
      toc(m);
    }
    for (int ch = 0; ch < nchunks; ++ch) {
      const int q0 = ch * RETRIEVE_CHUNK, nc = (int)std::min<int64_t>(RETRIEVE_CHUNK, nu - q0);
      RC(retrieve_chunk_scores<T>(m, b.qt + (size_t)q0 * b.D, nc, q0, Fm, Vm, b.z, b.ldz, b.part, b.lse));
      tic(m, "rank_score");
      const dim3 grid(RK_MAXN / RK_THREADS, ng);
      const int2* rg = d_ranges + (size_t)ch * ng;
      const int first = ch == 0 && !texts;
      if (rq.qw.user)
        rank_score_w_kernel<<<grid, RK_THREADS, 0, s>>>(d_grp, d_cand, b.z, b.ldz, b.lse, d_members, rg, q0, d_rm, d_rmoff, coef, logc, have_rc,
                                                        c0m, c1, first, d_uw, sc);
      else
        rank_score_kernel<<<grid, RK_THREADS, 0, s>>>(d_grp, d_cand, b.z, b.ldz, b.lse, d_members, rg, q0, d_rm, d_rmoff, coef, logc, have_rc,
                                                      c0m, c1, first, sc);
      RK_LAUNCH_CHECK();
      toc(m);
    }
  }
  if (rerank) {
    const RelCsc& rel = m->rank->related[medium];
    RC(launch_gram(m, gs, d_grp, d_cand, pl.E, pl.dim, G));
    tic(m, "rank_pairs");
    pair_rows_kernel<<<dim3(RK_MAXN / RK_THREADS, ng), RK_THREADS, 0, s>>>(d_grp, d_cand, d_sid, d_spos, rel.colptr, rel.rowval, bits);
    RK_LAUNCH_CHECK();
    if (nent) {
      related_flags_kernel<<<(unsigned)((nent + RK_THREADS - 1) / RK_THREADS), RK_THREADS, 0, s>>>(d_grp, d_eg, d_eid, nent, d_sid, d_spos,
                                                                                                  rel.colptr, rel.rowval, flags);
      RK_LAUNCH_CHECK();
    }
    toc(m);
    tic(m, "rank_loop");
    rerank_kernel<<<ng, RK_MAXN, 0, s>>>(d_grp, sc, G, bits, flags, picks);
    RK_LAUNCH_CHECK();
    toc(m);
  }
  if (dev) {   // only the pages leave the device (and, for the test hooks, the scores and the pick order)
    page_gather_kernel<<<ng, RK_THREADS, 0, s>>>(d_grp, d_cand, picks, d_plo, d_phi, d_poff, d_page);
    RK_LAUNCH_CHECK();
    if (npage) HIP_CHECK(hipMemcpyAsync(dev->page_out, d_page, (size_t)npage * 4, hipMemcpyDeviceToHost, s));
    if (dev->keep_r) HIP_CHECK(hipMemcpyAsync(dev->keep_r, sc, (size_t)gs.N * 4, hipMemcpyDeviceToHost, s));
    if (dev->keep_picks) HIP_CHECK(hipMemcpyAsync(dev->keep_picks, picks, (size_t)gs.N * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return RSYS_OK;
  }
  std::vector<int32_t> pos(rerank ? (size_t)gs.N : 0);
  if (rerank) HIP_CHECK(hipMemcpyAsync(pos.data(), picks, (size_t)gs.N * 4, hipMemcpyDeviceToHost, s));
  if (r_out) HIP_CHECK(hipMemcpyAsync(r_out, sc, (size_t)gs.N * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (rerank)
    for (const RankGroup& d : gs.g)
      for (int i = 0; i < d.n; ++i) ids_out[d.c0 + i] = i < d.k ? cand_ids[d.c0 + pos[d.c0 + i]] : -1;
  return RSYS_OK;
}

// the one body of rsys_rank_request and of rsys_render_request's last stage (dev != nullptr: candidates, queries and r_masked on the device)
static int rank_request_body(Model* m, int medium, const Request& rq, const RankCands& rc, int32_t* ids_out, float* r_out, const RankDev* dev) {
  const int32_t ng = rq.ng;
  const int64_t nu = rq.nq;
  const HistoryList& hist = rq.hist;
  ARG_CHECK(medium == 0 || medium == 1, "rank_request: medium must be 0 or 1");
  ARG_CHECK(ids_out || r_out || dev, "rank_request: no output (ids_out and r_out are both NULL)");
  ARG_CHECK(nu >= 1 && nu <= RK_MAXQ, "rank_request: 1 <= n_users <= 4096");
  ARG_CHECK(ng >= 1 && ng <= nu, "rank_request: 1 <= n_groups <= n_users (every group needs a user)");
  ARG_CHECK(rq.group != nullptr || ng == nu, "rank_request: without `group`, n_groups must equal n_users");
  const bool score = rc.r_in == nullptr;
  if (score) {
    ARG_CHECK(!m->sharded, "rank_request: the row-sharded item table is not supported (replicated table only)");
    ARG_CHECK(dev ? (dev->d_queries && dev->d_rm) : (rq.queries && rc.r_masked), "rank_request: queries and r_masked are required unless r_in is given");
  }
  const bool rerank = ids_out != nullptr || dev != nullptr;
  if (rerank) ARG_CHECK(rc.partialk && rc.penalties, "rank_request: partialk and penalties are required with ids_out");
  const int V[2] = {m->V0, m->V1};
  const int Vm = V[medium];
  RankPlan pl;
  Groups& gs = pl.gs;
  RC(make_groups("rank_request", ng, rc.cand_off, rc.cand_ids, rerank ? rc.partialk : nullptr, rerank ? rc.penalties : nullptr, Vm, gs, dev != nullptr));
  std::vector<int32_t>& ugroup = pl.ugroup;
  ugroup.resize((size_t)nu);
  std::vector<int> members(ng, 0);
  pl.rm_off.resize((size_t)nu);
  int64_t need = 0;
  for (int64_t u = 0; u < nu; ++u) {
    ugroup[u] = rq.group ? rq.group[u] : (int32_t)u;
    ARG_CHECK(ugroup[u] >= 0 && ugroup[u] < ng, "rank_request: group ids must be in [0, n_groups)");
    ++members[ugroup[u]];
    pl.rm_off[u] = need;
    need += gs.g[ugroup[u]].n;
  }
  for (int g = 0; g < ng; ++g) ARG_CHECK(members[g] > 0, "rank_request: every group needs at least one user");
  if (score) ARG_CHECK(rc.n_rm == need, "rank_request: r_masked must hold n_g values per user of group g (n_r_masked = their sum)");
  RC(check_ragged("rank_request", hist, nu));
  RC(check_list_items("rank_request", hist, nu, V));
  // related flags: every list entry of medium m whose status is not deleted / planned (render.jl:395-408 walks the whole list, not the
  // last status per item), one entry per distinct (group, id)
  if (hist.off) {
    std::vector<std::pair<int32_t, int32_t>> ent;
    for (int64_t u = 0; u < nu; ++u)
      for (int64_t j = hist.off[u]; j < hist.off[u + 1]; ++j)
        if (hist.medium[j] == medium && hist.status[j] != ST_DELETED && hist.status[j] != ST_PLANNED) ent.emplace_back(ugroup[u], hist.ids[j]);
    std::sort(ent.begin(), ent.end());
    ent.erase(std::unique(ent.begin(), ent.end()), ent.end());
    for (const auto& e : ent) { pl.ent_g.push_back(e.first); pl.ent_id.push_back(e.second); }
  }
  if (rerank) {
    int64_t dim = 0;
    pl.E = retrieve_similarity_table(m, medium, &dim);
    pl.dim = (int)dim;
    ARG_CHECK(pl.E != nullptr, "rank_request: the item-similarity embeddings of the medium are not loaded (rsys_retrieve_similarity_set)");
    const RankTables* R = rank_tables(m);
    ARG_CHECK(R->related[medium].colptr != nullptr, "rank_request: the related table of the medium is not loaded (rsys_rank_related_set)");
  }
  HIP_CHECK(hipSetDevice(m->device));
  return m->bf16_mode ? rank_t<bf16>(m, medium, rq, rc, pl, ids_out, r_out, dev) : rank_t<float>(m, medium, rq, rc, pl, ids_out, r_out, dev);
}

int model_rank_request(Model* m, int medium, const Request& rq, const RankCands& rc, int32_t* ids_out, float* r_out) {
  return rank_request_body(m, medium, rq, rc, ids_out, r_out, nullptr);
}

int model_rank_request_dev(Model* m, int medium, const Request& rq, const RankCands& rc, const RankDev* dev) {
  ARG_CHECK(dev && dev->d_cand && dev->page_lo && dev->page_hi && dev->page_off && dev->page_out, "rank_request: null device buffers");
  return rank_request_body(m, medium, rq, rc, nullptr, nullptr, dev);
}

int model_rank_items_dev(Model* m, int medium, int32_t ng, const int64_t* cand_off, const RankDev* dev, const int32_t* partialk,
                         const float* penalties) {
  ARG_CHECK(dev && dev->d_cand && dev->page_lo && dev->page_hi && dev->page_off && dev->page_out && cand_off, "render_items: null device buffers");
  ARG_CHECK(ng >= 1 && ng <= RK_MAXQ, "render_items: 1 <= n_groups <= 4096");
  // render.jl:354 ranks a state without users as zeros; one user without a list per group stands in for its (absent) users
  const std::vector<float> zeros((size_t)std::max<int64_t>(cand_off[ng], 1), 0.f);
  Request rq;
  rq.nq = ng; rq.ng = ng;
  RankCands rc;
  rc.cand_off = cand_off; rc.partialk = partialk; rc.penalties = penalties; rc.r_in = zeros.data();
  return rank_request_body(m, medium, rq, rc, nullptr, nullptr, dev);
}

int model_rank_gram(Model* m, int medium, int32_t ng, const int64_t* cand_off, const int32_t* cand_ids, float* out, int64_t n_out) {
  ARG_CHECK(medium == 0 || medium == 1, "rank_gram: medium must be 0 or 1");
  ARG_CHECK(ng >= 1 && out, "rank_gram: n_groups >= 1 and an output buffer");
  Groups gs;
  RC(make_groups("rank_gram", ng, cand_off, cand_ids, nullptr, nullptr, medium == 0 ? m->V0 : m->V1, gs));
  ARG_CHECK(n_out == gs.gram, "rank_gram: out must hold sum over groups of n_g * n_g floats");
  int64_t dim = 0;
  const float* E = retrieve_similarity_table(m, medium, &dim);
  ARG_CHECK(E != nullptr, "rank_gram: the item-similarity embeddings of the medium are not loaded");
  HIP_CHECK(hipSetDevice(m->device));
  hipStream_t s = m->stream;
  RankGroup* d_grp; int32_t* d_cand; float* G;
  RC(carve_into(rank_tables(m)->ws, s, [&](Carve& c) {
    d_grp = c.take<RankGroup>(ng);
    d_cand = c.take<int32_t>(gs.N);
    G = c.take<float>(gs.gram);
  }));
  HIP_CHECK(hipMemcpyAsync(d_grp, gs.g.data(), (size_t)ng * sizeof(RankGroup), hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_cand, cand_ids, (size_t)gs.N * 4, hipMemcpyHostToDevice, s));
  RC(launch_gram(m, gs, d_grp, d_cand, E, (int)dim, G));
  HIP_CHECK(hipMemcpyAsync(out, G, (size_t)gs.gram * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

int op_rerank(int32_t n, int32_t partialk, const float* pen, const float* r, const float* gram, const int32_t* ss_bits,
              const int32_t* related_bits, int32_t* picks) {
  ARG_CHECK(r && gram && ss_bits && related_bits && picks && pen, "rsys_op_rerank: null buffer");
  ARG_CHECK(n >= 1 && n <= RK_MAXN, "rsys_op_rerank: 1 <= n <= 1024");
  ARG_CHECK(partialk >= 1, "rsys_op_rerank: partialk >= 1");
  RankGroup d{};
  d.n = n; d.k = std::min(partialk, n);
  d.decay = pen[0]; d.mmr = pen[1]; d.ss = pen[2]; d.rel = pen[3];
  RankGroup* d_grp = nullptr;
  HIP_CHECK(hipMalloc(&d_grp, sizeof(RankGroup)));
  int rc = RSYS_OK;
  if (hipMemcpy(d_grp, &d, sizeof d, hipMemcpyHostToDevice) != hipSuccess) rc = RSYS_ERR_HIP;
  if (rc == RSYS_OK) {
    rerank_kernel<<<1, RK_MAXN>>>(d_grp, r, gram, (const unsigned*)ss_bits, (const unsigned*)related_bits, picks);
    if (hipGetLastError() != hipSuccess) { set_error("rsys_op_rerank: launch failed"); rc = RSYS_ERR_HIP; }
  }
  const hipError_t e = hipDeviceSynchronize();
  hipFree(d_grp);
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("rsys_op_rerank: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  return rc;
}

// rsys_op_query_weights, the ranking section: one launch of rank_score_w_kernel over device arrays; the groups' descriptors are built
// from the host offsets as rsys_rank_request builds them
int op_rank_score_weighted(int32_t ng, const int64_t* cand_off, const int32_t* cand, const float* z, int64_t ldz, const float* lse,
                           const int32_t* members, const int32_t* ranges, int32_t q0, const float* rm, const int64_t* rm_off,
                           const float* retrieval_coef, const float* rating_coefs, float rating_mean, int32_t first, const float* user_w,
                           float* sc) {
  ARG_CHECK(cand && z && lse && members && ranges && rm && rm_off && user_w && sc, "rsys_op_query_weights: null buffer (rank score)");
  ARG_CHECK(ng >= 1 && ng <= 65535 && q0 >= 0, "rsys_op_query_weights: 1 <= n_groups <= 65535, q0 >= 0");
  Groups gs;
  RC(make_groups("rsys_op_query_weights", ng, cand_off, nullptr, nullptr, nullptr, 0, gs, true));
  RankGroup* d_grp = nullptr;
  HIP_CHECK(hipMalloc(&d_grp, (size_t)ng * sizeof(RankGroup)));
  int rc = RSYS_OK;
  if (hipMemcpy(d_grp, gs.g.data(), (size_t)ng * sizeof(RankGroup), hipMemcpyHostToDevice) != hipSuccess) rc = RSYS_ERR_HIP;
  if (rc == RSYS_OK) {
    const float coef = retrieval_coef ? *retrieval_coef : 1.f;
    const int have_rc = rating_coefs != nullptr;
    const float c0m = have_rc ? rating_coefs[0] * rating_mean : 0.f, c1 = have_rc ? rating_coefs[1] : 0.f;
    rank_score_w_kernel<<<dim3(RK_MAXN / RK_THREADS, (unsigned)ng), RK_THREADS>>>(d_grp, cand, z, ldz, lse, members, (const int2*)ranges, q0, rm,
                                                                                 rm_off, coef, logf(coef), have_rc, c0m, c1, first, user_w, sc);
    if (hipGetLastError() != hipSuccess) { set_error("rsys_op_query_weights: launch failed (rank score)"); rc = RSYS_ERR_HIP; }
  }
  const hipError_t e = hipDeviceSynchronize();
  hipFree(d_grp);
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("rsys_op_query_weights: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  return rc;
}

}  // namespace rsys
