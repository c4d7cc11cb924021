// Retrieval top-k on the device (Finetune/embed.jl:86-90 + the scoring, masking and sort of Inference/render.jl:240-333): a request's
// query embeddings against the fused item table of one medium (the tied watch head, model.py:148-170), log soft-max per query, summed
// per group of queries on top of a prior, exclusions, and the best k items per group.  Only k ids and k scores per group leave the
// device.  The pipeline (DESIGN.md "Retrieval top-k"):
//   scores     gemm<T> "gemm_retrieve": z = Q F_m^T in fp32, at most 256 query rows per launch (one pass over the table per chunk)
//   lse        per row: RT_LSE_SPLIT workgroups each fold a slice into (max, sum of exp) partials, one ordered combine per row
//   combine    score_g[i] = prior_g[i] + sum over the group's queries, in query order, of (z_q[i] - lse_q); on the last chunk the
//              same pass maps each score to an order-preserving uint32 key (0 = excluded / -inf / NaN) and counts the first 8-bit
//              digit of the keys into a per-group histogram (wave-aggregated LDS counts, then one global add per bin)
//   select     radix select, at most four digit passes: a small kernel per pass picks each group's digit and the remaining rank
//   compact    keys above the threshold go to the group's candidate list, keys equal to it in ascending id order; every slot is an
//              exclusive prefix of per-workgroup counts over workgroup order (no atomics: independent of scheduling)
//   sort       bitonic sort of <= 8192 (key, id) pairs per group in LDS: descending key, then ascending id; -1 / -inf padding
// Every launch covers all groups (grid = blocks x groups); the host waits once, after the copy out.
// rsys_retrieve_window replaces select / compact / sort by their windowed forms (win_*_kernel): two rank bounds
// per group, the items between them, a sort of <= 1024 pairs -- any 1024 ranks of the ordering in n_groups x 1024 candidate slots.
#include <cmath>

#include "model_internal.hpp"

namespace rsys {

namespace {

constexpr int RT_THREADS = 256;
constexpr int RT_ITEMS = 1024;        // items per workgroup of the per-item passes (4 per thread)
constexpr int RT_CHUNK = 256;         // query rows per score GEMM
constexpr int RT_LSE_SPLIT = 64;      // workgroups per row of the log-sum-exp
constexpr int RT_MAXK = 8192;         // candidates per group: the sort's LDS holds 8192 x 8 B = 64 KiB
constexpr int RT_MAXQ = 4096;
constexpr int RT_WIN = 1024;          // ranks of one window (rsys_retrieve_window): one per lane of the window sort, 8 KiB of LDS

// selection state of one group: keys with (key & rmask) > prefix are taken, keys with (key & rmask) == prefix are ties of which the
// first `need` in ascending id order are taken; total = min(k, admissible) = the group's output count
struct SelState {
  unsigned prefix, rmask;
  int need, total, done, pad0, pad1, pad2;
};

// score_key (common.hpp) is the order-preserving key; key_score maps a key back to its score
__device__ __forceinline__ float key_score(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// h[digit] += 1 for every lane with `valid`, one LDS atomic per distinct digit of the wave (equal scores all land in one bin: the
// wave's leader counts its run of equal digits with a ballot instead of 64 atomics on one address).  Called by all 64 lanes.
__device__ __forceinline__ void hist_add_wave(unsigned* h, unsigned digit, bool valid) {
  unsigned long long act = __ballot(valid);
  while (act) {
    const int leader = __builtin_ctzll(act);
    const unsigned d = __shfl(digit, leader, 64);
    const unsigned long long same = __ballot(valid && digit == d);
    if (lane_id() == leader) atomicAdd(&h[d], (unsigned)__popcll(same));
    act &= ~same;
  }
}

__device__ __forceinline__ void lse_fold(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  if (mx == -INFINITY) return;
  s = (m == -INFINITY ? 0.f : s * expf(m - mx)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mx));
  m = mx;
}

// (max, sum exp(z - max)) of slice blockIdx.x of row blockIdx.y; one online pass, then a fixed-order fold (lanes, then waves)
__global__ void __launch_bounds__(RT_THREADS) lse_partial_kernel(const float* z, long long ldz, int V, float2* part) {
  const int row = blockIdx.y, p = blockIdx.x, P = gridDim.x;
  const long long lo = (long long)V * p / P, hi = (long long)V * (p + 1) / P;
  const float* zr = z + row * ldz;
  float m = -INFINITY, s = 0.f;
  for (long long i = lo + threadIdx.x; i < hi; i += RT_THREADS) {
    const float x = zr[i];
    if (x > m) { s = (m == -INFINITY ? 0.f : s * expf(m - x)) + 1.f; m = x; }
    else s += expf(x - m);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    lse_fold(m, s, m2, s2);
  }
  __shared__ float sm[2][RT_THREADS / 64];
  const int w = threadIdx.x >> 6;
  if (lane_id() == 0) { sm[0][w] = m; sm[1][w] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0][0], S = sm[1][0];
    for (int i = 1; i < RT_THREADS / 64; ++i) lse_fold(M, S, sm[0][i], sm[1][i]);
    part[(long long)row * P + p] = make_float2(M, S);
  }
}
// lse[q0 + row] = log sum exp of row `row`, its partials folded in slice order
__global__ void lse_final_kernel(const float2* part, int P, int rows, int q0, float* lse) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  float m = -INFINITY, s = 0.f;
  for (int p = 0; p < P; ++p) { const float2 v = part[(long long)row * P + p]; lse_fold(m, s, v.x, v.y); }
  lse[q0 + row] = m + logf(s);
}

__global__ void scatter_nan_kernel(float* sc, const long long* pos, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) sc[pos[i]] = __int_as_float(0x7fc00000);
}

// score_g[i] = src_g[i] + sum over the group's queries of this chunk (members[range.x .. range.y), ascending query index) of
// (z_q[i] - lse_q).  LAST: write the key instead of the score and count the keys' first digit (bits 31..24) into hist[g][256].
// ranges == nullptr: no queries (the op hook: keys of given scores).
// W (combine_w_kernel; rsys_query_weights_set): the term of query q is w[q] * (z_q[i] - lse_q), the product and
// the sum rounded on their own; a query whose weight is +-0.0 is skipped, so the running sum keeps its bits whatever the term holds.
// W == false (combine_kernel) never reads `w`.
template <bool LAST, bool W>
__device__ __forceinline__ void combine_body(const float* src, long long lds, float* dst, long long ldd, const float* z, long long ldz,
                                             const float* lse, const int* members, const int2* ranges, int q0, int V, unsigned* hist,
                                             const float* w) {
  const int g = blockIdx.y;
  const int2 r = ranges ? ranges[g] : make_int2(0, 0);
  if (!LAST && r.x == r.y) return;   // (in place, nothing to add)
  __shared__ unsigned h[256];
  if (LAST) { h[threadIdx.x] = 0; __syncthreads(); }
  const long long base = (long long)blockIdx.x * RT_ITEMS;
  const float* sg = src + g * lds;
  float* dg = dst + g * ldd;
  for (int j = 0; j < RT_ITEMS / RT_THREADS; ++j) {
    const long long i = base + j * RT_THREADS + threadIdx.x;
    const bool valid = i < V;
    float s = valid ? sg[i] : 0.f;
    if (valid)
      for (int t = r.x; t < r.y; ++t) {
        const int q = members[t];
        if constexpr (W) {
          s = weighted_add(s, w[q], __fsub_rn(z[(long long)(q - q0) * ldz + i], lse[q]));
        } else {
          s += z[(long long)(q - q0) * ldz + i] - lse[q];
        }
      }
    if (!LAST) {
      if (valid) dg[i] = s;
    } else {
      const unsigned key = valid ? score_key(s) : 0u;
      if (valid) ((unsigned*)dg)[i] = key;
      hist_add_wave(h, key >> 24, key != 0u);
    }
  }
  if (LAST) {
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[g * 256 + threadIdx.x], h[threadIdx.x]);
  }
}
template <bool LAST>
__global__ void __launch_bounds__(RT_THREADS) combine_kernel(const float* src, long long lds, float* dst, long long ldd, const float* z,
                                                             long long ldz, const float* lse, const int* members, const int2* ranges,
                                                             int q0, int V, unsigned* hist) {
  combine_body<LAST, false>(src, lds, dst, ldd, z, ldz, lse, members, ranges, q0, V, hist, nullptr);
}
// the weighted form: w[q] per query, indexed as lse is
template <bool LAST>
__global__ void __launch_bounds__(RT_THREADS) combine_w_kernel(const float* src, long long lds, float* dst, long long ldd, const float* z,
                                                               long long ldz, const float* lse, const int* members, const int2* ranges,
                                                               int q0, int V, unsigned* hist, const float* w) {
  combine_body<LAST, true>(src, lds, dst, ldd, z, ldz, lse, members, ranges, q0, V, hist, w);
}

// digit pass `pass` (digit = bits [24 - 8 pass, 32 - 8 pass)) of every group still open: pick the bin that holds the need-th largest
// candidate, narrow the prefix to it, clear the histogram for the next pass.  Pass 0 also sets the group's output count.
__global__ void __launch_bounds__(RT_THREADS) select_step_kernel(unsigned* hist, SelState* st, int k, int pass) {
  const int g = blockIdx.x;
  SelState* S = st + g;
  if (pass > 0 && S->done) return;
  __shared__ unsigned c[256];
  c[threadIdx.x] = hist[g * 256 + threadIdx.x];
  hist[g * 256 + threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  SelState t = *S;
  if (pass == 0) {
    unsigned adm = 0;
    for (int b = 0; b < 256; ++b) adm += c[b];
    t.prefix = 0; t.rmask = 0; t.done = 0;
    if ((int)adm <= k) {   // every admissible item is in: no digit to resolve
      t.need = (int)adm; t.total = (int)adm; t.done = 1;
      *S = t;
      return;
    }
    t.need = k; t.total = k;
  }
  const int shift = 24 - 8 * pass;
  unsigned cum = 0;
  int b = 255;
  for (; b > 0; --b) {
    if (cum + c[b] >= (unsigned)t.need) break;
    cum += c[b];
  }
  t.prefix |= (unsigned)b << shift;
  t.rmask |= 0xffu << shift;
  t.need -= (int)cum;
  if (c[b] == (unsigned)t.need || shift == 0) t.done = 1;   // (every key of the bin is taken, or the key is resolved)
  *S = t;
}

// histogram of digit (key >> shift) & 255 over the keys matching an open group's prefix
__global__ void __launch_bounds__(RT_THREADS) hist_pass_kernel(const unsigned* keys, long long ldk, int V, const SelState* st, int shift,
                                                               unsigned* hist) {
  const int g = blockIdx.y;
  const SelState S = st[g];
  if (S.done) return;
  __shared__ unsigned h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const unsigned* kg = keys + g * ldk;
  const long long base = (long long)blockIdx.x * RT_ITEMS;
  for (int j = 0; j < RT_ITEMS / RT_THREADS; ++j) {
    const long long i = base + j * RT_THREADS + threadIdx.x;
    const unsigned key = i < V ? kg[i] : 0u;
    hist_add_wave(h, (key >> shift) & 0xffu, key != 0u && (key & S.rmask) == S.prefix);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[g * 256 + threadIdx.x], h[threadIdx.x]);
}

__device__ __forceinline__ bool is_tie(unsigned key, const SelState& S) { return key != 0u && (key & S.rmask) == S.prefix; }
__device__ __forceinline__ bool is_above(unsigned key, const SelState& S) { return key != 0u && (key & S.rmask) > S.prefix; }

__device__ __forceinline__ unsigned long long cand_pack(unsigned key, long long id) {
  return ((unsigned long long)key << 32) | (unsigned long long)(0xffffffffu - (unsigned)id);
}

// exact integer sum over the workgroup (every thread gets it)
__device__ __forceinline__ int block_sum_int(int v, int* smem /* >= 4 */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if (lane_id() == 0) smem[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = 0;
  for (int i = 0; i < RT_THREADS / 64; ++i) r += smem[i];
  return r;
}

// cnt[g][blockIdx.x] = {keys above the threshold, keys equal to it} among this workgroup's items
__global__ void __launch_bounds__(RT_THREADS) count_kernel(const unsigned* keys, long long ldk, int V, const SelState* st, int2* cnt) {
  const int g = blockIdx.y;
  const SelState S = st[g];
  const unsigned* kg = keys + g * ldk;
  const long long base = (long long)blockIdx.x * RT_ITEMS;
  int na = 0, nt = 0;
  for (int j = 0; j < RT_ITEMS / RT_THREADS; ++j) {
    const long long i = base + j * RT_THREADS + threadIdx.x;
    const unsigned key = i < V ? kg[i] : 0u;
    na += is_above(key, S) ? 1 : 0;
    nt += is_tie(key, S) ? 1 : 0;
  }
  __shared__ int sm[RT_THREADS / 64];
  const int a = block_sum_int(na, sm);
  const int t = block_sum_int(nt, sm);
  if (threadIdx.x == 0) cnt[(long long)g * gridDim.x + blockIdx.x] = make_int2(a, t);
}

// candidate list of group g: [0, total - need) the keys above the threshold, [total - need, total) the first `need` threshold-equal
// keys by ascending id.  Every item's slot is an exclusive prefix over workgroup order (the counts of count_kernel), then over the
// waves and lanes of the workgroup: no atomics, the list does not depend on scheduling.
__global__ void __launch_bounds__(RT_THREADS) compact_kernel(const unsigned* keys, long long ldk, int V, const SelState* st, const int2* cnt,
                                                             unsigned long long* cand, int ldc) {
  const int g = blockIdx.y, nb = gridDim.x;
  const SelState S = st[g];
  const unsigned* kg = keys + g * ldk;
  unsigned long long* cg = cand + (long long)g * ldc;
  const int above0 = S.total - S.need;
  __shared__ int sm[RT_THREADS / 64];
  __shared__ int wa[RT_THREADS / 64], wt[RT_THREADS / 64];
  int a0 = 0, t0 = 0;
  for (int b = threadIdx.x; b < blockIdx.x; b += RT_THREADS) { const int2 c = cnt[(long long)g * nb + b]; a0 += c.x; t0 += c.y; }
  int abase = block_sum_int(a0, sm);
  int tbase = block_sum_int(t0, sm);
  const int w = threadIdx.x >> 6, lane = lane_id();
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long long base = (long long)blockIdx.x * RT_ITEMS;
  for (int j = 0; j < RT_ITEMS / RT_THREADS; ++j) {
    const long long i = base + j * RT_THREADS + threadIdx.x;
    const unsigned key = i < V ? kg[i] : 0u;
    const bool above = is_above(key, S), tie = is_tie(key, S);
    const unsigned long long ba = __ballot(above), bt = __ballot(tie);
    if (lane == 0) { wa[w] = __popcll(ba); wt[w] = __popcll(bt); }
    __syncthreads();
    int oa = abase, ot = tbase, ta = 0, tt = 0;
    for (int v = 0; v < RT_THREADS / 64; ++v) {
      if (v < w) { oa += wa[v]; ot += wt[v]; }
      ta += wa[v]; tt += wt[v];
    }
    __syncthreads();
    if (above) {
      const int slot = oa + __popcll(ba & lt);
      if (slot < above0) cg[slot] = cand_pack(key, i);   // (always: the select passes counted exactly above0 of them)
    }
    if (tie) {
      const int rank = ot + __popcll(bt & lt);
      if (rank < S.need) cg[above0 + rank] = cand_pack(key, i);
    }
    abase += ta; tbase += tt;
  }
}

// sort group g's candidates (descending key, ascending id) and write ids / scores / count, padding with -1 / -inf
__global__ void __launch_bounds__(1024) sort_out_kernel(const unsigned long long* cand, int ldc, const SelState* st, int k, int* ids,
                                                        float* vals, int* counts) {
  const int g = blockIdx.x;
  const int n = st[g].total;
  __shared__ unsigned long long s[RT_MAXK];
  int N2 = 1;
  while (N2 < n) N2 <<= 1;
  const unsigned long long* cg = cand + (long long)g * ldc;
  for (int i = threadIdx.x; i < N2; i += 1024) s[i] = i < n ? cg[i] : 0ull;
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
  int* ig = ids + (long long)g * k;
  float* vg = vals + (long long)g * k;
  for (int i = threadIdx.x; i < k; i += 1024) {
    if (i < n) {
      const unsigned long long v = s[i];
      ig[i] = (int)(0xffffffffu - (unsigned)v);
      vg[i] = key_score((unsigned)(v >> 32));
    } else {
      ig[i] = -1;
      vg[i] = -INFINITY;
    }
  }
  if (threadIdx.x == 0) counts[g] = n;
}


// ---- windowed selection (rsys_retrieve_window): the items of ranks [start, start + len) of the same ordering, len <= RT_WIN, as
// (top-stop) minus (top-start) with stop = min(start + len, total).  Each of the two rank bounds is resolved by the radix select
// above to an exact pair (T, need): the top-c set is every key above T plus the first `need` keys equal to T in ascending id order.
// st[g] is the bound of the window's end (c = stop), st[ng + g] that of its start (c = min(start, total)); prefix holds T, rmask is
// full once the bound is exact.  c == 0 is T = 0xffffffff (no score has that key), c == total is T = 0 (every admissible key is above).
// The candidate list of a group holds the window only: [n_groups][RT_WIN] whatever `start` is.

__device__ __forceinline__ int win_count(int adm, long long start, int len) {
  const long long left = (long long)adm - start;
  return left <= 0 ? 0 : (int)(left < len ? left : len);
}

// digit pass `pass` of both bounds of group blockIdx.x (wave 0: the end, wave 1: the start).  hist rows [0, ng) hold the end's
// histograms and, in pass 0, the first-digit histogram both bounds start from; rows [ng, 2 ng) the start's.  A bound whose bin is
// taken whole falls between two keys: T = the bin's smallest key - 1, need = 0.
__global__ void __launch_bounds__(RT_THREADS) win_select_step_kernel(unsigned* hist, SelState* st, const long long* wstart, const int* wlen,
                                                                     int ng, int pass) {
  const int g = blockIdx.x;
  __shared__ unsigned c[2][256];
  c[0][threadIdx.x] = hist[g * 256 + threadIdx.x];
  c[1][threadIdx.x] = pass == 0 ? c[0][threadIdx.x] : hist[(ng + g) * 256 + threadIdx.x];
  hist[g * 256 + threadIdx.x] = 0;
  hist[(ng + g) * 256 + threadIdx.x] = 0;
  __syncthreads();
  if (lane_id() != 0 || threadIdx.x >= 128) return;
  const int bound = threadIdx.x >> 6;
  const unsigned* cb = c[bound];
  SelState* S = st + bound * ng + g;
  SelState t = *S;
  if (pass > 0 && t.done) return;
  if (pass == 0) {
    unsigned adm = 0;
    for (int b = 0; b < 256; ++b) adm += cb[b];
    const long long s0 = wstart[g];
    const int lo = s0 < (long long)adm ? (int)s0 : (int)adm;
    const int cnt = bound == 0 ? lo + win_count((int)adm, s0, wlen[g]) : lo;
    t.total = (int)adm; t.need = 0; t.rmask = 0xffffffffu; t.done = 1;
    t.pad0 = t.pad1 = t.pad2 = 0;
    if (cnt <= 0) { t.prefix = 0xffffffffu; *S = t; return; }
    if (cnt >= (int)adm) { t.prefix = 0u; *S = t; return; }
    t.prefix = 0; t.rmask = 0; t.done = 0; t.need = cnt;
  }
  const int shift = 24 - 8 * pass;
  unsigned cum = 0;
  int b = 255;
  for (; b > 0; --b) {
    if (cum + cb[b] >= (unsigned)t.need) break;
    cum += cb[b];
  }
  t.prefix |= (unsigned)b << shift;
  t.rmask |= 0xffu << shift;
  t.need -= (int)cum;
  if (shift == 0) {
    t.done = 1;
  } else if (cb[b] == (unsigned)t.need) {
    t.prefix = (t.prefix ? t.prefix : 1u) - 1u; t.rmask = 0xffffffffu; t.need = 0; t.done = 1;
  }
  *S = t;
}

// one read of the keys for both bounds: histogram of digit (key >> shift) & 255 over the keys matching each open bound's prefix
__global__ void __launch_bounds__(RT_THREADS) win_hist_pass_kernel(const unsigned* keys, long long ldk, int V, const SelState* st, int ng,
                                                                   int shift, unsigned* hist) {
  const int g = blockIdx.y;
  const SelState A = st[g], B = st[ng + g];
  if (A.done && B.done) return;
  __shared__ unsigned h[2][256];
  h[0][threadIdx.x] = 0; h[1][threadIdx.x] = 0;
  __syncthreads();
  const unsigned* kg = keys + g * ldk;
  const long long base = (long long)blockIdx.x * RT_ITEMS;
  for (int j = 0; j < RT_ITEMS / RT_THREADS; ++j) {
    const long long i = base + j * RT_THREADS + threadIdx.x;
    const unsigned key = i < V ? kg[i] : 0u;
    const unsigned digit = (key >> shift) & 0xffu;
    if (!A.done) hist_add_wave(h[0], digit, is_tie(key, A));
    if (!B.done) hist_add_wave(h[1], digit, is_tie(key, B));
  }
  __syncthreads();
  if (h[0][threadIdx.x]) atomicAdd(&hist[g * 256 + threadIdx.x], h[0][threadIdx.x]);
  if (h[1][threadIdx.x]) atomicAdd(&hist[(ng + g) * 256 + threadIdx.x], h[1][threadIdx.x]);
}

// the three classes a window's items come from, for a key and the two thresholds TS <= TB (end, start)
__device__ __forceinline__ bool win_between(unsigned key, unsigned TS, unsigned TB) { return key > TS && key < TB; }
__device__ __forceinline__ bool win_at(unsigned key, unsigned T) { return key != 0u && key == T; }

// cnt[g][blockIdx.x] = {keys strictly between the thresholds, keys equal to the start's, keys equal to the end's} of this workgroup
__global__ void __launch_bounds__(RT_THREADS) win_count_kernel(const unsigned* keys, long long ldk, int V, const SelState* st, int ng, int4* cnt) {
  const int g = blockIdx.y;
  const unsigned TS = st[g].prefix, TB = st[ng + g].prefix;
  const unsigned* kg = keys + g * ldk;
  const long long base = (long long)blockIdx.x * RT_ITEMS;
  int nw = 0, nb = 0, ns = 0;
  for (int j = 0; j < RT_ITEMS / RT_THREADS; ++j) {
    const long long i = base + j * RT_THREADS + threadIdx.x;
    const unsigned key = i < V ? kg[i] : 0u;
    nw += win_between(key, TS, TB) ? 1 : 0;
    nb += win_at(key, TB) ? 1 : 0;
    ns += win_at(key, TS) ? 1 : 0;
  }
  __shared__ int sm[RT_THREADS / 64];
  const int w = block_sum_int(nw, sm);
  const int b = block_sum_int(nb, sm);
  const int s = block_sum_int(ns, sm);
  if (threadIdx.x == 0) cnt[(long long)g * gridDim.x + blockIdx.x] = make_int4(w, b, s, 0);
}

// the window's candidate list cand[g][0 .. n): [0, W) the keys strictly between the thresholds (W = their number), then the keys equal
// to the start's threshold whose tie rank (ascending id) is >= the start's need, then those equal to the end's whose tie rank is < the
// end's need; one threshold for both: the ties of rank [need_start, need_end).  Every slot is an exclusive prefix over workgroup
// order, waves and lanes, as in compact_kernel: no atomics.  The sort orders the list, so the order of the classes does not matter.
__global__ void __launch_bounds__(RT_THREADS) win_compact_kernel(const unsigned* keys, long long ldk, int V, const SelState* st, int ng,
                                                                 const long long* wstart, const int* wlen, const int4* cnt,
                                                                 unsigned long long* cand) {
  const int g = blockIdx.y, nblk = gridDim.x;
  const SelState SS = st[g], SB = st[ng + g];
  const unsigned TS = SS.prefix, TB = SB.prefix;
  const int n = win_count(SS.total, wstart[g], wlen[g]);
  if (n == 0) return;
  const bool same = TS == TB;
  const unsigned* kg = keys + g * ldk;
  unsigned long long* cg = cand + (long long)g * RT_WIN;
  __shared__ int sm[RT_THREADS / 64];
  __shared__ int ww[RT_THREADS / 64], wb[RT_THREADS / 64], ws[RT_THREADS / 64];
  int pw = 0, pb = 0, ps = 0, aw = 0, ab = 0;   // before this workgroup; over all workgroups
  for (int b = threadIdx.x; b < nblk; b += RT_THREADS) {
    const int4 c = cnt[(long long)g * nblk + b];
    if (b < blockIdx.x) { pw += c.x; pb += c.y; ps += c.z; }
    aw += c.x; ab += c.y;
  }
  int wbase = block_sum_int(pw, sm);
  int bbase = block_sum_int(pb, sm);
  int sbase = block_sum_int(ps, sm);
  const int W = block_sum_int(aw, sm);
  const int tail_b = W - SB.need;                                  // slot of the start's tie of rank r: tail_b + r
  const int tail_s = W + block_sum_int(ab, sm) - SB.need;          // slot of the end's tie of rank r: tail_s + r
  const int w = threadIdx.x >> 6, lane = lane_id();
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long long base = (long long)blockIdx.x * RT_ITEMS;
  for (int j = 0; j < RT_ITEMS / RT_THREADS; ++j) {
    const long long i = base + j * RT_THREADS + threadIdx.x;
    const unsigned key = i < V ? kg[i] : 0u;
    const bool inw = win_between(key, TS, TB), atb = win_at(key, TB), ats = win_at(key, TS);
    const unsigned long long bw = __ballot(inw), bb = __ballot(atb), bs = __ballot(ats);
    if (lane == 0) { ww[w] = __popcll(bw); wb[w] = __popcll(bb); ws[w] = __popcll(bs); }
    __syncthreads();
    int ow = wbase, ob = bbase, os = sbase, tw = 0, tb = 0, ts = 0;
    for (int v = 0; v < RT_THREADS / 64; ++v) {
      if (v < w) { ow += ww[v]; ob += wb[v]; os += ws[v]; }
      tw += ww[v]; tb += wb[v]; ts += ws[v];
    }
    __syncthreads();
    int slot = -1;
    if (inw) {
      slot = ow + __popcll(bw & lt);
    } else if (atb) {
      const int r = ob + __popcll(bb & lt);
      if (r >= SB.need && (!same || r < SS.need)) slot = same ? r - SB.need : tail_b + r;
    } else if (ats) {
      const int r = os + __popcll(bs & lt);
      if (r < SS.need) slot = tail_s + r;
    }
    if (slot >= 0 && slot < n) cg[slot] = cand_pack(key, i);   // (slot < n always: the bounds counted exactly n members)
    wbase += tw; bbase += tb; sbase += ts;
  }
}

// sort group g's window (descending key, ascending id), one candidate per lane, and write ids / scores / count / total with -1 / -inf padding
__global__ void __launch_bounds__(RT_WIN) win_sort_kernel(const unsigned long long* cand, const SelState* st, const long long* wstart,
                                                          const int* wlen, int* ids, float* vals, int* counts, int* totals) {
  const int g = blockIdx.x, i = threadIdx.x;
  const int adm = st[g].total;
  const int n = win_count(adm, wstart[g], wlen[g]);
  __shared__ unsigned long long s[RT_WIN];
  s[i] = i < n ? cand[(long long)g * RT_WIN + i] : 0ull;
  __syncthreads();
  int N2 = 1;
  while (N2 < n) N2 <<= 1;
  for (int size = 2; size <= N2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (i < N2 / 2) {
        const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const unsigned long long a = s[lo], b = s[hi];
        if ((a < b) == desc) { s[lo] = b; s[hi] = a; }
      }
      __syncthreads();
    }
  }
  const unsigned long long v = s[i];
  ids[(long long)g * RT_WIN + i] = i < n ? (int)(0xffffffffu - (unsigned)v) : -1;
  vals[(long long)g * RT_WIN + i] = i < n ? key_score((unsigned)(v >> 32)) : -INFINITY;
  if (i == 0) { counts[g] = n; totals[g] = adm; }
}

#define RT_LAUNCH_CHECK() HIP_CHECK(hipGetLastError())

// device buffers of the selection stage
struct SelBufs {
  unsigned* hist;          // [rows][256], zero on entry (pass 0 filled by combine_kernel<true>)
  SelState* st;            // [rows]
  int2* cnt;               // [rows][nb]
  unsigned long long* cand; int ldc;   // [rows][ldc >= k]
};

// radix select + compaction + sort on keys [rows][ldk] whose first-digit histogram is in b.hist
int topk_select(const unsigned* keys, long long ldk, int rows, int V, int k, const SelBufs& b, int* ids, float* vals, int* counts,
                hipStream_t s) {
  const int nb = (V + RT_ITEMS - 1) / RT_ITEMS;
  const dim3 grid(nb, rows);
  select_step_kernel<<<rows, RT_THREADS, 0, s>>>(b.hist, b.st, k, 0);
  RT_LAUNCH_CHECK();
  for (int pass = 1; pass < 4; ++pass) {
    hist_pass_kernel<<<grid, RT_THREADS, 0, s>>>(keys, ldk, V, b.st, 24 - 8 * pass, b.hist);
    RT_LAUNCH_CHECK();
    select_step_kernel<<<rows, RT_THREADS, 0, s>>>(b.hist, b.st, k, pass);
    RT_LAUNCH_CHECK();
  }
  count_kernel<<<grid, RT_THREADS, 0, s>>>(keys, ldk, V, b.st, b.cnt);
  RT_LAUNCH_CHECK();
  compact_kernel<<<grid, RT_THREADS, 0, s>>>(keys, ldk, V, b.st, b.cnt, b.cand, b.ldc);
  RT_LAUNCH_CHECK();
  sort_out_kernel<<<rows, 1024, 0, s>>>(b.cand, b.ldc, b.st, k, ids, vals, counts);
  RT_LAUNCH_CHECK();
  return RSYS_OK;
}

// the window [wstart[g], wstart[g] + wlen[g]) of every row's ordering on keys [rows][ldk] whose first-digit histogram is in rows
// [0, rows) of b.hist ([2 rows][256], the rest zero); b.st [2 rows], b.cnt [rows][nb] int4, b.cand [rows][RT_WIN]
int window_select(const unsigned* keys, long long ldk, int rows, int V, const long long* wstart, const int* wlen, const SelBufs& b, int* ids,
                  float* vals, int* counts, int* totals, hipStream_t s) {
  const int nb = (V + RT_ITEMS - 1) / RT_ITEMS;
  const dim3 grid(nb, rows);
  win_select_step_kernel<<<rows, RT_THREADS, 0, s>>>(b.hist, b.st, wstart, wlen, rows, 0);
  RT_LAUNCH_CHECK();
  for (int pass = 1; pass < 4; ++pass) {
    win_hist_pass_kernel<<<grid, RT_THREADS, 0, s>>>(keys, ldk, V, b.st, rows, 24 - 8 * pass, b.hist);
    RT_LAUNCH_CHECK();
    win_select_step_kernel<<<rows, RT_THREADS, 0, s>>>(b.hist, b.st, wstart, wlen, rows, pass);
    RT_LAUNCH_CHECK();
  }
  win_count_kernel<<<grid, RT_THREADS, 0, s>>>(keys, ldk, V, b.st, rows, (int4*)b.cnt);
  RT_LAUNCH_CHECK();
  win_compact_kernel<<<grid, RT_THREADS, 0, s>>>(keys, ldk, V, b.st, rows, wstart, wlen, (const int4*)b.cnt, b.cand);
  RT_LAUNCH_CHECK();
  win_sort_kernel<<<rows, RT_WIN, 0, s>>>(b.cand, b.st, wstart, wlen, ids, vals, counts, totals);
  RT_LAUNCH_CHECK();
  return RSYS_OK;
}

}  // namespace

int launch_scatter_nan(float* sc, const long long* pos, long long n, hipStream_t s) {
  scatter_nan_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(sc, pos, n);
  RT_LAUNCH_CHECK();
  return RSYS_OK;
}

static_assert(RT_CHUNK == RETRIEVE_CHUNK && RT_LSE_SPLIT == RETRIEVE_LSE_SPLIT, "retrieval chunk constants");

// z[r][0, V_m) = q_{q0 + r} . F_m[i] (gemm_retrieve, fp32 accumulation) and lse[q0 + r] for the nc <= RETRIEVE_CHUNK query rows of one
// chunk; part holds nc * RETRIEVE_LSE_SPLIT partials.  The scoring of rsys_retrieve_topk, shared with rsys_rank_request.
template <typename T>
int retrieve_chunk_scores(Model* m, const T* qt, int nc, int q0, const T* Fm, int Vm, float* z, long long ldz, float2* part, float* lse) {
  hipStream_t s = m->stream;
  StepGemm p = gemm_xwt(qt, m->D, Fm, m->D, z, ldz, nc, Vm, m->D);
  p.c_f32 = 1;
  RC(gemm<T>(m, "gemm_retrieve", p));
  tic(m, "retrieve_lse");
  lse_partial_kernel<<<dim3(RT_LSE_SPLIT, nc), RT_THREADS, 0, s>>>(z, ldz, Vm, part);
  RT_LAUNCH_CHECK();
  lse_final_kernel<<<(nc + 255) / 256, 256, 0, s>>>(part, RT_LSE_SPLIT, nc, q0, lse);
  RT_LAUNCH_CHECK();
  toc(m);
  return RSYS_OK;
}
template int retrieve_chunk_scores<float>(Model*, const float*, int, int, const float*, int, float*, long long, float2*, float*);
template int retrieve_chunk_scores<bf16>(Model*, const bf16*, int, int, const bf16*, int, float*, long long, float2*, float*);

template <typename T>
int score_upload_queries(const ScoreBufs<T>& b, const float* queries, int64_t nq, hipMemcpyKind kind, hipStream_t s) {
  HIP_CHECK(hipMemcpyAsync(b.qf, queries, (size_t)nq * b.D * 4, kind, s));
  if constexpr (is_bf16<T>::value) RC(launch_cast<T>(b.qf, b.qt, (long long)nq * b.D, s));
  return RSYS_OK;
}
template int score_upload_queries<float>(const ScoreBufs<float>&, const float*, int64_t, hipMemcpyKind, hipStream_t);
template int score_upload_queries<bf16>(const ScoreBufs<bf16>&, const float*, int64_t, hipMemcpyKind, hipStream_t);

template <typename T>
int score_table_ready(Model* m, int medium, const T** Fm) {
  if (m->table_dirty) { RC(table_forward<T>(m)); m->table_dirty = false; }
  *Fm = AT<T>(m->FT) + (int64_t)(medium == 0 ? 0 : m->V0) * m->D;
  return RSYS_OK;
}
template int score_table_ready<float>(Model*, int, const float**);
template int score_table_ready<bf16>(Model*, int, const bf16**);

int group_plan(const char* who, const int32_t* group, int64_t nq, int ng, int chunk, GroupPlan& gp, bool allow_empty) {
  gp.goff.assign((size_t)ng + 1, 0);
  for (int64_t q = 0; q < nq; ++q) {
    const int g = group ? group[q] : (int)q;
    ARG_CHECK(g >= 0 && g < ng, std::string(who) + ": group ids must be in [0, n_groups)");
    ++gp.goff[g + 1];
  }
  for (int g = 0; g < ng; ++g) {
    ARG_CHECK(allow_empty || gp.goff[g + 1] > 0, std::string(who) + ": every group needs at least one query");
    gp.goff[g + 1] += gp.goff[g];
  }
  gp.members.resize((size_t)nq);
  std::vector<int> fill(gp.goff.begin(), gp.goff.end() - 1);
  for (int64_t q = 0; q < nq; ++q) gp.members[fill[group ? group[q] : (int)q]++] = (int)q;
  gp.nchunks = (int)((nq + chunk - 1) / chunk);
  gp.ranges.resize((size_t)gp.nchunks * ng);
  for (int g = 0; g < ng; ++g) {
    int t = gp.goff[g];
    for (int c = 0; c < gp.nchunks; ++c) {
      const int lo = t;
      while (t < gp.goff[g + 1] && gp.members[t] < (c + 1) * chunk) ++t;
      gp.ranges[(size_t)c * ng + g] = make_int2(lo, t);
    }
  }
  return RSYS_OK;
}

int check_ragged(const char* who, const ListKind& what, const int64_t* off, int64_t n, std::initializer_list<const void*> arrays) {
  for (const void* a : arrays) ARG_CHECK((off == nullptr) == (a == nullptr), std::string(who) + ": " + what.given);
  if (!off) return RSYS_OK;
  ARG_CHECK(off[0] == 0, std::string(who) + ": " + what.offsets + "[0] must be 0");
  for (int64_t i = 0; i < n; ++i) ARG_CHECK(off[i + 1] >= off[i], std::string(who) + ": " + what.offsets + " must be non-decreasing");
  return RSYS_OK;
}

int check_list_items(const char* who, const ListKind& what, const int64_t* off, int64_t n, const int32_t* medium, const int32_t* ids,
                     const int V[2]) {
  if (!off) return RSYS_OK;
  for (int64_t j = 0; j < off[n]; ++j) {
    if (medium) ARG_CHECK(medium[j] == 0 || medium[j] == 1, std::string(who) + ": " + what.media);
    ARG_CHECK(ids[j] >= 0 && ids[j] < V[medium ? medium[j] : 0], std::string(who) + ": " + what.ids);
  }
  return RSYS_OK;
}

int csc_nonzero_pattern(const char* who, const char* rows, int64_t n_rows, int64_t n_cols, const int64_t* colptr, const int32_t* rowval,
                        const float* nzval, std::vector<int64_t>& cp, std::vector<int32_t>& rv) {
  const std::string w = std::string(who) + ": ";
  ARG_CHECK(colptr[0] == 0, w + "colptr[0] must be 0");
  for (int64_t c = 0; c < n_cols; ++c) ARG_CHECK(colptr[c + 1] >= colptr[c], w + "colptr must be non-decreasing");
  cp.assign((size_t)n_cols + 1, 0);
  rv.reserve((size_t)colptr[n_cols]);
  for (int64_t c = 0; c < n_cols; ++c) {
    for (int64_t j = colptr[c]; j < colptr[c + 1]; ++j) {
      ARG_CHECK(rowval[j] >= 0 && rowval[j] < n_rows, w + "row indices must be in " + rows);
      ARG_CHECK(std::isfinite(nzval[j]) && nzval[j] >= 0.f, w + "stored values must be finite and >= 0");
      if (nzval[j] != 0.f) rv.push_back(rowval[j]);   // (explicitly stored zeros reach nothing: render.jl tests related_vals[k] != 0)
    }
    cp[(size_t)c + 1] = (int64_t)rv.size();
  }
  return RSYS_OK;
}

template <typename T>
static int retrieve_t(Model* m, int medium, const float* queries, int64_t nq, const int32_t* group, int ng, const float* prior,
                      const int64_t* excl_off, const int32_t* excl_ids, const RetrieveInit* init, int k, int32_t* ids_out, float* scores_out,
                      int32_t* counts_out, RetrieveDev* dev = nullptr, const RetrieveWin* win = nullptr, const float* user_w = nullptr) {
  // user_w (host, [nq], or null): a weight per query (rsys_query_weights_set); null runs the unweighted kernels
  // win: the window [start, start + len) of each group's ordering instead of its top k (rsys_retrieve_window): rows of RT_WIN ranks, a
  // group may have no queries (its score row is what `init` wrote), nq may be 0 (nothing is scored, the item table is not read)
  const int Vm = medium == 0 ? m->V0 : m->V1;
  hipStream_t s = m->stream;
  if (win) k = RT_WIN;
  // host-side index arrays: the queries of each group in query order, per chunk the range of them it holds, exclusion positions
  GroupPlan gp;
  RC(group_plan(win ? "retrieve_window" : "retrieve_topk", group, nq, ng, RT_CHUNK, gp, win != nullptr));
  RC(check_ragged("retrieve_topk", LIST_EXCLUDED, excl_off, ng, {excl_ids}));
  RC(check_list_items("retrieve_topk", LIST_EXCLUDED, excl_off, ng, nullptr, excl_ids, &Vm));
  std::vector<long long> xpos;
  if (excl_off)
    for (int g = 0; g < ng; ++g)
      for (int64_t j = excl_off[g]; j < excl_off[g + 1]; ++j) xpos.push_back((long long)g * Vm + excl_ids[j]);
  HIP_CHECK(hipSetDevice(m->device));
  const T* Fm = nullptr;
  if (nq) RC(score_table_ready<T>(m, medium, &Fm));
  // workspace: queries (f32 + compute type), lse, partials, the per-chunk score slab (the candidate lists reuse it after the last
  // chunk), the group scores / keys, the selection state, the outputs, the index arrays
  const int nb = (Vm + RT_ITEMS - 1) / RT_ITEMS;
  ScoreBufs<T> b(m);
  const size_t zrows = win ? (size_t)std::min<int64_t>(nq, RT_CHUNK) : (size_t)RT_CHUNK;
  const size_t slab = std::max<size_t>(zrows * (size_t)b.ldz * 4, (size_t)ng * (size_t)k * 8);
  const size_t nbound = win ? 2 : 1;   // (a window selects two rank bounds per group and counts int4 per workgroup)
  float *sc, *d_vals, *d_uw; SelBufs sb; int *d_ids, *d_counts, *d_members, *d_totals, *d_wlen; int2* d_ranges; long long *d_xpos, *d_wstart;
  RC(carve_into(m->rws, s, [&](Carve& c) {
    b.take(c, nq, slab);
    sc = c.take<float>((size_t)ng * Vm);
    sb.hist = c.take<unsigned>(nbound * ng * 256);
    sb.st = c.take<SelState>(nbound * ng);
    sb.cnt = c.take<int2>(nbound * ng * nb);
    d_ids = c.take<int>((size_t)ng * k);
    d_vals = c.take<float>((size_t)ng * k);
    d_counts = c.take<int>(ng);
    d_members = c.take<int>(nq);
    d_ranges = c.take<int2>(gp.ranges.size());
    d_uw = c.take<float>(user_w ? (size_t)nq : 0);
    d_xpos = c.take<long long>(xpos.size());
    d_totals = c.take<int>(win ? ng : 0);
    d_wstart = c.take<long long>(win ? ng : 0);
    d_wlen = c.take<int>(win ? ng : 0);
  }));
  sb.cand = (unsigned long long*)b.z; sb.ldc = k;

  tic(m, "retrieve_prep");
  // (dev: the queries are on the device already and the result stays there; the arithmetic below is the same)
  if (nq) {
    RC(score_upload_queries(b, dev ? dev->d_queries : queries, nq, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_members, gp.members.data(), gp.members.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_ranges, gp.ranges.data(), gp.ranges.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    if (user_w) HIP_CHECK(hipMemcpyAsync(d_uw, user_w, (size_t)nq * 4, hipMemcpyHostToDevice, s));
  }
  if (win) {
    static_assert(sizeof(long long) == sizeof(int64_t), "window starts are copied as they are");
    HIP_CHECK(hipMemcpyAsync(d_wstart, win->start, (size_t)ng * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_wlen, win->len, (size_t)ng * 4, hipMemcpyHostToDevice, s));
  }
  if (init) RC((*init)(sc, s));   // the device-side initialiser of the group score rows (rsys_retrieve_request)
  else if (prior) HIP_CHECK(hipMemcpyAsync(sc, prior, (size_t)ng * Vm * 4, hipMemcpyHostToDevice, s));
  else HIP_CHECK(hipMemsetAsync(sc, 0, (size_t)ng * Vm * 4, s));
  if (!xpos.empty()) {
    HIP_CHECK(hipMemcpyAsync(d_xpos, xpos.data(), xpos.size() * 8, hipMemcpyHostToDevice, s));
    RC(launch_scatter_nan(sc, d_xpos, (long long)xpos.size(), s));
  }
  HIP_CHECK(hipMemsetAsync(sb.hist, 0, nbound * ng * 256 * 4, s));
  toc(m);
  if (gp.nchunks == 0) {   // (a window call without queries: the keys of the initialised rows)
    combine_kernel<true><<<dim3(nb, ng), RT_THREADS, 0, s>>>(sc, Vm, sc, Vm, nullptr, 0, nullptr, nullptr, nullptr, 0, Vm, sb.hist);
    RT_LAUNCH_CHECK();
  }
  for (int ch = 0; ch < gp.nchunks; ++ch) {
    const int q0 = ch * RT_CHUNK, nc = (int)std::min<int64_t>(RT_CHUNK, nq - q0);
    RC(retrieve_chunk_scores<T>(m, b.qt + (size_t)q0 * b.D, nc, q0, Fm, Vm, b.z, b.ldz, b.part, b.lse));
    tic(m, "retrieve_combine");
    const dim3 grid(nb, ng);
    const bool last = ch + 1 == gp.nchunks;
    const int2* rg = d_ranges + (size_t)ch * ng;
    if (user_w) {
      if (!last) combine_w_kernel<false><<<grid, RT_THREADS, 0, s>>>(sc, Vm, sc, Vm, b.z, b.ldz, b.lse, d_members, rg, q0, Vm, sb.hist, d_uw);
      else combine_w_kernel<true><<<grid, RT_THREADS, 0, s>>>(sc, Vm, sc, Vm, b.z, b.ldz, b.lse, d_members, rg, q0, Vm, sb.hist, d_uw);
    } else {
      if (!last) combine_kernel<false><<<grid, RT_THREADS, 0, s>>>(sc, Vm, sc, Vm, b.z, b.ldz, b.lse, d_members, rg, q0, Vm, sb.hist);
      else combine_kernel<true><<<grid, RT_THREADS, 0, s>>>(sc, Vm, sc, Vm, b.z, b.ldz, b.lse, d_members, rg, q0, Vm, sb.hist);
    }
    RT_LAUNCH_CHECK();
    toc(m);
  }
  tic(m, "retrieve_select");
  if (win) RC(window_select((const unsigned*)sc, Vm, ng, Vm, d_wstart, d_wlen, sb, d_ids, d_vals, d_counts, d_totals, s));
  else RC(topk_select((const unsigned*)sc, Vm, ng, Vm, k, sb, d_ids, d_vals, d_counts, s));
  toc(m);
  if (dev) { dev->d_ids = d_ids; dev->d_vals = d_vals; }
  else {
    HIP_CHECK(hipMemcpyAsync(ids_out, d_ids, (size_t)ng * k * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(scores_out, d_vals, (size_t)ng * k * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipMemcpyAsync(counts_out, d_counts, (size_t)ng * 4, hipMemcpyDeviceToHost, s));
  if (win) HIP_CHECK(hipMemcpyAsync(win->total_out, d_totals, (size_t)ng * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

int model_retrieve_topk(Model* m, int medium, const float* queries, int64_t nq, const int32_t* group, int32_t ng, const float* prior,
                        const int64_t* excl_off, const int32_t* excl_ids, int32_t k, int32_t* ids_out, float* scores_out,
                        int32_t* counts_out) {
  ARG_CHECK(medium == 0 || medium == 1, "retrieve_topk: medium must be 0 or 1");
  ARG_CHECK(!m->sharded, "retrieve_topk: the row-sharded item table is not supported (replicated table only)");
  ARG_CHECK(queries && ids_out && scores_out && counts_out, "retrieve_topk: null buffer");
  ARG_CHECK(nq >= 1 && nq <= RT_MAXQ, "retrieve_topk: 1 <= n_queries <= 4096");
  ARG_CHECK(ng >= 1 && ng <= nq, "retrieve_topk: 1 <= n_groups <= n_queries (every group needs a query)");
  ARG_CHECK(group != nullptr || ng == nq, "retrieve_topk: without `group`, n_groups must equal n_queries");
  const int Vm = medium == 0 ? m->V0 : m->V1;
  ARG_CHECK(k >= 1 && k <= std::min(Vm, RT_MAXK), "retrieve_topk: 1 <= k <= min(V_m, 8192)");
  return m->bf16_mode ? retrieve_t<bf16>(m, medium, queries, nq, group, ng, prior, excl_off, excl_ids, nullptr, k, ids_out, scores_out, counts_out)
                      : retrieve_t<float>(m, medium, queries, nq, group, ng, prior, excl_off, excl_ids, nullptr, k, ids_out, scores_out, counts_out);
}

// the pipeline of model_retrieve_topk with the group score rows [n_groups][V_m] filled on the device by `init` (called on the model's
// stream after the workspace is in place): the prior and the NaN masks of rsys_retrieve_request.  The caller has checked the arguments
// model_retrieve_topk checks.
int model_retrieve_run(Model* m, int medium, const float* queries, int64_t nq, const int32_t* group, int32_t ng, const RetrieveInit& init,
                       int32_t k, int32_t* ids_out, float* scores_out, int32_t* counts_out, RetrieveDev* dev, const RetrieveWin* win,
                       const float* user_w) {
  return m->bf16_mode ? retrieve_t<bf16>(m, medium, queries, nq, group, ng, nullptr, nullptr, nullptr, &init, k, ids_out, scores_out, counts_out, dev, win, user_w)
                      : retrieve_t<float>(m, medium, queries, nq, group, ng, nullptr, nullptr, nullptr, &init, k, ids_out, scores_out, counts_out, dev, win, user_w);
}

static void topk_rows_layout(Carve& c, int rows, int V, int k, unsigned** keys, SelBufs* sb) {
  const int nb = (V + RT_ITEMS - 1) / RT_ITEMS;
  *keys = c.take<unsigned>((size_t)rows * V);
  sb->hist = c.take<unsigned>((size_t)rows * 256);
  sb->st = c.take<SelState>(rows);
  sb->cnt = c.take<int2>((size_t)rows * nb);
  sb->cand = c.take<unsigned long long>((size_t)rows * k);
  sb->ldc = k;
}

size_t topk_rows_ws_bytes(int rows, int V, int k) {
  Carve probe{nullptr};
  unsigned* keys; SelBufs sb;
  topk_rows_layout(probe, rows, V, k, &keys, &sb);
  return probe.off;
}

int topk_rows(const float* scores, long long ld, int rows, int V, int k, void* ws, int* ids, float* vals, int* counts, hipStream_t s) {
  const int nb = (V + RT_ITEMS - 1) / RT_ITEMS;
  Carve c{(char*)ws};
  unsigned* keys; SelBufs sb;
  topk_rows_layout(c, rows, V, k, &keys, &sb);
  HIP_CHECK(hipMemsetAsync(sb.hist, 0, (size_t)rows * 256 * 4, s));
  combine_kernel<true><<<dim3(nb, rows), RT_THREADS, 0, s>>>(scores, ld, (float*)keys, V, nullptr, 0, nullptr, nullptr, nullptr, 0, V, sb.hist);
  RT_LAUNCH_CHECK();
  return topk_select(keys, V, rows, V, k, sb, ids, vals, counts, s);
}

int op_topk(const float* scores, int64_t ld, int32_t rows, int32_t V, int32_t k, int32_t* ids, float* vals, int32_t* counts) {
  ARG_CHECK(scores && ids && vals && counts, "rsys_op_topk: null buffer");
  ARG_CHECK(rows >= 1 && rows <= 65535 && V >= 1 && ld >= V, "rsys_op_topk: 1 <= rows <= 65535 (grid.y), V >= 1, ld >= V");
  ARG_CHECK(k >= 1 && k <= std::min(V, RT_MAXK), "rsys_op_topk: 1 <= k <= min(V, 8192)");
  void* buf = nullptr;
  HIP_CHECK(hipMalloc(&buf, topk_rows_ws_bytes(rows, V, k)));
  int rc = topk_rows(scores, ld, rows, V, k, buf, ids, vals, counts, nullptr);
  const hipError_t e = hipDeviceSynchronize();
  hipFree(buf);
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("rsys_op_topk: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  return rc;
}

// workspace of rsys_op_topk_window: the keys, the selection buffers of a window (two bounds per row, int4 counts) and the windows
struct WinOpBufs { unsigned* keys; SelBufs sb; long long* wstart; int* wlen; };
static void topk_window_layout(Carve& c, int rows, int V, WinOpBufs* w) {
  const int nb = (V + RT_ITEMS - 1) / RT_ITEMS;
  w->keys = c.take<unsigned>((size_t)rows * V);
  w->sb.hist = c.take<unsigned>((size_t)2 * rows * 256);
  w->sb.st = c.take<SelState>((size_t)2 * rows);
  w->sb.cnt = c.take<int2>((size_t)2 * rows * nb);
  w->sb.cand = c.take<unsigned long long>((size_t)rows * RT_WIN);
  w->sb.ldc = RT_WIN;
  w->wstart = c.take<long long>(rows);
  w->wlen = c.take<int>(rows);
}

// rsys_op_topk_window: the keys of given scores (combine_kernel<true> without queries, as topk_rows) and window_select, on a workspace of
// its own; bounds (device, or null) [rows][2][2] = (T, need) of the end bound and of the start bound as the select left them
int op_topk_window(const float* scores, int64_t ld, int32_t rows, int32_t V, const int64_t* start, const int32_t* len, int32_t* ids,
                   float* vals, int32_t* counts, int32_t* totals, int32_t* bounds) {
  ARG_CHECK(scores && start && len && ids && vals && counts && totals, "rsys_op_topk_window: null buffer");
  ARG_CHECK(rows >= 1 && rows <= 65535 && V >= 1 && ld >= V, "rsys_op_topk_window: 1 <= rows <= 65535 (grid.y), V >= 1, ld >= V");
  for (int r = 0; r < rows; ++r) {
    ARG_CHECK(len[r] >= 1 && len[r] <= RT_WIN, "rsys_op_topk_window: 1 <= len <= 1024");
    ARG_CHECK(start[r] >= 0, "rsys_op_topk_window: start >= 0");
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "window starts are copied as they are");
  Carve probe{nullptr};
  WinOpBufs w;
  topk_window_layout(probe, rows, V, &w);
  void* buf = nullptr;
  HIP_CHECK(hipMalloc(&buf, probe.off));
  Carve c{(char*)buf};
  topk_window_layout(c, rows, V, &w);
  const int nb = (V + RT_ITEMS - 1) / RT_ITEMS;
  std::vector<SelState> st(bounds ? (size_t)2 * rows : 0);
  auto run = [&]() -> int {
    HIP_CHECK(hipMemcpy(w.wstart, start, (size_t)rows * 8, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(w.wlen, len, (size_t)rows * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemsetAsync(w.sb.hist, 0, (size_t)2 * rows * 256 * 4, nullptr));
    combine_kernel<true><<<dim3(nb, rows), RT_THREADS>>>(scores, ld, (float*)w.keys, V, nullptr, 0, nullptr, nullptr, nullptr, 0, V, w.sb.hist);
    RT_LAUNCH_CHECK();
    RC(window_select(w.keys, V, rows, V, w.wstart, w.wlen, w.sb, ids, vals, counts, totals, nullptr));
    if (bounds) {
      HIP_CHECK(hipMemcpy(st.data(), w.sb.st, st.size() * sizeof(SelState), hipMemcpyDeviceToHost));
      std::vector<int32_t> hb((size_t)rows * 4);
      for (int r = 0; r < rows; ++r)
        for (int b = 0; b < 2; ++b) {
          hb[(size_t)r * 4 + 2 * b] = (int32_t)st[(size_t)b * rows + r].prefix;
          hb[(size_t)r * 4 + 2 * b + 1] = st[(size_t)b * rows + r].need;
        }
      HIP_CHECK(hipMemcpy(bounds, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
    }
    return RSYS_OK;
  };
  int rc = run();
  const hipError_t e = hipDeviceSynchronize();
  hipFree(buf);
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("rsys_op_topk_window: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  return rc;
}

// the two log-sum-exp launches of retrieve_chunk_scores on device rows, stream-ordered (rsys_op_lse; the text rows of search.hip)
int lse_rows(const float* z, long long ldz, int rows, int V, float2* part, float* lse, hipStream_t s) {
  lse_partial_kernel<<<dim3(RT_LSE_SPLIT, rows), RT_THREADS, 0, s>>>(z, ldz, V, part);
  if (hipGetLastError() != hipSuccess) { set_error("lse_rows: launch failed (partial)"); return RSYS_ERR_HIP; }
  lse_final_kernel<<<(rows + 255) / 256, 256, 0, s>>>(part, RT_LSE_SPLIT, rows, 0, lse);
  if (hipGetLastError() != hipSuccess) { set_error("lse_rows: launch failed (final)"); return RSYS_ERR_HIP; }
  return RSYS_OK;
}

// rsys_op_lse: lse_rows on device rows
int op_lse(const float* z, int64_t ldz, int32_t rows, int32_t V, float* lse) {
  ARG_CHECK(z && lse, "rsys_op_lse: null buffer");
  ARG_CHECK(rows >= 1 && rows <= 65535 && V >= 1 && ldz >= V, "rsys_op_lse: 1 <= rows <= 65535 (grid.y), V >= 1, ldz >= V");
  float2* part = nullptr;
  HIP_CHECK(hipMalloc(&part, (size_t)rows * RT_LSE_SPLIT * sizeof(float2)));
  int rc = lse_rows(z, ldz, rows, V, part, lse, nullptr);
  const hipError_t e = hipDeviceSynchronize();
  hipFree(part);
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("rsys_op_lse: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  return rc;
}

// the text terms of a request (rsys_query_texts_set) onto the group score rows, in place: combine_w_kernel<false> with the texts' rows as
// its queries (q0 = 0: z, lse and the weights are indexed by row)
int retrieve_text_terms(float* sc, int ng, int V, const QueryTexts& qt, const int32_t* d_members, const int32_t* d_ranges, hipStream_t s) {
  const dim3 grid((unsigned)((V + RT_ITEMS - 1) / RT_ITEMS), (unsigned)ng);
  combine_w_kernel<false><<<grid, RT_THREADS, 0, s>>>(sc, V, sc, V, qt.z, qt.ldz, qt.lse, d_members, (const int2*)d_ranges, 0, V, nullptr, qt.d_w);
  RT_LAUNCH_CHECK();
  return RSYS_OK;
}

// rsys_op_query_weights, the combine section: one launch of combine_w_kernel over device arrays; the first-digit histogram of `last`
// goes to a scratch of its own
int op_combine_weighted(const float* src, float* dst, int32_t ng, int32_t V, int32_t last, const float* z, int64_t ldz, const float* lse,
                        const int32_t* members, const int32_t* ranges, int32_t q0, const float* user_w) {
  ARG_CHECK(src && dst && z && lse && members && ranges && user_w, "rsys_op_query_weights: null buffer (combine)");
  ARG_CHECK(ng >= 1 && ng <= 65535 && V >= 1 && ldz >= V && q0 >= 0, "rsys_op_query_weights: 1 <= n_groups <= 65535, V >= 1, ldz >= V, q0 >= 0");
  unsigned* hist = nullptr;
  HIP_CHECK(hipMalloc(&hist, (size_t)ng * 256 * 4));
  int rc = RSYS_OK;
  if (hipMemset(hist, 0, (size_t)ng * 256 * 4) != hipSuccess) rc = RSYS_ERR_HIP;
  if (rc == RSYS_OK) {
    const dim3 grid((unsigned)((V + RT_ITEMS - 1) / RT_ITEMS), (unsigned)ng);
    if (last) combine_w_kernel<true><<<grid, RT_THREADS>>>(src, V, dst, V, z, ldz, lse, members, (const int2*)ranges, q0, V, hist, user_w);
    else combine_w_kernel<false><<<grid, RT_THREADS>>>(src, V, dst, V, z, ldz, lse, members, (const int2*)ranges, q0, V, hist, user_w);
    if (hipGetLastError() != hipSuccess) { set_error("rsys_op_query_weights: launch failed (combine)"); rc = RSYS_ERR_HIP; }
  }
  const hipError_t e = hipDeviceSynchronize();
  hipFree(hist);
  if (rc == RSYS_OK && e != hipSuccess) { set_error(std::string("rsys_op_query_weights: ") + hipGetErrorString(e)); rc = RSYS_ERR_HIP; }
  return rc;
}

}  // namespace rsys
