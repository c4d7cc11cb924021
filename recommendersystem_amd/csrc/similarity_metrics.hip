// Item-similarity catalogue ranks on the device (Training/item_similarity/pairwise_metrics.jl:72-97, 172-174): for every test source
// the rank of each of its targets among ALL other items of the medium, under the scores v[s][i] = (E E^T)[s][i] * testmask[s][i] and the
// order of Julia's sortperm(..., rev = true).  nDCG@k and Recall@k are functions of those ranks alone (similarity.py), so nothing else
// leaves the device.  Per chunk of 256 sources:
//   rows     the chunk's rows of the fp32 export, gathered
//   scores   g = rows . export^T through launch_gemm<float> (v_mfma_f32_16x16x4_f32: fp32 operands, fp32 accumulation, a fixed order)
//            into a [256][V] slab.  The test mask is NOT applied to the slab: prep and count apply it to what they load (one bit word
//            per 16-byte load), which saves a read and a write of the slab per chunk.
//   prep     one workgroup per source: the composite keys (isless_key(v_t) << 32 | ~t) of its targets, sorted ascending in LDS in
//            batches of PR_TB with their output slots (bitonic sort, as sim_rank_kernel); a target's rank starts at 1 (0 for t == s)
//   count    grid = item blocks x sources.  A workgroup turns its 4096 items of the row into composite keys held in registers, and per
//            target batch stages the sorted target keys in LDS, finds by binary search the number p of targets each candidate sorts
//            before (a candidate sorts before a target iff its composite key is larger: a larger score, or the same score and a smaller
//            id), and adds 1 to LDS bin p (one add per wave for the lanes that agree with its first lane).  The suffix sum of the bins
//            is every target's count, added to rank[slot] with one integer atomic.  Integer sums do not depend on order: the result is
//            bitwise reproducible.  The row is read once however many targets or batches it has.
// Everything runs on the handle's stream; the host waits once, after the copy out.
#include <algorithm>
#include <vector>

#include "encoder_handle.hpp"

namespace rsys {

namespace {

typedef unsigned long long u64;

constexpr int PR_THREADS = 256;
constexpr int PR_UNROLL = 4;                                   // float4 loads per thread
constexpr int PR_ITEMS = PR_THREADS * 4 * PR_UNROLL;           // items per workgroup of the count pass
constexpr int PR_TB = 1024;                                    // targets per LDS staging (8 KB of keys, 4 KB of bins)
constexpr int PR_SORT_THREADS = 512;
constexpr int PR_CHUNK = 256;                                  // sources per score GEMM

// M .* testmask with the Int8 mask (pairwise_dataset.jl:288): an IEEE product, so a masked zero keeps g's sign and a non-finite g is NaN
__device__ __forceinline__ float masked_score(float g, unsigned word, int i) { return ((word >> (i & 31)) & 1u) ? g : g * 0.0f; }

__device__ __forceinline__ u64 composite_key(float v, int i) { return ((u64)isless_key(v) << 32) | (u64)(0xffffffffu - (unsigned)i); }

__global__ void pair_rows_kernel(const float* __restrict__ tab, int E, const int* __restrict__ ids, int rows, float* __restrict__ out) {
  const long long n4 = (long long)rows * E / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const long long e = 4 * i, r = e / E;
    const int c = (int)(e - r * E);
    *(float4*)(out + e) = *(const float4*)(tab + (long long)ids[r] * E + c);
  }
}

// z[row][i] = masked_score(z[row][i]) in place (the debug read-back of the masked rows; the ranking applies the mask on load)
__global__ void __launch_bounds__(256) pair_mask_kernel(float* z, long long ldz, int V, const int* __restrict__ self,
                                                        const unsigned* __restrict__ tmask, long long tmw) {
  const int row = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= V) return;
  float* p = z + row * ldz + i;
  *p = masked_score(*p, tmask[self[row] * tmw + (i >> 5)], i);
}

// per source row (blockIdx.x; its targets are tid[off[row] .. off[row + 1])): rank = 1 (0 where the target is the source itself), and
// per batch of PR_TB targets the composite keys sorted ascending (skeys) with the rank slot of each (sslot, -1 for the source itself)
template <bool MASK>
__global__ void __launch_bounds__(PR_SORT_THREADS) pair_prep_kernel(const float* __restrict__ z, long long ldz, const int* __restrict__ self,
                                                                    const unsigned* __restrict__ tmask, long long tmw,
                                                                    const long long* __restrict__ off, const int* __restrict__ tid,
                                                                    u64* __restrict__ skeys, int* __restrict__ sslot, int* __restrict__ rank) {
  const int row = blockIdx.x, s = self[row];
  const long long b = off[row], e = off[row + 1];
  const float* zr = z + row * ldz;
  __shared__ u64 k[PR_TB];
  __shared__ int sl[PR_TB];
  for (long long b0 = b; b0 < e; b0 += PR_TB) {
    const int n = (int)(e - b0 < PR_TB ? e - b0 : PR_TB);
    int N2 = 1;
    while (N2 < n) N2 <<= 1;
    for (int i = threadIdx.x; i < N2; i += PR_SORT_THREADS) {
      u64 key = ~0ull;
      int slot = -1;
      if (i < n) {
        const int t = tid[b0 + i];
        const float g = zr[t];
        key = composite_key(MASK ? masked_score(g, tmask[s * tmw + (t >> 5)], t) : g, t);
        slot = t == s ? -1 : (int)(b0 + i);
        rank[b0 + i] = t == s ? 0 : 1;
      }
      k[i] = key; sl[i] = slot;
    }
    __syncthreads();
    for (int size = 2; size <= N2; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = threadIdx.x; i < N2 / 2; i += PR_SORT_THREADS) {
          const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
          const bool asc = (lo & size) == 0;
          const u64 a = k[lo], c = k[hi];
          if ((a > c) == asc) {
            k[lo] = c; k[hi] = a;
            const int t = sl[lo]; sl[lo] = sl[hi]; sl[hi] = t;
          }
        }
        __syncthreads();
      }
    }
    for (int i = threadIdx.x; i < n; i += PR_SORT_THREADS) { skeys[b0 + i] = k[i]; sslot[b0 + i] = sl[i]; }
    __syncthreads();
  }
}

// rank[slot] += #{candidates i != self of this workgroup's PR_ITEMS items whose composite key is above the target's}, for every target
// of row blockIdx.y.  VEC: 16-byte loads (ldz % 4 == 0, aligned base).  An item outside [0, V) or equal to self gets composite key 0, which
// is below every target's and lands in bin 0, the bin no target reads.
template <bool MASK, bool VEC>
__global__ void __launch_bounds__(PR_THREADS) pair_count_kernel(const float* __restrict__ z, long long ldz, int V, const int* __restrict__ self,
                                                                const unsigned* __restrict__ tmask, long long tmw,
                                                                const long long* __restrict__ off, const u64* __restrict__ skeys,
                                                                const int* __restrict__ sslot, int* rank) {
  const int row = blockIdx.y;
  const long long b = off[row], e = off[row + 1];
  if (b == e) return;
  const int s = self[row];
  const float* zr = z + row * ldz;
  const unsigned* mr = MASK ? tmask + s * tmw : nullptr;
  __shared__ u64 keys[PR_TB];
  __shared__ __attribute__((aligned(16))) int bins[PR_TB + 4];
  __shared__ int wtot[PR_THREADS / 64];
  u64 c[4 * PR_UNROLL];
  const int base = blockIdx.x * PR_ITEMS;
#pragma unroll
  for (int u = 0; u < PR_UNROLL; ++u) {
    const int i = base + 4 * (u * PR_THREADS + (int)threadIdx.x);
    if (VEC && i + 4 <= V) {
      const float4 v = *reinterpret_cast<const float4*>(zr + i);
      const unsigned w = MASK ? mr[i >> 5] : 0u;
      const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) c[4 * u + j] = i + j == s ? 0ull : composite_key(MASK ? masked_score(f[j], w, i + j) : f[j], i + j);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        u64 ck = 0ull;
        if (i + j < V && i + j != s) {
          const float g = zr[i + j];
          ck = composite_key(MASK ? masked_score(g, mr[(i + j) >> 5], i + j) : g, i + j);
        }
        c[4 * u + j] = ck;
      }
    }
  }
  const int lane = lane_id(), w = threadIdx.x >> 6;
  for (long long b0 = b; b0 < e; b0 += PR_TB) {
    const int n = (int)(e - b0 < PR_TB ? e - b0 : PR_TB);
    int N2 = 1;
    while (N2 < n) N2 <<= 1;
    for (int i = threadIdx.x; i < N2; i += PR_THREADS) keys[i] = i < n ? skeys[b0 + i] : ~0ull;
    for (int i = threadIdx.x; i < PR_TB + 4; i += PR_THREADS) bins[i] = 0;
    __syncthreads();
    const u64 kmin = keys[0], kmax = keys[n - 1];
#pragma unroll
    for (int q = 0; q < 4 * PR_UNROLL; ++q) {
      const u64 ck = c[q];
      // p = #{targets of the batch with a key below ck}: 0 at or below the smallest, n above the largest, else a binary search over the N2
      // staged keys (the padding is the largest key, never below ck)
      const bool below = ck <= kmin, above = ck > kmax;
      int p = above ? n : 0;
      if (__ballot(!(below || above)) != 0ull) {
        int lo = 0;
        for (int step = N2 >> 1; step > 0; step >>= 1)
          if (keys[lo + step - 1] < ck) lo += step;
        if (lo == N2 - 1 && keys[N2 - 1] < ck) ++lo;
        if (!(below || above)) p = lo;
      }
      // one LDS add per wave for the lanes that agree with lane 0 (nearly the whole wave: the masked zeros of a row share a bin)
      const int p0 = __builtin_amdgcn_readfirstlane(p);
      const u64 agree = __ballot(p == p0);
      if (lane == 0) { if (p0 != 0) atomicAdd(&bins[p0], __popcll(agree)); }
      else if (p != p0 && p != 0) atomicAdd(&bins[p], 1);
    }
    __syncthreads();
    // count of target j = sum of bins p > j: thread t owns bins 4t .. 4t + 3, a suffix sum over lanes, waves, and the last bin
    const int4 own = *reinterpret_cast<const int4*>(&bins[4 * threadIdx.x]);
    const int tot = own.x + own.y + own.z + own.w;
    int v = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_down(v, o, 64);
      if (lane + o < 64) v += x;
    }
    if (lane == 0) wtot[w] = v;
    __syncthreads();
    int hi = bins[PR_TB];
    for (int ww = w + 1; ww < PR_THREADS / 64; ++ww) hi += wtot[ww];
    const int a3 = v - tot + hi, a2 = a3 + own.w, a1 = a2 + own.z, a0 = a1 + own.y;
    const int cnt[4] = {a0, a1, a2, a3};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * threadIdx.x + q;
      if (j < n && cnt[q] != 0) {
        const int slot = sslot[b0 + j];
        if (slot >= 0) atomicAdd(rank + slot, cnt[q]);
      }
    }
    __syncthreads();
  }
}

// the device arrays of one call
struct PairBufs {
  float *A, *z;
  int *src, *tid, *rank, *sslot;
  long long* off;
  u64* skeys;
  void take(Carve& c, int n_src, long long total, int C, int E, long long ldz, bool scores) {
    A = c.take<float>(scores ? (size_t)C * E : 0);
    z = c.take<float>(scores ? (size_t)C * ldz : 0);
    src = c.take<int>(n_src);
    off = c.take<long long>((size_t)n_src + 1);
    tid = c.take<int>(total);
    rank = c.take<int>(total);
    sslot = c.take<int>(total);
    skeys = c.take<u64>(total);
  }
};

int pair_check_csr(const char* who, int V, int32_t n_rows, const int32_t* self, const int64_t* off, const int32_t* tids) {
  ARG_CHECK(self && off, std::string(who) + ": null buffer");
  ARG_CHECK(n_rows >= 1, std::string(who) + ": at least one row");
  ARG_CHECK(off[0] == 0, std::string(who) + ": tgt_offsets[0] must be 0");
  for (int r = 0; r < n_rows; ++r) {
    ARG_CHECK(self[r] >= 0 && self[r] < V, std::string(who) + ": source ids must be in [0, V)");
    ARG_CHECK(off[r + 1] >= off[r], std::string(who) + ": tgt_offsets must be non-decreasing");
  }
  ARG_CHECK(off[n_rows] <= 0x7fffffffLL, std::string(who) + ": at most 2^31 - 1 targets per call");
  ARG_CHECK(off[n_rows] == 0 || tids, std::string(who) + ": null target ids");
  for (int64_t j = 0; j < off[n_rows]; ++j) ARG_CHECK(tids[j] >= 0 && tids[j] < V, std::string(who) + ": target ids must be in [0, V)");
  return RSYS_OK;
}

// prep + count of rows [r0, r0 + nc) over their score rows z [nc][ldz]
template <bool MASK>
int pair_count_rows(const float* z, long long ldz, int V, int r0, int nc, const unsigned* tmask, long long tmw, const PairBufs& b,
                    hipStream_t s) {
  pair_prep_kernel<MASK><<<nc, PR_SORT_THREADS, 0, s>>>(z, ldz, b.src + r0, tmask, tmw, b.off + r0, b.tid, b.skeys, b.sslot, b.rank);
  HIP_CHECK(hipGetLastError());
  const dim3 grid((V + PR_ITEMS - 1) / PR_ITEMS, nc);
  if (ldz % 4 == 0 && ((uintptr_t)z & 15) == 0)
    pair_count_kernel<MASK, true><<<grid, PR_THREADS, 0, s>>>(z, ldz, V, b.src + r0, tmask, tmw, b.off + r0, b.skeys, b.sslot, b.rank);
  else
    pair_count_kernel<MASK, false><<<grid, PR_THREADS, 0, s>>>(z, ldz, V, b.src + r0, tmask, tmw, b.off + r0, b.skeys, b.sslot, b.rank);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

// g = rows(sources[c0 .. c0 + nc)) . export^T into b.z
int pair_chunk_scores(const float* exp32, int V, int E, int c0, int nc, long long ldz, const PairBufs& b, hipStream_t s) {
  pair_rows_kernel<<<grid_for((long long)nc * E / 4), 256, 0, s>>>(exp32, E, b.src + c0, nc, b.A);
  HIP_CHECK(hipGetLastError());
  GemmParams p{};
  p.A = b.A; p.lda = E; p.B = exp32; p.ldb = E; p.C = b.z; p.ldc = ldz; p.c_f32 = 1;
  p.M = nc; p.N = V; p.K = E; p.epi = EPI_STORE; p.alpha = 1.f; p.splitk = 1;
  return launch_gemm<float>(p, false, false, false, false, s);
}

}  // namespace

int pair_ranks_run(const float* exp32, int V, int E, const unsigned* tmask, long long tmw, int32_t n_src, const int32_t* sources,
                   const int64_t* off, const int32_t* tids, int32_t* ranks_out, DevScratch* ws, hipStream_t s) {
  ARG_CHECK(ranks_out, "rsys_sim_pair_ranks: null output");
  if (int rc = pair_check_csr("rsys_sim_pair_ranks", V, n_src, sources, off, tids)) return rc;
  const long long total = off[n_src];
  if (total == 0) return RSYS_OK;
  const int C = std::min<int>(n_src, PR_CHUNK);
  const long long ldz = (V + 7) / 8 * 8;
  PairBufs b;
  if (int rc = carve_into(*ws, s, [&](Carve& c) { b.take(c, n_src, total, C, E, ldz, true); })) return rc;
  HIP_CHECK(hipMemcpyAsync(b.src, sources, (size_t)n_src * 4, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b.off, off, ((size_t)n_src + 1) * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(b.tid, tids, (size_t)total * 4, hipMemcpyHostToDevice, s));
  for (int c0 = 0; c0 < n_src; c0 += PR_CHUNK) {
    const int nc = std::min(PR_CHUNK, n_src - c0);
    if (off[c0 + nc] == off[c0]) continue;
    if (int rc = pair_chunk_scores(exp32, V, E, c0, nc, ldz, b, s)) return rc;
    if (int rc = pair_count_rows<true>(b.z, ldz, V, c0, nc, tmask, tmw, b, s)) return rc;
  }
  HIP_CHECK(hipMemcpyAsync(ranks_out, b.rank, (size_t)total * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

int pair_scores_run(const float* exp32, int V, int E, const unsigned* tmask, long long tmw, int32_t n_src, const int32_t* sources,
                    float* out, DevScratch* ws, hipStream_t s) {
  ARG_CHECK(sources && out && n_src >= 1, "rsys_sim_pair_scores: null buffer or no source");
  for (int i = 0; i < n_src; ++i) ARG_CHECK(sources[i] >= 0 && sources[i] < V, "rsys_sim_pair_scores: source ids must be in [0, V)");
  const int C = std::min<int>(n_src, PR_CHUNK);
  const long long ldz = (V + 7) / 8 * 8;
  PairBufs b;
  if (int rc = carve_into(*ws, s, [&](Carve& c) { b.take(c, n_src, 0, C, E, ldz, true); })) return rc;
  HIP_CHECK(hipMemcpyAsync(b.src, sources, (size_t)n_src * 4, hipMemcpyHostToDevice, s));
  for (int c0 = 0; c0 < n_src; c0 += PR_CHUNK) {
    const int nc = std::min(PR_CHUNK, n_src - c0);
    if (int rc = pair_chunk_scores(exp32, V, E, c0, nc, ldz, b, s)) return rc;
    pair_mask_kernel<<<dim3((V + 255) / 256, nc), 256, 0, s>>>(b.z, ldz, V, b.src + c0, tmask, tmw);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpy2DAsync(out + (size_t)c0 * V, (size_t)V * 4, b.z, (size_t)ldz * 4, (size_t)V * 4, nc, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

int op_pair_ranks(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* self, const int64_t* off, const int32_t* tids,
                  int32_t* ranks_out) {
  ARG_CHECK(scores && ranks_out, "rsys_op_pair_ranks: null buffer");
  ARG_CHECK(rows >= 1 && rows <= 65535 && V >= 1 && ld >= V, "rsys_op_pair_ranks: 1 <= rows <= 65535, V >= 1, ld >= V");
  if (int rc = pair_check_csr("rsys_op_pair_ranks", V, rows, self, off, tids)) return rc;
  const long long total = off[rows];
  if (total == 0) return RSYS_OK;
  DevScratch ws;
  PairBufs b;
  if (int rc = carve_into(ws, nullptr, [&](Carve& c) { b.take(c, rows, total, 0, 0, 0, false); })) return rc;
  const int rc = [&]() -> int {
    HIP_CHECK(hipMemcpy(b.src, self, (size_t)rows * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(b.off, off, ((size_t)rows + 1) * 8, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(b.tid, tids, (size_t)total * 4, hipMemcpyHostToDevice));
    if (int r = pair_count_rows<false>(scores, ld, V, 0, rows, nullptr, 0, b, nullptr)) return r;
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(ranks_out, b.rank, (size_t)total * 4, hipMemcpyDeviceToHost));
    return RSYS_OK;
  }();
  ws.release();
  return rc;
}

}  // namespace rsys
