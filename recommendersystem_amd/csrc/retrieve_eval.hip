// Finetune evaluation on the device (Finetune/regress.jl:193-266, `retrieval_metrics` and `regress_retrieval`): per held-out user the rank
// of one given item among every admissible item of the medium, and that item's log-probability.  HR@k and nDCG@k of one relevant item
// are functions of that rank alone, the cross-entropy of the log-probability, so nothing else leaves the device.  The kernels
// (DESIGN.md section 4o):
//   scores     retrieve.hip's gemm_retrieve and log-sum-exp over the whole item table (retrieve_chunk_scores, chunks of 256 queries)
//   logp       one thread per query row: logp[q] = z_q[t_q] - lse_q, read before any exclusion
//   exclude    the chunk's exclusion positions become NaN in the score slab
//   count      grid = item blocks x query rows; a workgroup streams 4096 items of its row with 16-byte loads, counts the items that sort
//              before the target (key above the target's, or equal with a smaller id), sums over lanes and waves, and adds the sum to
//              rank[q] with one integer atomic (block 0 also adds the 1 of a 1-based rank).  Integer sums do not depend on order, so
//              the result is bitwise reproducible; a target that is excluded, -inf or NaN has key 0 and nothing adds to its rank.
// Every launch covers the whole chunk; everything runs on the model's stream; the host waits once, after the copy out.
#include "model_internal.hpp"

namespace rsys {

namespace {

constexpr int RE_THREADS = 256;
constexpr int RE_UNROLL = 4;                                   // float4 loads per thread
constexpr int RE_ITEMS = RE_THREADS * 4 * RE_UNROLL;           // items per workgroup of the count pass
constexpr int RE_MAXQ = 4096;

// 1 if item i (key k) sorts before the target (key kt != 0, id t) in descending-key, ascending-id order
__device__ __forceinline__ int before(unsigned k, long long i, unsigned kt, int t) { return (k > kt || (k == kt && i < t)) ? 1 : 0; }

// rank[q0 + row] += #{i < V : item i of row `row` sorts before the row's target} (+1 from block 0), nothing when the target's key is 0.
// Scores are z - lse[q] (LSE) or z itself.  VEC: 16-byte loads, which needs a 16-byte aligned row start (ldz % 4 == 0, aligned base).
template <bool LSE, bool VEC>
__global__ void __launch_bounds__(RE_THREADS) target_count_kernel(const float* z, long long ldz, int V, const float* lse,
                                                                  const int* targets, int q0, int* rank) {
  const int row = blockIdx.y, q = q0 + row;
  const float* zr = z + row * ldz;
  const int t = targets[q];
  const float l = LSE ? lse[q] : 0.f;
  const unsigned kt = score_key(LSE ? zr[t] - l : zr[t]);
  if (kt == 0u) return;
  int c = 0;
  const long long base = (long long)blockIdx.x * RE_ITEMS;
#pragma unroll
  for (int u = 0; u < RE_UNROLL; ++u) {
    const long long i = base + 4ll * (u * RE_THREADS + threadIdx.x);
    if (VEC && i + 4 <= V) {
      const float4 v = *reinterpret_cast<const float4*>(zr + i);
      c += before(score_key(LSE ? v.x - l : v.x), i, kt, t);
      c += before(score_key(LSE ? v.y - l : v.y), i + 1, kt, t);
      c += before(score_key(LSE ? v.z - l : v.z), i + 2, kt, t);
      c += before(score_key(LSE ? v.w - l : v.w), i + 3, kt, t);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i + j < V) c += before(score_key(LSE ? zr[i + j] - l : zr[i + j]), i + j, kt, t);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  __shared__ int sm[RE_THREADS / 64];
  if (lane_id() == 0) sm[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = blockIdx.x == 0 ? 1 : 0;
    for (int w = 0; w < RE_THREADS / 64; ++w) s += sm[w];
    if (s) atomicAdd(rank + q, s);
  }
}

// logp[q0 + row] = z[row][t] - lse[q0 + row] for the nc rows of a chunk
__global__ void target_logp_kernel(const float* z, long long ldz, int nc, const float* lse, const int* targets, int q0, float* logp) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nc) return;
  const int q = q0 + row;
  logp[q] = z[row * ldz + targets[q]] - lse[q];
}

}  // namespace

template <typename T>
static int target_rank_t(Model* m, int medium, const float* queries, int64_t nq, const int32_t* targets, const std::vector<long long>& xpos,
                         const std::vector<long long>& xcoff, int32_t* rank_out, float* logp_out) {
  const int Vm = medium == 0 ? m->V0 : m->V1;
  hipStream_t s = m->stream;
  const int nchunks = (int)((nq + RETRIEVE_CHUNK - 1) / RETRIEVE_CHUNK);
  ScoreBufs<T> b(m);   // (the slab stride of rsys_retrieve_topk: the same GEMM launch)
  int *d_tgt, *d_rank; float* d_logp; long long* d_xpos;
  HIP_CHECK(hipSetDevice(m->device));
  RC(carve_into(m->ews, s, [&](Carve& c) {
    b.take(c, nq);
    d_tgt = c.take<int>(nq);
    d_rank = c.take<int>(nq);
    d_logp = c.take<float>(nq);
    d_xpos = c.take<long long>(xpos.size());
  }));
  const T* Fm;
  RC(score_table_ready<T>(m, medium, &Fm));

  tic(m, "eval_prep");
  RC(score_upload_queries(b, queries, nq, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_tgt, targets, (size_t)nq * 4, hipMemcpyHostToDevice, s));
  if (!xpos.empty()) HIP_CHECK(hipMemcpyAsync(d_xpos, xpos.data(), xpos.size() * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(d_rank, 0, (size_t)nq * 4, s));
  toc(m);
  const int nb = (Vm + RE_ITEMS - 1) / RE_ITEMS;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int q0 = ch * RETRIEVE_CHUNK, nc = (int)std::min<int64_t>(RETRIEVE_CHUNK, nq - q0);
    RC(retrieve_chunk_scores<T>(m, b.qt + (size_t)q0 * b.D, nc, q0, Fm, Vm, b.z, b.ldz, b.part, b.lse));
    tic(m, "eval_logp");
    target_logp_kernel<<<(nc + 255) / 256, 256, 0, s>>>(b.z, b.ldz, nc, b.lse, d_tgt, q0, d_logp);
    HIP_CHECK(hipGetLastError());
    const long long nx = xcoff[ch + 1] - xcoff[ch];
    if (nx) RC(launch_scatter_nan(b.z, d_xpos + xcoff[ch], nx, s));
    toc(m);
    tic(m, "eval_count");
    target_count_kernel<true, true><<<dim3(nb, nc), RE_THREADS, 0, s>>>(b.z, b.ldz, Vm, b.lse, d_tgt, q0, d_rank);
    HIP_CHECK(hipGetLastError());
    toc(m);
  }
  HIP_CHECK(hipMemcpyAsync(rank_out, d_rank, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(logp_out, d_logp, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return RSYS_OK;
}

int model_retrieve_target_rank(Model* m, int medium, const float* queries, int64_t nq, const int32_t* targets, const int64_t* excl_off,
                               const int32_t* excl_ids, int32_t* rank_out, float* logp_out) {
  ARG_CHECK(medium == 0 || medium == 1, "retrieve_target_rank: medium must be 0 or 1");
  ARG_CHECK(!m->sharded, "retrieve_target_rank: the row-sharded item table is not supported (replicated table only)");
  ARG_CHECK(queries && targets && rank_out && logp_out, "retrieve_target_rank: null buffer");
  ARG_CHECK(nq >= 1 && nq <= RE_MAXQ, "retrieve_target_rank: 1 <= n_queries <= 4096");
  RC(check_ragged("retrieve_target_rank", LIST_EXCLUDED, excl_off, nq, {excl_ids}));
  const int Vm = medium == 0 ? m->V0 : m->V1;
  for (int64_t q = 0; q < nq; ++q) ARG_CHECK(targets[q] >= 0 && targets[q] < Vm, "retrieve_target_rank: targets must be in [0, V_m)");
  // exclusion positions in the score slab of their chunk: (q - q0) * ldz + id, in query order; xcoff[ch] = first of chunk ch
  const long long ldz = score_ldz(m);
  const int nchunks = (int)((nq + RETRIEVE_CHUNK - 1) / RETRIEVE_CHUNK);
  std::vector<long long> xpos, xcoff(nchunks + 1, 0);
  RC(check_list_items("retrieve_target_rank", LIST_EXCLUDED, excl_off, nq, nullptr, excl_ids, &Vm));
  if (excl_off)
    for (int64_t q = 0; q < nq; ++q) {
      for (int64_t j = excl_off[q]; j < excl_off[q + 1]; ++j) xpos.push_back((q % RETRIEVE_CHUNK) * ldz + excl_ids[j]);
      if ((q + 1) % RETRIEVE_CHUNK == 0 || q + 1 == nq) xcoff[q / RETRIEVE_CHUNK + 1] = (long long)xpos.size();
    }
  return m->bf16_mode ? target_rank_t<bf16>(m, medium, queries, nq, targets, xpos, xcoff, rank_out, logp_out)
                      : target_rank_t<float>(m, medium, queries, nq, targets, xpos, xcoff, rank_out, logp_out);
}

int op_target_rank(const float* scores, int64_t ld, int32_t rows, int32_t V, const int32_t* targets, int32_t* rank_out) {
  ARG_CHECK(scores && targets && rank_out, "rsys_op_target_rank: null buffer");
  ARG_CHECK(rows >= 1 && rows <= 65535 && V >= 1 && ld >= V, "rsys_op_target_rank: 1 <= rows <= 65535, V >= 1, ld >= V");
  std::vector<int32_t> t(rows);
  HIP_CHECK(hipMemcpy(t.data(), targets, (size_t)rows * 4, hipMemcpyDeviceToHost));
  for (int r = 0; r < rows; ++r) ARG_CHECK(t[r] >= 0 && t[r] < V, "rsys_op_target_rank: targets must be in [0, V)");
  HIP_CHECK(hipMemset(rank_out, 0, (size_t)rows * 4));
  const dim3 grid((V + RE_ITEMS - 1) / RE_ITEMS, rows);
  if (ld % 4 == 0 && ((uintptr_t)scores & 15) == 0)
    target_count_kernel<false, true><<<grid, RE_THREADS>>>(scores, ld, V, nullptr, targets, 0, rank_out);
  else
    target_count_kernel<false, false><<<grid, RE_THREADS>>>(scores, ld, V, nullptr, targets, 0, rank_out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  return RSYS_OK;
}

}  // namespace rsys
