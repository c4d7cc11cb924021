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

__global__ void eval_scatter_nan_kernel(float* z, const long long* pos, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) z[pos[i]] = __int_as_float(0x7fc00000);
}

struct Carve {
  char* p; size_t off = 0;
  template <typename X> X* take(size_t count) {
    X* r = (X*)(p ? p + off : nullptr);
    off += (std::max<size_t>(count, 1) * sizeof(X) + 255) / 256 * 256;
    return r;
  }
};

}  // namespace

// rsys_retrieve_target_rank's workspace: one device buffer, grown on demand, freed with the model
struct EvalWs {
  void* buf = nullptr;
  size_t bytes = 0;
};

void retrieve_eval_free(Model* m) {
  if (!m->ews) return;
  if (m->ews->buf) hipFree(m->ews->buf);
  delete m->ews;
  m->ews = nullptr;
}

template <typename T>
static int target_rank_t(Model* m, int medium, const float* queries, int64_t nq, const int32_t* targets, const std::vector<long long>& xpos,
                         const std::vector<long long>& xcoff, int32_t* rank_out, float* logp_out) {
  const int D = m->D, Vm = medium == 0 ? m->V0 : m->V1, vs = medium == 0 ? 0 : m->V0;
  hipStream_t s = m->stream;
  const long long ldz = pad8(std::max(m->V0, m->V1));   // (the slab stride of rsys_retrieve_topk: the same GEMM launch)
  const int nchunks = (int)((nq + RETRIEVE_CHUNK - 1) / RETRIEVE_CHUNK);
  auto layout = [&](Carve& c, float** qf, T** qt, float** lse, float2** part, float** z, int** d_tgt, int** d_rank, float** d_logp,
                    long long** d_xpos) {
    *qf = c.take<float>((size_t)nq * D);
    *qt = is_bf16<T>::value ? c.take<T>((size_t)nq * D) : (T*)*qf;
    *lse = c.take<float>(nq);
    *part = c.take<float2>((size_t)RETRIEVE_CHUNK * RETRIEVE_LSE_SPLIT);
    *z = c.take<float>((size_t)std::min<int64_t>(nq, RETRIEVE_CHUNK) * ldz);
    *d_tgt = c.take<int>(nq);
    *d_rank = c.take<int>(nq);
    *d_logp = c.take<float>(nq);
    *d_xpos = c.take<long long>(xpos.size());
  };
  float *qf, *lse, *z, *d_logp; T* qt; float2* part; int *d_tgt, *d_rank; long long* d_xpos;
  Carve probe{nullptr};
  layout(probe, &qf, &qt, &lse, &part, &z, &d_tgt, &d_rank, &d_logp, &d_xpos);
  HIP_CHECK(hipSetDevice(m->device));
  if (!m->ews) m->ews = new EvalWs();
  EvalWs* ws = m->ews;
  if (ws->bytes < probe.off) {
    HIP_CHECK(hipStreamSynchronize(s));
    if (ws->buf) HIP_CHECK(hipFree(ws->buf));
    ws->buf = nullptr; ws->bytes = 0;
    HIP_CHECK(hipMalloc(&ws->buf, probe.off));
    ws->bytes = probe.off;
  }
  Carve c{(char*)ws->buf};
  layout(c, &qf, &qt, &lse, &part, &z, &d_tgt, &d_rank, &d_logp, &d_xpos);
  if (m->table_dirty) { RC(table_forward<T>(m)); m->table_dirty = false; }

  tic(m, "eval_prep");
  HIP_CHECK(hipMemcpyAsync(qf, queries, (size_t)nq * D * 4, hipMemcpyHostToDevice, s));
  if constexpr (is_bf16<T>::value) RC(launch_cast<T>(qf, qt, (long long)nq * D, s));
  HIP_CHECK(hipMemcpyAsync(d_tgt, targets, (size_t)nq * 4, hipMemcpyHostToDevice, s));
  if (!xpos.empty()) HIP_CHECK(hipMemcpyAsync(d_xpos, xpos.data(), xpos.size() * 8, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemsetAsync(d_rank, 0, (size_t)nq * 4, s));
  toc(m);
  const T* Fm = AT<T>(m->FT) + (int64_t)vs * D;
  const int nb = (Vm + RE_ITEMS - 1) / RE_ITEMS;
  for (int ch = 0; ch < nchunks; ++ch) {
    const int q0 = ch * RETRIEVE_CHUNK, nc = (int)std::min<int64_t>(RETRIEVE_CHUNK, nq - q0);
    RC(retrieve_chunk_scores<T>(m, qt + (size_t)q0 * D, nc, q0, Fm, Vm, z, ldz, part, lse));
    tic(m, "eval_logp");
    target_logp_kernel<<<(nc + 255) / 256, 256, 0, s>>>(z, ldz, nc, lse, d_tgt, q0, d_logp);
    HIP_CHECK(hipGetLastError());
    const long long nx = xcoff[ch + 1] - xcoff[ch];
    if (nx) {
      eval_scatter_nan_kernel<<<(unsigned)((nx + 255) / 256), 256, 0, s>>>(z, d_xpos + xcoff[ch], nx);
      HIP_CHECK(hipGetLastError());
    }
    toc(m);
    tic(m, "eval_count");
    target_count_kernel<true, true><<<dim3(nb, nc), RE_THREADS, 0, s>>>(z, ldz, Vm, lse, d_tgt, q0, d_rank);
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
  ARG_CHECK((excl_off == nullptr) == (excl_ids == nullptr), "retrieve_target_rank: excl_offsets and excl_ids are both given or both NULL");
  const int Vm = medium == 0 ? m->V0 : m->V1;
  for (int64_t q = 0; q < nq; ++q) ARG_CHECK(targets[q] >= 0 && targets[q] < Vm, "retrieve_target_rank: targets must be in [0, V_m)");
  // exclusion positions in the score slab of their chunk: (q - q0) * ldz + id, in query order; xcoff[ch] = first of chunk ch
  const long long ldz = pad8(std::max(m->V0, m->V1));
  const int nchunks = (int)((nq + RETRIEVE_CHUNK - 1) / RETRIEVE_CHUNK);
  std::vector<long long> xpos, xcoff(nchunks + 1, 0);
  if (excl_off) {
    ARG_CHECK(excl_off[0] == 0, "retrieve_target_rank: excl_offsets[0] must be 0");
    for (int64_t q = 0; q < nq; ++q) {
      ARG_CHECK(excl_off[q + 1] >= excl_off[q], "retrieve_target_rank: excl_offsets must be non-decreasing");
      for (int64_t j = excl_off[q]; j < excl_off[q + 1]; ++j) {
        ARG_CHECK(excl_ids[j] >= 0 && excl_ids[j] < Vm, "retrieve_target_rank: exclusion ids must be medium-local, in [0, V_m)");
        xpos.push_back((q % RETRIEVE_CHUNK) * ldz + excl_ids[j]);
      }
      if ((q + 1) % RETRIEVE_CHUNK == 0 || q + 1 == nq) xcoff[q / RETRIEVE_CHUNK + 1] = (long long)xpos.size();
    }
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
