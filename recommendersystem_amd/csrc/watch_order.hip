// Watch-order counts on the device (Training/media_relations.jl `get_watch_order`, :174-197): W[a][b] = the number of users whose
// projected history (project_earliest, :156-172) has a before b.  A handle of its own (rsys_watch_order_*) holds one row band
// [row0, row1) of the dense V x V int32 matrix.  The pipeline of one add:
//   upload     offsets + items of a chunk of users through one pinned staging buffer, one copy; freed when the call returns
//   work       one wave per user: w[r] = L - 1 - i for the i-th item r of a user of L items when items[r] lies in the band, else 0
//              (rows outside the band drop out here, before any per-pair work); the host checked every item against [0, V)
//   scan       exclusive prefix P of w over the chunk (fixed-order three-pass scan), P[N] = the chunk's pair count T
//   count      the pairs form one flat index p in [0, T): pair p lies in the row r with P[r] <= p < P[r + 1], its column item is
//              items[r + 1 + p - P[r]].  Waves take slices of PAIR_SLICE consecutive pairs grid-stride, lane l pairs p0 + l + 64 k:
//              a long row spreads over every wave of the chip, short users pack many to a wave.  One no-return 32-bit global
//              atomic add per pair; integer adds do not depend on arrival order, so the matrix is bitwise reproducible.
// The band is stored with a row stride ld = V rounded up to 4, so that the CSR export reads every row with aligned 16-B loads; the
// padding columns are never added to.  Every element offset is 64-bit (a band can pass 2^32 elements).
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rsys.h"
#include "common.hpp"

namespace rsys {

namespace {

constexpr int WO_THREADS = 256;
constexpr int WO_SCAN_PER_THREAD = 16;
constexpr int WO_SCAN_CHUNK = WO_THREADS * WO_SCAN_PER_THREAD;   // elements per workgroup of the scan
constexpr long long WO_PAIR_SLICE = 64LL * 64;                   // pairs per wave slice of the count kernel (64 per lane)
constexpr long long WO_MAX_CHUNK_ITEMS = 1LL << 26;              // items per device chunk of an add (bounds the temporaries)
constexpr long long WO_FILL_CHUNK_NNZ = 1LL << 27;               // non-zeros per device chunk of the CSR fill

struct WatchOrder {
  int device = 0;
  long long V = 0, ld = 0, row0 = 0, row1 = 0;
  int* W = nullptr;                 // [row1 - row0][ld]
  hipStream_t stream = nullptr;
  long long users = 0;
  void* stage = nullptr;            // pinned staging buffer of the upload
  size_t stage_bytes = 0;
  long long rows() const { return row1 - row0; }
};

// ---- kernels

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// per-row pair work of a chunk: one wave per user (grid-stride)
__global__ void __launch_bounds__(WO_THREADS) wo_work_kernel(const long long* __restrict__ off, long long n_users, const int* __restrict__ items,
                                                             int row0, int row1, long long* __restrict__ w) {
  const long long waves = (long long)gridDim.x * (WO_THREADS / 64);
  for (long long u = (long long)blockIdx.x * (WO_THREADS / 64) + (threadIdx.x >> 6); u < n_users; u += waves) {
    const long long s = off[u], L = off[u + 1] - s;
    for (long long i = lane_id(); i < L; i += 64) {
      const int a = items[s + i];
      w[s + i] = (a >= row0 && a < row1) ? L - 1 - i : 0;
    }
  }
}

// scan pass 1: part[b] = sum of workgroup b's WO_SCAN_CHUNK elements
__global__ void __launch_bounds__(WO_THREADS) wo_scan_partial_kernel(const long long* __restrict__ x, long long n, long long* __restrict__ part) {
  __shared__ long long red[WO_THREADS / 64];
  const long long base = (long long)blockIdx.x * WO_SCAN_CHUNK + (long long)threadIdx.x * WO_SCAN_PER_THREAD;
  long long s = 0;
#pragma unroll
  for (int k = 0; k < WO_SCAN_PER_THREAD; ++k) s += base + k < n ? x[base + k] : 0;
  s = wave_sum_ll(s);
  if (lane_id() == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
    for (int i = 0; i < WO_THREADS / 64; ++i) t += red[i];
    part[blockIdx.x] = t;
  }
}

// exclusive scan of the values of the threads of one workgroup (fixed order); *total = the sum
__device__ long long block_exclusive_scan(long long v, long long* sm /* [blockDim.x] */, long long* total) {
  sm[threadIdx.x] = v;
  __syncthreads();
  for (unsigned o = 1; o < blockDim.x; o <<= 1) {
    const long long t = threadIdx.x >= o ? sm[threadIdx.x - o] : 0;
    __syncthreads();
    sm[threadIdx.x] += t;
    __syncthreads();
  }
  const long long incl = sm[threadIdx.x];
  *total = sm[blockDim.x - 1];
  __syncthreads();
  return incl - v;
}

// scan pass 2 (one workgroup of 1024): part[0..nb) -> exclusive prefixes in place, part[nb] = the total
__global__ void __launch_bounds__(1024) wo_scan_top_kernel(long long* part, long long nb) {
  __shared__ long long sm[1024];
  const long long per = (nb + 1023) / 1024, b0 = threadIdx.x * per, b1 = std::min(nb, b0 + per);
  long long s = 0;
  for (long long b = b0; b < b1; ++b) s += part[b];
  long long total;
  long long run = block_exclusive_scan(s, sm, &total);
  for (long long b = b0; b < b1; ++b) { const long long v = part[b]; part[b] = run; run += v; }
  if (threadIdx.x == 0) part[nb] = total;
}

// scan pass 3: x -> exclusive prefix in place (each thread holds its elements in registers before writing)
__global__ void __launch_bounds__(WO_THREADS) wo_scan_final_kernel(long long* x, long long n, const long long* __restrict__ part) {
  __shared__ long long sm[WO_THREADS];
  const long long base = (long long)blockIdx.x * WO_SCAN_CHUNK + (long long)threadIdx.x * WO_SCAN_PER_THREAD;
  long long v[WO_SCAN_PER_THREAD];
  long long s = 0;
#pragma unroll
  for (int k = 0; k < WO_SCAN_PER_THREAD; ++k) { v[k] = base + k < n ? x[base + k] : 0; s += v[k]; }
  long long total;
  long long run = part[blockIdx.x] + block_exclusive_scan(s, sm, &total);
#pragma unroll
  for (int k = 0; k < WO_SCAN_PER_THREAD; ++k) {
    if (base + k < n) x[base + k] = run;
    run += v[k];
  }
}

// the pair count: P[0..N] exclusive prefix of the row work (P[N] = T); pair p of row r adds 1 to W[items[r] - row0][items[r+1+p-P[r]]]
__global__ void __launch_bounds__(WO_THREADS) wo_pair_count_kernel(const long long* __restrict__ P, long long N, const int* __restrict__ items,
                                                                   int row0, long long ld, int* __restrict__ W) {
  const long long T = P[N];
  const long long n_slices = (T + WO_PAIR_SLICE - 1) / WO_PAIR_SLICE;
  const long long waves = (long long)gridDim.x * (WO_THREADS / 64);
  for (long long sl = (long long)blockIdx.x * (WO_THREADS / 64) + (threadIdx.x >> 6); sl < n_slices; sl += waves) {
    const long long p1 = std::min(T, (sl + 1) * WO_PAIR_SLICE);
    long long p = sl * WO_PAIR_SLICE + lane_id();
    if (p >= p1) continue;
    // the last row r with P[r] <= p (it has work: P[r + 1] > p)
    long long lo = 0, hi = N - 1;
    while (lo < hi) {
      const long long mid = (lo + hi + 1) >> 1;
      if (P[mid] <= p) lo = mid; else hi = mid - 1;
    }
    long long r = lo, pr = P[r], pn = P[r + 1];
    int* row = W + (long long)(items[r] - row0) * ld;
    for (; p < p1; p += 64) {
      if (pn <= p) {
        do { ++r; pr = pn; pn = P[r + 1]; } while (pn <= p);
        row = W + (long long)(items[r] - row0) * ld;
      }
      atomicAdd(row + items[r + 1 + (p - pr)], 1);
    }
  }
}

// out[k] = W[a[k] - row0][b[k]], one lane per pair (the host checked the ranges)
__global__ void wo_gather_kernel(const int* __restrict__ W, long long ld, int row0, long long n, const int* __restrict__ a,
                                 const int* __restrict__ b, int* __restrict__ out) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x)
    out[k] = W[(long long)(a[k] - row0) * ld + b[k]];
}

// non-zeros per row, one wave per row, 16-B loads (ld % 4 == 0)
__global__ void __launch_bounds__(WO_THREADS) wo_row_nnz_kernel(const int* __restrict__ W, long long rows, long long ld, long long* __restrict__ cnt) {
  const long long waves = (long long)gridDim.x * (WO_THREADS / 64);
  for (long long r = (long long)blockIdx.x * (WO_THREADS / 64) + (threadIdx.x >> 6); r < rows; r += waves) {
    const int4* row = (const int4*)(W + r * ld);
    long long c = 0;
    for (long long k = lane_id(); k < ld / 4; k += 64) {
      const int4 v = row[k];
      c += (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0);
    }
    c = wave_sum_ll(c);
    if (lane_id() == 0) cnt[r] = c;
  }
}

// CSR fill of rows [r0, r1): row r's non-zeros in column order at indptr[r] - base, one wave per row
__global__ void __launch_bounds__(WO_THREADS) wo_fill_kernel(const int* __restrict__ W, long long r0, long long r1, long long ld,
                                                             const long long* __restrict__ indptr, long long base, int* __restrict__ idx,
                                                             int* __restrict__ val) {
  const long long waves = (long long)gridDim.x * (WO_THREADS / 64);
  const int lane = lane_id();
  for (long long r = r0 + (long long)blockIdx.x * (WO_THREADS / 64) + (threadIdx.x >> 6); r < r1; r += waves) {
    const int4* row = (const int4*)(W + r * ld);
    long long at = indptr[r] - base;
    for (long long k0 = 0; k0 < ld / 4; k0 += 64) {
      const long long k = k0 + lane;
      int4 v = k < ld / 4 ? row[k] : make_int4(0, 0, 0, 0);
      const int c = (v.x != 0) + (v.y != 0) + (v.z != 0) + (v.w != 0);
      int incl = c;   // inclusive scan over lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      long long q = at + incl - c;
      const int vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (vv[e] != 0) { idx[q] = (int)(4 * k + e); val[q] = vv[e]; ++q; }
      at += __shfl(incl, 63, 64);
    }
  }
}

// ---- host side

int grid_for(long long work_units_per_block_of_waves, int cap_per_cu = 8) {
  const long long g = std::max<long long>(1, work_units_per_block_of_waves);
  return (int)std::min<long long>(g, (long long)cu_count() * cap_per_cu);
}

// in-place exclusive scan of x[0..n) on the stream; x[n] = the total (x holds n + 1 elements); part holds >= nb + 1
int exclusive_scan(long long* x, long long n, long long* part, hipStream_t s) {
  const long long nb = std::max<long long>(1, (n + WO_SCAN_CHUNK - 1) / WO_SCAN_CHUNK);
  wo_scan_partial_kernel<<<(unsigned)nb, WO_THREADS, 0, s>>>(x, n, part);
  wo_scan_top_kernel<<<1, 1024, 0, s>>>(part, nb);
  wo_scan_final_kernel<<<(unsigned)nb, WO_THREADS, 0, s>>>(x, n, part);
  HIP_CHECK(hipMemcpyAsync(x + n, part + nb, 8, hipMemcpyDeviceToDevice, s));
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

long long scan_parts(long long n) { return std::max<long long>(1, (n + WO_SCAN_CHUNK - 1) / WO_SCAN_CHUNK) + 1; }

struct DevBufs {   // temporaries of one call, freed on every return path
  std::vector<void*> p;
  ~DevBufs() { for (void* q : p) hipFree(q); }
  int alloc(void** out, size_t bytes) {
    *out = nullptr;
    HIP_CHECK(hipMalloc(out, std::max<size_t>(bytes, 16)));
    p.push_back(*out);
    return RSYS_OK;
  }
};
#define WO_RC(expr) do { int _rc = (expr); if (_rc != RSYS_OK) return _rc; } while (0)

int stage_reserve(WatchOrder* h, size_t bytes) {
  if (bytes <= h->stage_bytes) return RSYS_OK;
  if (h->stage) HIP_CHECK(hipHostFree(h->stage));
  h->stage = nullptr; h->stage_bytes = 0;
  HIP_CHECK(hipHostMalloc(&h->stage, bytes, hipHostMallocDefault));
  h->stage_bytes = bytes;
  return RSYS_OK;
}

void wo_free(WatchOrder* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->W) hipFree(h->W);
  if (h->stage) hipHostFree(h->stage);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

int wo_create(int64_t V, int64_t row0, int64_t row1, int32_t device, void** out) {
  ARG_CHECK(out, "rsys_watch_order_create: null output");
  ARG_CHECK(V >= 1 && V <= (1LL << 30), "rsys_watch_order_create: 1 <= V <= 2^30");
  ARG_CHECK(row0 >= 0 && row0 <= row1 && row1 <= V, "rsys_watch_order_create: the band [row0, row1) must lie in [0, V]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("rsys_watch_order_create: no HIP device visible"); return RSYS_ERR_HIP; }
  ARG_CHECK(device >= 0 && device < ndev, "rsys_watch_order_create: device index out of range");
  HIP_CHECK(hipSetDevice(device));
  const long long ld = (V + 3) / 4 * 4;
  const size_t bytes = (size_t)(row1 - row0) * (size_t)ld * 4;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  if (bytes + (64ull << 20) > free_b) {
    set_error("rsys_watch_order_create: the band needs " + std::to_string(bytes) + " bytes of device memory, " + std::to_string(free_b) +
              " are free (cap the band: fewer rows per handle)");
    return RSYS_ERR_STATE;
  }
  WatchOrder* h = new WatchOrder();
  h->device = device; h->V = V; h->ld = ld; h->row0 = row0; h->row1 = row1;
  const int rc = [&]() -> int {
    HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    if (hipMalloc((void**)&h->W, std::max<size_t>(bytes, 16)) != hipSuccess) {
      h->W = nullptr;
      hipGetLastError();
      set_error("rsys_watch_order_create: allocating the band of " + std::to_string(bytes) + " bytes failed");
      return RSYS_ERR_STATE;
    }
    HIP_CHECK(hipMemsetAsync(h->W, 0, std::max<size_t>(bytes, 16), h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    return RSYS_OK;
  }();
  if (rc != RSYS_OK) { wo_free(h); return rc; }
  *out = h;
  return RSYS_OK;
}

// one chunk of users [u0, u1) of a validated batch
int wo_add_chunk(WatchOrder* h, const int64_t* offsets, const int32_t* items, long long u0, long long u1) {
  const long long n = u1 - u0, N = offsets[u1] - offsets[u0];
  if (N == 0) return RSYS_OK;
  hipStream_t s = h->stream;
  // pinned staging: rebased offsets [n + 1] int64, then items [N] int32
  const size_t off_b = (size_t)(n + 1) * 8, bytes = off_b + (size_t)N * 4;
  WO_RC(stage_reserve(h, bytes));
  long long* so = (long long*)h->stage;
  for (long long u = 0; u <= n; ++u) so[u] = offsets[u0 + u] - offsets[u0];
  memcpy((char*)h->stage + off_b, items + offsets[u0], (size_t)N * 4);
  DevBufs tmp;
  void *d_blob, *d_P, *d_part;
  WO_RC(tmp.alloc(&d_blob, bytes));
  WO_RC(tmp.alloc(&d_P, (size_t)(N + 1) * 8));
  WO_RC(tmp.alloc(&d_part, (size_t)scan_parts(N) * 8));
  HIP_CHECK(hipMemcpyAsync(d_blob, h->stage, bytes, hipMemcpyHostToDevice, s));
  const long long* d_off = (const long long*)d_blob;
  const int* d_items = (const int*)((char*)d_blob + off_b);
  long long* P = (long long*)d_P;
  wo_work_kernel<<<grid_for((n + 3) / 4, 16), WO_THREADS, 0, s>>>(d_off, n, d_items, (int)h->row0, (int)h->row1, P);
  HIP_CHECK(hipGetLastError());
  WO_RC(exclusive_scan(P, N, (long long*)d_part, s));
  long long T = 0;
  HIP_CHECK(hipMemcpyAsync(&T, P + N, 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));   // (also frees the staging buffer for the next chunk)
  if (T > 0) {
    const long long slices = (T + WO_PAIR_SLICE - 1) / WO_PAIR_SLICE;
    wo_pair_count_kernel<<<grid_for((slices + 3) / 4, 8), WO_THREADS, 0, s>>>(P, N, d_items, (int)h->row0, h->ld, h->W);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
  }
  return RSYS_OK;
}

int wo_add(WatchOrder* h, int64_t n_users, const int64_t* offsets, const int32_t* items) {
  ARG_CHECK(n_users >= 0, "rsys_watch_order_add: n_users >= 0");
  if (n_users == 0) return RSYS_OK;
  ARG_CHECK(offsets, "rsys_watch_order_add: null offsets");
  ARG_CHECK(offsets[0] == 0, "rsys_watch_order_add: offsets[0] must be 0");
  long long nonempty = 0;
  for (long long u = 0; u < n_users; ++u) {
    ARG_CHECK(offsets[u + 1] >= offsets[u], "rsys_watch_order_add: offsets must be non-decreasing");
    nonempty += offsets[u + 1] > offsets[u];
  }
  ARG_CHECK(items || offsets[n_users] == 0, "rsys_watch_order_add: null items");
  ARG_CHECK(h->users + nonempty <= 2147483647LL, "rsys_watch_order_add: the user count would pass 2^31 - 1 (int32 counts)");
  // items: checked on the host before any count is added, so a rejected batch leaves the matrix as it was
  const long long N = offsets[n_users];
  for (long long k = 0; k < N; ++k) ARG_CHECK(items[k] >= 0 && items[k] < h->V, "rsys_watch_order_add: an item lies outside [0, V)");
  HIP_CHECK(hipSetDevice(h->device));
  // chunks of whole users of at most WO_MAX_CHUNK_ITEMS items (a longer user alone)
  long long u0 = 0;
  while (u0 < n_users) {
    long long u1 = u0 + 1;
    while (u1 < n_users && offsets[u1 + 1] - offsets[u0] <= WO_MAX_CHUNK_ITEMS) ++u1;
    WO_RC(wo_add_chunk(h, offsets, items, u0, u1));
    u0 = u1;
  }
  h->users += nonempty;
  return RSYS_OK;
}

int wo_rows_get(WatchOrder* h, int64_t row0, int64_t n_rows, int32_t* out) {
  ARG_CHECK(n_rows >= 0 && row0 >= h->row0 && row0 + n_rows <= h->row1, "rsys_watch_order_rows_get: rows outside the band");
  if (n_rows == 0) return RSYS_OK;
  ARG_CHECK(out, "rsys_watch_order_rows_get: null output");
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipMemcpy2D(out, (size_t)h->V * 4, h->W + (row0 - h->row0) * h->ld, (size_t)h->ld * 4, (size_t)h->V * 4, (size_t)n_rows,
                        hipMemcpyDeviceToHost));
  return RSYS_OK;
}

int wo_gather(WatchOrder* h, int64_t n, const int32_t* a, const int32_t* b, int32_t* out) {
  ARG_CHECK(n >= 0, "rsys_watch_order_gather: n >= 0");
  if (n == 0) return RSYS_OK;
  ARG_CHECK(a && b && out, "rsys_watch_order_gather: null buffer");
  for (long long k = 0; k < n; ++k) {
    ARG_CHECK(a[k] >= h->row0 && a[k] < h->row1, "rsys_watch_order_gather: a row outside the band");
    ARG_CHECK(b[k] >= 0 && b[k] < h->V, "rsys_watch_order_gather: a column outside [0, V)");
  }
  HIP_CHECK(hipSetDevice(h->device));
  DevBufs tmp;
  void* d;
  WO_RC(tmp.alloc(&d, (size_t)n * 12));
  int* da = (int*)d;
  HIP_CHECK(hipMemcpyAsync(da, a, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(hipMemcpyAsync(da + n, b, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  wo_gather_kernel<<<grid_for((n + 255) / 256, 16), 256, 0, h->stream>>>(h->W, h->ld, (int)h->row0, n, da, da + n, da + 2 * n);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(out, da + 2 * n, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  return RSYS_OK;
}

int wo_csr(WatchOrder* h, int64_t* indptr, int32_t* indices, int32_t* values, int64_t cap, int64_t* nnz) {
  ARG_CHECK(nnz, "rsys_watch_order_csr: null nnz");
  HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const long long R = h->rows();
  DevBufs tmp;
  void *d_ptr, *d_part;
  WO_RC(tmp.alloc(&d_ptr, (size_t)(R + 1) * 8));
  WO_RC(tmp.alloc(&d_part, (size_t)scan_parts(R) * 8));
  long long* ptr = (long long*)d_ptr;
  if (R > 0) {
    wo_row_nnz_kernel<<<grid_for((R + 3) / 4, 16), WO_THREADS, 0, s>>>(h->W, R, h->ld, ptr);
    HIP_CHECK(hipGetLastError());
    WO_RC(exclusive_scan(ptr, R, (long long*)d_part, s));
  } else {
    HIP_CHECK(hipMemsetAsync(ptr, 0, 8, s));
  }
  std::vector<long long> hp((size_t)R + 1);
  HIP_CHECK(hipMemcpyAsync(hp.data(), ptr, (size_t)(R + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  const long long total = hp[(size_t)R];
  *nnz = total;
  if (!indptr || !indices || !values || cap < total) return RSYS_OK;
  memcpy(indptr, hp.data(), (size_t)(R + 1) * 8);
  // fill in chunks of whole rows of at most WO_FILL_CHUNK_NNZ non-zeros (a denser row alone)
  long long r0 = 0;
  void* d_iv = nullptr;
  long long iv_cap = 0;
  while (r0 < R) {
    long long r1 = r0 + 1;
    while (r1 < R && hp[(size_t)r1 + 1] - hp[(size_t)r0] <= WO_FILL_CHUNK_NNZ) ++r1;
    const long long cn = hp[(size_t)r1] - hp[(size_t)r0];
    if (cn > 0) {
      if (cn > iv_cap) {
        WO_RC(tmp.alloc(&d_iv, (size_t)cn * 8));
        iv_cap = cn;
      }
      int* di = (int*)d_iv;
      int* dv = di + iv_cap;
      wo_fill_kernel<<<grid_for((r1 - r0 + 3) / 4, 16), WO_THREADS, 0, s>>>(h->W, r0, r1, h->ld, ptr, hp[(size_t)r0], di, dv);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(indices + hp[(size_t)r0], di, (size_t)cn * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipMemcpyAsync(values + hp[(size_t)r0], dv, (size_t)cn * 4, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
    r0 = r1;
  }
  return RSYS_OK;
}

int wo_clear(WatchOrder* h) {
  HIP_CHECK(hipSetDevice(h->device));
  HIP_CHECK(hipMemsetAsync(h->W, 0, std::max<size_t>((size_t)h->rows() * (size_t)h->ld * 4, 16), h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  h->users = 0;
  return RSYS_OK;
}

}  // namespace

}  // namespace rsys

using namespace rsys;

#define WO_HANDLE(hv)                                                           \
  WatchOrder* h = (WatchOrder*)(hv);                                            \
  do {                                                                          \
    if (h == nullptr) { set_error("null handle"); return RSYS_ERR_ARG; }        \
  } while (0)

extern "C" {

int32_t rsys_watch_order_create(int64_t V, int64_t row0, int64_t row1, int32_t device, void** out) { return wo_create(V, row0, row1, device, out); }
int32_t rsys_watch_order_destroy(void* hv) { wo_free((WatchOrder*)hv); return RSYS_OK; }
int32_t rsys_watch_order_add(void* hv, int64_t n_users, const int64_t* offsets, const int32_t* items) {
  WO_HANDLE(hv); return wo_add(h, n_users, offsets, items);
}
int32_t rsys_watch_order_users(void* hv, int64_t* out) {
  WO_HANDLE(hv); ARG_CHECK(out, "rsys_watch_order_users: null output"); *out = h->users; return RSYS_OK;
}
int32_t rsys_watch_order_rows_get(void* hv, int64_t row0, int64_t n_rows, int32_t* out) { WO_HANDLE(hv); return wo_rows_get(h, row0, n_rows, out); }
int32_t rsys_watch_order_gather(void* hv, int64_t n, const int32_t* a, const int32_t* b, int32_t* out) { WO_HANDLE(hv); return wo_gather(h, n, a, b, out); }
int32_t rsys_watch_order_csr(void* hv, int64_t* indptr, int32_t* indices, int32_t* values, int64_t cap, int64_t* nnz) {
  WO_HANDLE(hv); return wo_csr(h, indptr, indices, values, cap, nnz);
}
int32_t rsys_watch_order_clear(void* hv) { WO_HANDLE(hv); return wo_clear(h); }

}  // extern "C"
