// Row movers: whole rows copied or added between buffers through an index (heads, compact top, sharded table, page pipeline).
//
// One kernel, one wave per row, 16-byte chunks, lane l takes chunks l, l + 64, ...; 256 threads = four rows per workgroup.  Row r
// has a "near" row (r itself) and a "far" row that an index policy looks up; the operation says which way the bytes go:
//   GATHER   dst[r]    = src[far]   (zeros where there is no far row)
//   SCATTER  dst[far]  = src[r]
//   ADD      dst[far] += src[r]     (fp32; skipped where there is no far row; the far rows of one launch are distinct)
// The twelve forms (launchers below) with their live rows and far rows: DESIGN 7a.
// The near side has row stride D, the far side `ld`; scatter_rows_fill is the exception (a gather whose near side is the strided one).
// Sel and Fill stay apart from Plain: their live range comes from device data of another shape (a padded count, a count per batch row).
#include "kernels.hpp"

namespace rsys {

namespace {

// head rows: far = token 2 idx[r] + parity, or that token's compact row (SLOT; -1 = not in the set)
template <bool SLOT, bool COUNT>
struct Head {
  static constexpr bool kNone = SLOT;
  const int *idx, *slot, *count; int parity, n;
  __device__ bool at(long long r, long long& far) const {
    if (r >= n || (COUNT && r >= *count)) return false;   // (rows from *count on are zero-weight padding: their gradient is zero)
    far = 2LL * idx[r] + parity;
    if (SLOT) far = slot[far];
    return true;
  }
};
// far = base + idx[r]; a negative idx[r] names no row (a dropped entry).  Rows by id: base = -sub, ids never below sub.
template <bool COUNT>
struct Plain {
  static constexpr bool kNone = true;
  const int *idx, *count; int base, n;
  __device__ bool at(long long r, long long& far) const {
    if (r >= n || (COUNT && r >= *count)) return false;
    const int i = idx[r];
    far = i >= 0 ? base + i : -1;
    return true;
  }
};
// compact rows [0, *n) <- rows sel[r]; rows [*n, pad256(*n)) clipped at cap <- 0 (the GEMMs that read them stop at a tile edge)
struct Sel {
  static constexpr bool kNone = true;
  const int *sel, *n_dev; int cap;
  __device__ bool at(long long r, long long& far) const {
    const int n = *n_dev;
    if (r >= min(cap, (n + 255) & ~255)) return false;
    far = r < n ? sel[r] : -1;
    return true;
  }
};
// place p of batch row b, p < 64 q_active[b] (the query tiles the last layer's attention backward visits) <- compact row slot_p[place],
// zeros where the place holds no selected token; places beyond the visited tiles are never read and keep what they held
struct Fill {
  static constexpr bool kNone = true;
  const int *slot_p, *q_active; int Tseq; long long places;
  __device__ bool at(long long r, long long& far) const {
    if (r >= places) return false;
    const int b = (int)(r / Tseq), pp = (int)(r - (long long)b * Tseq);
    if (pp >= 64 * q_active[b]) return false;
    far = slot_p[r];
    return true;
  }
};

enum Op { GATHER, SCATTER, ADD };

template <typename T>
__device__ void copy_row(const T* s, bool none, T* d, int D, int l) {   // none: zeros, s is not read
  constexpr int E = 16 / sizeof(T);
  uint4* d4 = (uint4*)d;
  if (!none) {
    const uint4* s4 = (const uint4*)s;
    for (int c = l; c < D / E; c += 64) d4[c] = s4[c];
  } else {
    for (int c = l; c < D / E; c += 64) d4[c] = make_uint4(0, 0, 0, 0);
  }
}
__device__ void add_row(const float* s, float* d, int D, int l) {
  const float4* s4 = (const float4*)s;
  float4* d4 = (float4*)d;
  for (int c = l; c < D / 4; c += 64) {
    float4 a = d4[c]; const float4 b = s4[c];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    d4[c] = a;
  }
}

template <typename T, Op OP, typename P>
__global__ void row_mover_kernel(P p, const T* __restrict__ src, long long sld, T* dst, long long dld, int D) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int l = threadIdx.x & 63;
  long long far;
  if (!p.at(r, far)) return;
  const bool none = P::kNone && far < 0;   // compile-time false for the policies that always name a row
  if constexpr (OP == GATHER) copy_row<T>(none ? src : src + far * sld, none, dst + r * dld, D, l);
  else if (none) return;
  else if constexpr (OP == SCATTER) copy_row<T>(src + r * sld, false, dst + far * dld, D, l);
  else add_row(src + r * sld, dst + far * dld, D, l);
}

// rows: the bound the grid covers (ceil(rows / 4) workgroups); none: nothing to do
template <typename T, Op OP, typename P>
int launch_rows(P p, long long rows, const T* src, long long sld, T* dst, long long dld, int D, hipStream_t s) {
  ARG_CHECK((D * sizeof(T)) % 16 == 0 && (sld * sizeof(T)) % 16 == 0 && (dld * sizeof(T)) % 16 == 0, "row movers: rows and row strides must be 16-byte multiples");
  ARG_CHECK(rows >= 0, "row movers: a negative row count");
  if (rows == 0) return RSYS_OK;
  hipLaunchKernelGGL((row_mover_kernel<T, OP, P>), dim3(div_up(rows, 4)), dim3(256), 0, s, p, src, sld, dst, dld, D);
  HIP_CHECK(hipGetLastError());
  return RSYS_OK;
}

}  // namespace

template <typename T>
int launch_gather_rows(const T* src, long long ld, const int* idx, int parity, T* dst, int n, int D, hipStream_t s) {
  return launch_rows<T, GATHER>(Head<false, false>{idx, nullptr, nullptr, parity, n}, n, src, ld, dst, D, D, s);
}
int launch_scatter_rows_add(const float* src, const int* idx, int parity, float* dst, long long ld, int n, int D, hipStream_t s, const int* npos) {
  if (npos != nullptr) return launch_rows<float, ADD>(Head<false, true>{idx, nullptr, npos, parity, n}, n, src, D, dst, ld, D, s);
  return launch_rows<float, ADD>(Head<false, false>{idx, nullptr, nullptr, parity, n}, n, src, D, dst, ld, D, s);
}
template <typename T>
int launch_gather_rows_slot(const T* compact, const int* slot, const int* idx, int parity, T* dst, int n, int D, hipStream_t s) {
  return launch_rows<T, GATHER>(Head<true, false>{idx, slot, nullptr, parity, n}, n, compact, D, dst, D, D, s);
}
int launch_scatter_rows_add_slot(const float* src, const int* slot, const int* idx, int parity, const int* npos, float* compact, int n, int D,
                                 hipStream_t s) {
  return launch_rows<float, ADD>(Head<true, true>{idx, slot, npos, parity, n}, n, src, D, compact, D, D, s);
}
template <typename T>
int launch_gather_rows_sel(const T* src, long long ld, const int* sel, const int* n_dev, int cap, T* dst, int D, hipStream_t s) {
  return launch_rows<T, GATHER>(Sel{sel, n_dev, cap}, cap, src, ld, dst, D, D, s);
}
template <typename T>
int launch_scatter_rows_fill(const T* src, const int* slot_p, const int* q_active, int B, int Tseq, T* dst, long long ld, int D, hipStream_t s) {
  const long long places = (long long)B * Tseq;
  return launch_rows<T, GATHER>(Fill{slot_p, q_active, Tseq, places}, places, src, D, dst, ld, D, s);
}
template <typename T>
int launch_scatter_rows_map(const T* src, const int* map, int n, T* dst, long long ld, int D, hipStream_t s) {
  return launch_rows<T, SCATTER>(Plain<false>{map, nullptr, 0, n}, n, src, D, dst, ld, D, s);
}
template <typename T>
int launch_gather_rows_plain(const T* src, long long ld, const int* idx, int base, T* dst, int n, int D, hipStream_t s) {
  return launch_rows<T, GATHER>(Plain<false>{idx, nullptr, base, n}, n, src, ld, dst, D, D, s);
}
int launch_add_rows_plain(const float* src, const int* idx, int base, float* dst, long long ld, int n, int D, hipStream_t s) {
  return launch_rows<float, ADD>(Plain<false>{idx, nullptr, base, n}, n, src, D, dst, ld, D, s);
}
int launch_gather_rows_by_id(const float* src, long long ld, const int* ids, int sub, float* dst, int n, int D, hipStream_t s) {
  return launch_gather_rows_plain<float>(src, ld, ids, -sub, dst, n, D, s);
}
int launch_add_rows_by_id(const float* src, const int* ids, int sub, float* dst, long long ld, int n, int D, hipStream_t s) {
  return launch_add_rows_plain(src, ids, -sub, dst, ld, n, D, s);
}
int launch_add_rows_by_id_counted(const float* src, const int* ids, const int* count_dev, float* dst, long long ld, int cap, int D, hipStream_t s) {
  return launch_rows<float, ADD>(Plain<true>{ids, count_dev, 0, cap}, cap, src, D, dst, ld, D, s);
}

#define INST(T)                                                                                                             \
  template int launch_gather_rows<T>(const T*, long long, const int*, int, T*, int, int, hipStream_t);                       \
  template int launch_gather_rows_slot<T>(const T*, const int*, const int*, int, T*, int, int, hipStream_t);                 \
  template int launch_gather_rows_sel<T>(const T*, long long, const int*, const int*, int, T*, int, hipStream_t);            \
  template int launch_scatter_rows_fill<T>(const T*, const int*, const int*, int, int, T*, long long, int, hipStream_t);     \
  template int launch_scatter_rows_map<T>(const T*, const int*, int, T*, long long, int, hipStream_t);                       \
  template int launch_gather_rows_plain<T>(const T*, long long, const int*, int, T*, int, int, hipStream_t);
INST(bf16)
INST(float)
#undef INST

}  // namespace rsys
